"""The checker of the λ models checks itself: the Float64 restatement of src/models/filter.jl
(tests/msed_reference.py) against its 40-digit twin, and the reference's quirks, one assertion each."""
from __future__ import annotations

import numpy as np
import pytest

import msed_reference as R
from yfm_amd import synthetic as S

REL = 1e-11


@pytest.fixture(scope="module")
def panel():
    mats = S.maturities_30()[::3]  # N = 10
    return mats, S.simulate_panel(R.KIND_SD_NS, 24, maturities=mats)


@pytest.mark.parametrize("kind", R.KINDS)
def test_float_restatement_matches_truth(panel, kind):
    mats, Y = panel
    Th = S.theta_batch(kind, 8, scale=0.1, seed=100 + kind, bad_frac=0.0)
    worst = 0.0
    for b in range(8):
        f = R.get_loss(kind, mats, Y, Th[:, b], 0, R.FLOAT)
        t = R.get_loss(kind, mats, Y, Th[:, b], 0, R.TRUTH)
        assert np.isfinite(f) and np.isfinite(t)
        worst = max(worst, abs(f - t) / abs(t))
    print("kind", kind, "max rel", worst)
    assert worst <= REL


def _theta_c(kind):
    return S.theta0_constrained(kind)


def test_nan_in_second_maturity_gives_minus_inf(panel):
    mats, Y = panel
    Yn = Y.copy(order="F")
    Yn[1, 7] = np.nan
    for kind in R.KINDS:
        assert R.get_loss(kind, mats, Yn, _theta_c(kind)) == -np.inf


def test_nan_in_first_maturity_is_a_prediction_only_step(panel):
    mats, Y = panel
    Yn = Y.copy(order="F")
    Yn[0, 7] = np.nan
    for kind in R.KINDS:
        th = _theta_c(kind)
        # windows that stop before column 8 never compare it: the values of the clean panel
        assert R.get_loss(kind, mats, Yn, th, T_use=7) == pytest.approx(R.get_loss(kind, mats, Y, th, T_use=7), rel=1e-13)
        # −Inf as soon as the column is compared
        assert R.get_loss(kind, mats, Yn, th, T_use=8) == -np.inf
        # the step itself only predicts: β ← μ + Φβ, γ ← ν + Bγ, the score average untouched
        m = R.set_params(kind, th, mats)
        for t in range(7):
            R.filter_step(m, Yn[:, t])
        beta, gamma, count = m.beta.copy(), m.gamma, m.count
        pred = R.filter_step(m, Yn[:, 7])
        np.testing.assert_array_equal(m.beta, m.mu + m.Phi @ beta)
        assert m.gamma == (m.nu + m.B * gamma if m.B is not None else gamma)
        assert m.count == count
        assert np.all(np.isfinite(pred))
    # a first column without its first maturity is never compared: finite
    Y0 = Y.copy(order="F")
    Y0[0, 0] = np.nan
    assert np.isfinite(R.get_loss(R.KIND_SD_NS, mats, Y0, _theta_c(R.KIND_SD_NS)))


def test_one_column_window_gives_zero(panel):
    mats, Y = panel
    for kind in R.KINDS:
        assert R.get_loss(kind, mats, Y, _theta_c(kind), T_use=1) == 0.0


def test_divisor_is_nobs(panel):
    mats, Y = panel
    kind = R.KIND_SD_NS
    arr = R.get_loss_array(kind, mats, Y, _theta_c(kind), T_use=12)
    assert arr.shape == (11,)
    assert R.get_loss(kind, mats, Y, _theta_c(kind), T_use=12) == pytest.approx(arr.sum() / 12, rel=1e-14)


def test_first_entry_of_the_loss_array_is_a_real_value(panel):
    mats, Y = panel
    for kind in R.KINDS:
        assert R.get_loss_array(kind, mats, Y, _theta_c(kind))[0] < 0.0


def test_ewma_resets_between_calls(panel):
    mats, Y = panel
    kind = R.KIND_SSD_NS
    m = R.set_params(kind, _theta_c(kind), mats)
    first = [R.filter_step(m, Y[:, t]) for t in range(5)]
    assert m.count == 5 and m.ewma > 0.0
    m2 = R.set_params(kind, _theta_c(kind), mats)  # what the next get_loss call starts from
    assert m2.count == 0 and m2.ewma == 0.0
    again = [R.filter_step(m2, Y[:, t]) for t in range(5)]
    np.testing.assert_array_equal(np.array(first), np.array(again))
    R.initialize_filter(m)
    assert m.count == 0 and m.ewma == 0.0
    assert R.get_loss(kind, mats, Y, _theta_c(kind)) == R.get_loss(kind, mats, Y, _theta_c(kind))


def test_trial_grid_order():
    """get_new_initial_params: B cycles fastest, 30 trials with B and 6 without, None past the last."""
    p = np.zeros(15)
    assert R.trial_params(R.KIND_SD_NS, p, 1)[:2].tolist() == [1e-6, 0.9]
    assert R.trial_params(R.KIND_SD_NS, p, 7)[:2].tolist() == [1e-5, 0.95]
    assert R.trial_params(R.KIND_SD_NS, p, 30)[:2].tolist() == [1e-1, 0.999]
    assert R.trial_params(R.KIND_SD_NS, p, 31) is None
    assert R.trial_params(R.KIND_RWSD_NS, np.zeros(14), 6)[0] == 1e-1
    assert R.trial_params(R.KIND_RWSD_NS, np.zeros(14), 7) is None
