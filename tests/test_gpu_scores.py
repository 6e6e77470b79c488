"""GPU tests of the DNS score series (csrc/yfm_score.hip dns_score_kernel through yfm_loglik_scores_batch).

S[d, k, b] = ∂ℓ_k/∂θ_d, ℓ_k the term get_loss adds after column k (0-based), for 1 ≤ k ≤ T_use_b − 2 and exactly 0.0
elsewhere (include/yfm.h).  The checks:

  telescoping   S[:, k, b] = grad(T_use = k+2) − grad(T_use = k+1) of the shipped gradient kernel, within
                1e-9·max(‖g‖∞) of the two windows (the project's gradient bar: both sides are FP64 kernels that meet it)
  sum rule      |Σ_k S[d, k, b] − grad[d, b]| ≤ 4·T·2⁻⁵³·Σ_k |S[d, k, b]| (the bound of a sum taken in another order)
  truth         on tests/golden/info/info_cases.npz (make_info.py: nested windows of the binary128 difference
                gradient), max |S − s_truth| ≤ 1e-9·‖g_fd‖∞ + e_fd per candidate
  mapping       partial blocks, batch independence to the bit, one-term and no-term windows, a deferred candidate,
                the device entry point on a side stream, the refusals.
"""
from __future__ import annotations

import ctypes
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_device_entry_matches
from yfm_amd import KIND_DNS, KIND_GNS, KIND_TVL, _lib
from yfm_amd import synthetic as S
from yfm_amd.params import KIND_NNS, KIND_SD_NS, n_params, transform_params

sys.path.insert(0, str(GOLDEN / "grad"))
sys.path.insert(0, str(GOLDEN / "info"))
import make_grad_long as MGL  # noqa: E402
import make_info as MI  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-9
U = 2.0 ** -53


@pytest.fixture(scope="module")
def small():
    """T = 12, N = 10, column 4 all NaN, 5 candidates on the windows 1, 2, 3, 7, 12."""
    m = S.maturities_30()[::3]
    Y = S.simulate_panel(KIND_DNS, 12, m, 31).copy()
    Y[:, 4] = np.nan
    Th = S.theta_batch(KIND_DNS, 5, 0.1, 32, bad_frac=0)
    return Y, m, Th, np.array([1, 2, 3, 7, 12], dtype=np.int32)


@pytest.fixture(scope="module")
def cases():
    return MI.load_cases()


def window_grads(engine, Th, space, T):
    """g[P, w, b]: the shipped gradient kernel on the window of w + 1 columns, w = 0 … T − 1."""
    P, B = Th.shape
    X = np.asfortranarray(np.repeat(Th, T, axis=1))
    _, g = engine.loglik_grad(KIND_DNS, X, space=space, T_use=np.tile(np.arange(1, T + 1, dtype=np.int32), B))
    return g.reshape(P, B, T).transpose(0, 2, 1)


@pytest.mark.parametrize("space", [0, 1])
def test_scores_telescope_the_gradient_and_sum_to_it(engine, small, space):
    Y, m, Th, tu = small
    T = Y.shape[1]
    X = Th if space == 0 else transform_params(KIND_DNS, Th)
    engine.set_panel(Y, m)
    ll, Sc = engine.loglik_scores(KIND_DNS, X, space=space, T_use=tu)
    assert Sc.shape == (20, T - 1, 5) and engine.last_grad_unavailable() == 0
    np.testing.assert_array_equal(ll, engine.loglik(KIND_DNS, X, space=space, T_use=tu))
    gw = window_grads(engine, X, space, T)
    worst = 0.0
    for b in range(5):
        for k in range(T - 1):
            if 1 <= k <= tu[b] - 2:
                hi, lo = gw[:, k + 1, b], gw[:, k, b]  # the windows of k + 2 and k + 1 columns
                tol = REL * max(np.abs(hi).max(), np.abs(lo).max())
                err = np.abs(Sc[:, k, b] - (hi - lo)).max()
                worst = max(worst, err / tol)
                assert err <= tol, (b, k, err, tol)
            else:
                assert np.all(Sc[:, k, b] == 0.0), (b, k)
    # the sum rule against the whole window's gradient
    _, g = engine.loglik_grad(KIND_DNS, X, space=space, T_use=tu)
    gap = np.abs(Sc.sum(axis=1) - g)
    bound = 4 * T * U * np.abs(Sc).sum(axis=1)
    print(f"space {space}: telescoping worst err/tol {worst:.3e}; sum rule worst gap/bound "
          f"{np.max(gap[bound > 0] / bound[bound > 0]):.3e}")
    assert np.all(gap <= bound), np.argwhere(gap > bound)


@pytest.mark.parametrize("name", MI.SCORE_CASES)
def test_scores_match_truth_differences(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    ll, Sc = engine.loglik_scores(KIND_DNS, c["Theta"], space=0)
    err = np.abs(Sc - c["s_truth"]).max(axis=(0, 1))
    gn = np.abs(c["g_fd"]).max(axis=0)
    bound = REL * gn + c["e_fd"]
    print(f"case {name}: max err/bound {np.max(err / bound):.3e}, max err/|g| {np.max(err / gn):.3e}")
    assert np.all(err <= bound), err / bound
    assert np.all(Sc[:, 0, :] == 0.0)
    np.testing.assert_allclose(ll, c["loglik_truth"], rtol=REL)


def test_partial_blocks_and_batch_independence(engine, small):
    """33 candidates (one block of 32 and one more) against B = 1 and a reversed batch: the same bits."""
    Y, m, _, _ = small
    T = Y.shape[1]
    engine.set_panel(Y, m)
    Th = S.theta_batch(KIND_DNS, 33, 0.1, 33, bad_frac=0)
    tu = np.array([(3 + 5 * b) % T + 1 for b in range(33)], dtype=np.int32)
    ll, Sc = engine.loglik_scores(KIND_DNS, Th, T_use=tu)
    llr, Sr = engine.loglik_scores(KIND_DNS, Th[:, ::-1], T_use=tu[::-1])
    np.testing.assert_array_equal(Sr[:, :, ::-1], Sc)
    np.testing.assert_array_equal(llr[::-1], ll)
    for b in (0, 7, 31, 32):
        l1, S1 = engine.loglik_scores(KIND_DNS, Th[:, b], T_use=tu[b:b + 1])
        np.testing.assert_array_equal(S1[:, :, 0], Sc[:, :, b])
        np.testing.assert_array_equal(l1[0], ll[b])
    assert np.isfinite(Sc).all()


def test_one_term_and_no_term_windows(engine, small):
    Y, m, Th, _ = small
    engine.set_panel(Y[:, :3], m)  # T = 3: one accumulated column
    ll, Sc = engine.loglik_scores(KIND_DNS, Th)
    _, g = engine.loglik_grad(KIND_DNS, Th)
    assert Sc.shape == (20, 2, 5) and np.all(Sc[:, 0, :] == 0.0)
    assert np.all(np.abs(Sc[:, 1, :] - g) <= 4 * 3 * U * np.abs(Sc[:, 1, :])) and np.abs(g).min(axis=0).max() > 0
    for w in (1, 2):  # nothing accumulated: zeros to the bit, loglik 0
        ll, Sc = engine.loglik_scores(KIND_DNS, Th, T_use=w)
        assert np.all(Sc == 0.0) and np.all(ll == 0.0)


def test_a_deferred_candidate_has_nan_scores_and_is_counted(engine):
    m = S.maturities_30()
    gam = next(g for g in MGL.GAMMAS if MGL.kappa1(g, m) >= 1e6)
    engine.set_panel(S.simulate_panel(KIND_DNS, 10), m)
    Th = np.asfortranarray(np.repeat(S.theta0(KIND_DNS)[:, None], 3, axis=1))
    Th[0, 1] = gam
    ll, Sc = engine.loglik_scores(KIND_DNS, Th)
    assert engine.last_grad_unavailable() == 1 == engine.last_deferred()
    assert np.isnan(Sc[:, :, 1]).all() and np.isfinite(Sc[:, :, [0, 2]]).all() and np.isfinite(ll).all()
    np.testing.assert_array_equal(Sc[:, :, 0], Sc[:, :, 2])
    # a −Inf loglik (σ² = e⁻⁸⁰⁰ = 0): NaN scores as well
    Th[1, 2] = -800.0
    ll, Sc = engine.loglik_scores(KIND_DNS, Th)
    assert np.isneginf(ll[2]) and np.isnan(Sc[:, :, 1:]).all() and np.isfinite(Sc[:, :, 0]).all()


def test_device_entry_point_on_a_side_stream(engine, small):
    Y, m, Th, tu = small
    engine.set_panel(Y, m)
    assert_device_entry_matches(engine.loglik_scores, engine.loglik_scores_device, KIND_DNS, Th, tu)


def test_other_kinds_are_refused(engine, small):
    Y, m, _, _ = small
    engine.set_panel(Y, m)
    for kind in (KIND_TVL, KIND_GNS, KIND_SD_NS, KIND_NNS):
        P = n_params(kind)
        Th = np.zeros((P, 1), order="F")
        out = np.zeros(P * (Y.shape[1] - 1))
        ll = np.zeros(1)
        rc = engine.lib.yfm_loglik_scores_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, _lib.dptr(ll),
                                                _lib.dptr(out))
        assert rc == -4 and b"YFM_MODEL_DNS" in engine.lib.yfm_last_error(), (kind, rc)
        rc = engine.lib.yfm_loglik_info_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, 0, ctypes.c_double(0.0),
                                              _lib.dptr(ll), _lib.dptr(out), _lib.dptr(out), None)
        assert rc == -4 and b"YFM_MODEL_DNS" in engine.lib.yfm_last_error(), (kind, rc)
        with pytest.raises(NotImplementedError):
            engine.loglik_scores(kind, Th)
    # … and more maturities than the tangent kernel's lane mapping holds
    m65 = np.linspace(3, 360, 65)
    engine.set_panel(S.simulate_panel(KIND_DNS, 8, m65, 3), m65)
    Th = S.theta_batch(KIND_DNS, 2, 0.1, 3, bad_frac=0)
    for call in (engine.loglik_scores, engine.loglik_info):
        with pytest.raises(_lib.YFMError) as e:
            call(KIND_DNS, Th)
        assert e.value.code == -4 and "65" in str(e.value)
