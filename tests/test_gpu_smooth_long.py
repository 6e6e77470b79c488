"""The fixed-interval smoother on the device (csrc/yfm_smooth.hip smooth_kernel, M = 3 and 5) at estimation length, on the
cases of tests/golden/smooth_long/smooth_long_cases.npz: an interior 64-column chunk, windows that end on and just past
a chunk boundary, missing columns on both sides of one, GNS5 across chunks and at N = 30, N = 64 with three chunks, and
the bench panel (T = 600, N = 30) at two hard θ.

Rule (tests/smooth_long_fixture.py): per array, with a step's error measured normwise, an ordinary candidate is within
1e-9 of the dense FP64 checker computed here; a hard one is within 1e-9 of it or at least as close to the stored 40-digit
truth as the checker is.  Nothing is widened; every candidate of every case is compared.

Observed on an MI355X, worst array, window and ordinary candidate, device − checker as a fraction of the 1e-9 bar:
SL-chunk 2.1e-4, SL-n64 4.7e-4, SL-hard (bench columns 0, 1) 1.2e-4, GL-chunk 5.5e-3, GL-n30 2.2e-3.  Hard candidates of
SL-hard, (device − checker, device − truth, checker − truth): column 10283 β̂ 5.04e-10, 1.26e-11, 5.17e-10; V 3.29e-9,
1.90e-9, 3.48e-9; C 3.15e-9, 2.17e-9, 5.32e-9; column 1679 β̂ 2.72e-10, 2.94e-13, 2.72e-10; V 1.33e-9, 1.98e-10, 1.35e-9;
C 1.26e-9, 2.21e-10, 1.28e-9.  With a_{t|t} = a_t + P_ts_t, as the kernel had it before these cases, β̂ of column 10283 was
2.28e-9, 1.77e-9, 5.17e-10 and missed the rule.
"""
from __future__ import annotations

import numpy as np
import pytest

import smooth_long_fixture as LF
import smoother_reference as SR
from gpu_scenarios import same_bits

pytestmark = pytest.mark.gpu

CHUNK_CASES = ("SL-chunk", "GL-chunk")


@pytest.mark.parametrize("name,n", LF.case_windows("fixed"))
def test_parity_on_every_case_and_window(engine, name, n):
    c = LF.cases("fixed")[name]
    T = c["Y"].shape[1]
    engine.set_panel(c["Y"], c["maturities"])
    bs, V, C = engine.smooth(c["kind"], c["Theta"], T_use=None if n == T else n)
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    for b in range(c["Theta"].shape[1]):
        LF.assert_candidate("fixed", name, n, b, bs[..., b], V[..., b], C[..., b])


@pytest.mark.parametrize("name,n,b,what", LF.hard_params("fixed"))
def test_hard_candidate_meets_the_rule(engine, name, n, b, what):
    c = LF.cases("fixed")[name]
    engine.set_panel(c["Y"], c["maturities"])
    bs, V, C = engine.smooth(c["kind"], c["Theta"][:, b:b + 1], T_use=n)
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    LF.assert_hard_array("fixed", name, n, b, what, bs[..., 0], V[..., 0], C[..., 0])


@pytest.mark.parametrize("name", CHUNK_CASES)
def test_mixed_windows_in_one_batch_are_the_solo_windows(engine, name):
    """T_use = (1, 64, 65, 128, 129, 192, 193, 200) over copies of one θ: neighbouring candidates end in different
    chunks, so a wave that reads another's window shows up.  Each column is bit-equal to the solo run of its window."""
    c = LF.cases("fixed")[name]
    engine.set_panel(c["Y"], c["maturities"])
    tu = np.array(LF.MIXED_WINDOWS, dtype=np.int32)
    th = c["Theta"][:, :1]
    got = engine.smooth(c["kind"], np.asfortranarray(np.repeat(th, len(tu), axis=1)), T_use=tu)
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    for k, n in enumerate(tu):
        solo = engine.smooth(c["kind"], th, T_use=int(n))
        for g, s in zip(got, solo):
            assert same_bits(g[..., k], s[..., 0]), (name, int(n))
        LF.assert_candidate("fixed", name, int(n), 0, got[0][..., k], got[1][..., k], got[2][..., k])


@pytest.mark.parametrize("n", LF.CUT_WINDOWS)
@pytest.mark.parametrize("name", CHUNK_CASES)
def test_a_window_is_the_panel_cut_to_it(engine, name, n):
    c = LF.cases("fixed")[name]
    engine.set_panel(c["Y"], c["maturities"])
    full = engine.smooth(c["kind"], c["Theta"], T_use=n)
    engine.set_panel(c["Y"][:, :n], c["maturities"])
    cut = engine.smooth(c["kind"], c["Theta"])
    for f, k, m in zip(full, cut, (n, n, n - 1)):
        assert same_bits(f[..., :m, :], k)
        assert np.isnan(f[..., m:, :]).all()


def test_variances_at_T600_are_positive_and_below_the_predicted_ones(engine):
    """SL-hard's benign candidates (bench columns 0 and 1): diag V_t > 0 at every t and diag V_t ≤ diag P_t (1 + 1e-12) —
    conditioning on more data cannot raise a variance.  P_t for t ≥ 2 is slot t − 2 of filter_states."""
    c = LF.cases("fixed")["SL-hard"]
    engine.set_panel(c["Y"], c["maturities"])
    Th = np.asfortranarray(c["Theta"][:, ~c["hard"]])
    assert Th.shape[1] == 2
    _, V, _ = engine.smooth(c["kind"], Th)
    _, _, P = engine.filter_states(c["kind"], Th)
    dV = np.einsum("iitb->itb", V)
    dP = np.einsum("iitb->itb", P)
    assert np.all(dV > 0) and np.all(dV[:, 1:, :] <= dP * (1 + 1e-12))


@pytest.mark.parametrize("name", ("SL-hard", "SL-chunk", "GL-chunk"))
def test_last_smoothed_state_is_the_filtered_one(engine, name):
    """β̂_n = a_{n|n} and V_n = P_{n|n}, to 1e-9 normwise.  filter_states gives the predicted a_{n+1|n} = δ + Φa_{n|n}
    and P_{n+1|n} = ΦP_{n|n}Φ' + Q on the panel with one more column, so the smoother runs on the window n = T − 1 and
    its last state is pushed through the same map (the transition is not inverted: Φ may be near-singular)."""
    c = LF.cases("fixed")[name]
    T = c["Y"].shape[1]
    n = T - 1
    engine.set_panel(c["Y"], c["maturities"])
    bs, V, _ = engine.smooth(c["kind"], c["Theta"], T_use=n, lag_one=False)
    _, a, P = engine.filter_states(c["kind"], c["Theta"])
    for b in range(c["Theta"].shape[1]):
        _, _, Q, delta, Phi = SR.model_fp64(c["kind"], c["maturities"], c["Theta"][:, b])
        want_a, want_P = a[:, n - 1, b], P[:, :, n - 1, b]
        got_a = delta + Phi @ bs[:, n - 1, b]
        got_P = Phi @ V[:, :, n - 1, b] @ Phi.T + Q
        assert np.abs(got_a - want_a).max() <= 1e-9 * np.abs(want_a).max(), (name, b)
        assert np.abs(got_P - want_P).max() <= 1e-9 * np.abs(want_P).max(), (name, b)
