"""The TVλ extended smoother on the device (csrc/yfm_tvl_smooth.hip tvl_smooth_kernel) at estimation length, on the cases
of tests/golden/tvl_smooth_long/tvl_smooth_long_cases.npz: an interior 64-column chunk, windows that end on and just past
a chunk boundary, missing columns on both sides of one, N = 90 across three chunks and T = 600 at N = 30 — under both
precisions of the forward pass.

Rule (tests/smooth_long_fixture.py): per array, with a step's error measured normwise, an ordinary candidate is within
1e-9 of the dense FP64 checker computed here; a hard one is within 1e-9 of it or at least as close to the stored 40-digit
truth as the checker is.  Nothing is widened; every candidate of every case is compared.

Observed on an MI355X, worst array, window, ordinary candidate and precision, device − checker as a fraction of the
1e-9 bar: TL-chunk 1.1e-3, TL-n90 2.1e-3, TL-600 7.0e-3.  TL-n90's hard candidate 1, worst precision,
(device − checker, device − truth, checker − truth): β̂ 3.27e-11, 5.49e-12, 2.72e-11; V 6.57e-11, 1.10e-11, 5.47e-11;
C 1.24e-10, 3.79e-11, 1.03e-10.
"""
from __future__ import annotations

import numpy as np
import pytest

import smooth_long_fixture as LF
import tvl_smoother_reference as TR
from gpu_scenarios import same_bits
from test_gpu_tvl_smooth import MODES
from yfm_amd import KIND_TVL

pytestmark = pytest.mark.gpu


@pytest.fixture
def prec(engine):
    """engine.precision for the length of a test."""
    old = engine.precision

    def use(mode):
        engine.precision = mode
    yield use
    engine.precision = old


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,n", LF.case_windows("tvl"))
def test_parity_on_every_case_and_window(engine, prec, name, n, mode):
    c = LF.cases("tvl")[name]
    T = c["Y"].shape[1]
    engine.set_panel(c["Y"], c["maturities"])
    prec(mode)
    bs, V, C = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=None if n == T else n)
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    for b in range(c["Theta"].shape[1]):
        LF.assert_candidate("tvl", name, n, b, bs[..., b], V[..., b], C[..., b])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,n,b,what", LF.hard_params("tvl"))
def test_hard_candidate_meets_the_rule(engine, prec, name, n, b, what, mode):
    """In the batch of the parity test: the TVλ kernel promises its bits at a fixed batch size only."""
    c = LF.cases("tvl")[name]
    engine.set_panel(c["Y"], c["maturities"])
    prec(mode)
    bs, V, C = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=n)
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    LF.assert_hard_array("tvl", name, n, b, what, bs[..., b], V[..., b], C[..., b])


def test_mixed_windows_in_one_batch_are_the_solo_windows(engine):
    """T_use = (1, 64, 65, 128, 129, 192, 193, 200) over copies of one θ of TL-chunk: neighbouring candidates end in
    different chunks.  Each column is bit-equal to the same window in a batch of the same size whose windows are all
    that one (the header promises the bits at a fixed batch size), and meets the rule on its window."""
    c = LF.cases("tvl")["TL-chunk"]
    engine.set_panel(c["Y"], c["maturities"])
    tu = np.array(LF.MIXED_WINDOWS, dtype=np.int32)
    Th = np.asfortranarray(np.repeat(c["Theta"][:, :1], len(tu), axis=1))
    got = engine.tvl_smooth(KIND_TVL, Th, T_use=tu)
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    for k, n in enumerate(tu):
        solo = engine.tvl_smooth(KIND_TVL, Th, T_use=int(n))
        for g, s in zip(got, solo):
            assert same_bits(g[..., k], s[..., k]), int(n)
        LF.assert_candidate("tvl", "TL-chunk", int(n), 0, got[0][..., k], got[1][..., k], got[2][..., k])


@pytest.mark.parametrize("n", LF.CUT_WINDOWS)
def test_a_window_agrees_with_the_panel_cut_to_it(engine, n):
    """T_use = n against the panel cut to n columns, as tests/test_gpu_tvl_smooth.py states it: both meet the rule on
    that window and they are within 1e-9 of each other normwise per step (the bits are printed, not asserted)."""
    c = LF.cases("tvl")["TL-chunk"]
    engine.set_panel(c["Y"], c["maturities"])
    full = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=n)
    engine.set_panel(c["Y"][:, :n], c["maturities"])
    cut = engine.tvl_smooth(KIND_TVL, c["Theta"])
    for b in range(c["Theta"].shape[1]):
        LF.assert_candidate("tvl", "TL-chunk", n, b, cut[0][..., b], cut[1][..., b], cut[2][..., b])
        LF.assert_candidate("tvl", "TL-chunk", n, b, full[0][..., b], full[1][..., b], full[2][..., b])
        for f, k, m in zip(full, cut, (n, n, n - 1)):
            assert TR.traj_err(f[..., :m, b], k[..., b], k[..., b]) <= 1e-9
    print("bitwise equal:", all(same_bits(f[..., :m, :], k) for f, k, m in zip(full, cut, (n, n, n - 1))))


def test_variances_at_T600_are_positive_and_below_the_predicted_ones(engine):
    """TL-600: diag V_t > 0 at every t and diag V_t ≤ diag P_t (1 + 1e-12).  P_t for t ≥ 2 is slot t − 2 of filter_states."""
    c = LF.cases("tvl")["TL-600"]
    engine.set_panel(c["Y"], c["maturities"])
    _, V, _ = engine.tvl_smooth(KIND_TVL, c["Theta"])
    _, _, P = engine.filter_states(KIND_TVL, c["Theta"])
    dV = np.einsum("iitb->itb", V)
    dP = np.einsum("iitb->itb", P)
    assert np.all(dV > 0) and np.all(dV[:, 1:, :] <= dP * (1 + 1e-12))


@pytest.mark.parametrize("name", ("TL-600", "TL-chunk"))
def test_last_smoothed_state_is_the_filtered_one(engine, name):
    """β̂_n = a_{n|n} and V_n = P_{n|n}, to 1e-9 normwise: the smoother on the window n = T − 1, its last state pushed
    through a_{n+1|n} = δ + Φa_{n|n}, P_{n+1|n} = ΦP_{n|n}Φ' + Q, against slot n − 1 of filter_states."""
    c = LF.cases("tvl")[name]
    T = c["Y"].shape[1]
    n = T - 1
    engine.set_panel(c["Y"], c["maturities"])
    bs, V, _ = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=n, lag_one=False)
    _, a, P = engine.filter_states(KIND_TVL, c["Theta"])
    for b in range(c["Theta"].shape[1]):
        s = TR.model_fp64(c["maturities"], c["Theta"][:, b])
        want_a, want_P = a[:, n - 1, b], P[:, :, n - 1, b]
        got_a = s.delta + s.Phi @ bs[:, n - 1, b]
        got_P = s.Phi @ V[:, :, n - 1, b] @ s.Phi.T + s.Omega_state
        assert np.abs(got_a - want_a).max() <= 1e-9 * np.abs(want_a).max(), (name, b)
        assert np.abs(got_P - want_P).max() <= 1e-9 * np.abs(want_P).max(), (name, b)
