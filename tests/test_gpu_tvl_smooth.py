"""The TVλ extended smoother on the device (include/yfm.h yfm_tvl_smooth_batch; csrc/yfm_tvl_smooth.hip) against the
committed checker and truth arrays of tests/golden/tvl_smooth/tvl_smooth_cases.npz.

Rule (tests/test_gpu_smooth.py, factor 1): per array, with a step's error measured normwise against the truth's
magnitude at that step, the device is within 1e-9 of the dense FP64 checker, or at least as close to the 40-digit truth
as the checker is.  Nothing is widened; every candidate of every case is compared, under both precisions of the forward
pass.
"""
from __future__ import annotations

import numpy as np
import pytest

import tvl_smooth_fixture as TF
import tvl_smoother_reference as TR
from conftest import GOLDEN
from gpu_scenarios import same_bits
from yfm_amd import KIND_DNS, KIND_NNS, KIND_SD_NS, KIND_TVL, _lib, n_params
from yfm_amd import synthetic as S

pytestmark = pytest.mark.gpu

MODES = (_lib.PREC_CERTIFIED, _lib.PREC_FP64)


@pytest.fixture
def prec(engine):
    """engine.precision for the length of a test."""
    old = engine.precision

    def use(mode):
        engine.precision = mode
    yield use
    engine.precision = old


def n30(engine):
    c = TF.cases()["T-n30"]
    engine.set_panel(c["Y"], c["maturities"])
    return c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("space", (0, 1))
@pytest.mark.parametrize("name,n", TF.CASE_WINDOWS)
def test_parity_on_every_case_and_window(engine, prec, name, n, space, mode):
    c = TF.cases()[name]
    T = c["Y"].shape[1]
    n = TF.window_of(c, n)
    engine.set_panel(c["Y"], c["maturities"])
    prec(mode)
    Th = c["Theta"] if space == 0 else c["Theta_c"]
    bs, V, C = engine.tvl_smooth(KIND_TVL, Th, space=space, T_use=None if n == T else n)
    assert bs.shape == (4, T, Th.shape[1]) and V.shape == (4, 4, T, Th.shape[1]) and C.shape[2] == T - 1
    assert engine.last_grad_unavailable() == 0
    for b in range(Th.shape[1]):
        TF.assert_candidate(name, n, b, space, bs[..., b], V[..., b], C[..., b])


def test_covariance_is_symmetric_to_the_bit_and_below_the_predicted_one(engine):
    """V_t = V_t' bitwise, diag V_t > 0 at every column, and diag V_t ≤ diag P_t (1 + 1e-12): conditioning on more data
    cannot raise a variance.  P_t for t ≥ 2 is slot t − 2 of filter_states."""
    c = n30(engine)
    bs, V, C = engine.tvl_smooth(KIND_TVL, c["Theta"])
    _, _, P = engine.filter_states(KIND_TVL, c["Theta"])
    assert same_bits(V, np.transpose(V, (1, 0, 2, 3)))
    dV = np.einsum("iitb->itb", V)
    dP = np.einsum("iitb->itb", P)
    assert np.all(dV > 0) and np.all(dV[:, 1:, :] <= dP * (1 + 1e-12))


def test_last_smoothed_state_propagates_to_predicts_forecast(engine):
    """δ + Φβ̂_n is a_{n+1|n}: column n − 1 (1-based) of yfm_predict's factors at horizon 1, within 1e-9 normwise."""
    c = n30(engine)
    T = c["Y"].shape[1]
    bs = engine.tvl_smooth(KIND_TVL, c["Theta"], lag_one=False)[0]
    fac = engine.predict(KIND_TVL, c["Theta"], space=0, horizon=1)["factors"]
    for b in range(c["Theta"].shape[1]):
        s = TR.model_fp64(c["maturities"], c["Theta"][:, b])
        want = fac[:, T - 2, b]
        got = s.delta + s.Phi @ bs[:, T - 1, b]
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("n", (1, 3, 64, 65))  # one column, a partial chunk, a chunk exactly full, one column beyond it
def test_a_window_agrees_with_the_panel_cut_to_it(engine, n):
    """T_use = n against the panel cut to n columns: both meet the parity rule on that window, and they are within 1e-9
    of each other normwise per step.  Whether they are bitwise equal is printed, not asserted: the header promises the
    rule across launches of different shape, not the bits."""
    c = TF.cases()["T-n30"]
    engine.set_panel(c["Y"], c["maturities"])
    full = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=n)
    engine.set_panel(c["Y"][:, :n], c["maturities"])
    cut = engine.tvl_smooth(KIND_TVL, c["Theta"])
    for b in range(c["Theta"].shape[1]):
        TF.assert_candidate("T-n30", n, b, 0, cut[0][..., b], cut[1][..., b], cut[2][..., b])
        TF.assert_candidate("T-n30", n, b, 0, full[0][..., b], full[1][..., b], full[2][..., b])
        for f, k, m in zip(full, cut, (n, n, n - 1)):
            assert TR.traj_err(f[..., :m, b], k[..., b], k[..., b]) <= 1e-9
    print("bitwise equal:", all(same_bits(f[..., :m, :], k) for f, k, m in zip(full, cut, (n, n, n - 1))))


@pytest.mark.parametrize("mode", MODES)
def test_a_candidate_does_not_depend_on_its_position_at_a_fixed_batch_size(engine, prec, mode):
    """B = 70 twice: the candidate at positions 0, 37 and 69 of one batch and at position 5 of a batch whose other
    candidates are different ones — the same bits everywhere."""
    c = n30(engine)
    prec(mode)
    th = c["Theta"][:, 0]
    Th = np.asfortranarray(S.theta_batch(KIND_TVL, 70, 0.02, 91, bad_frac=0))
    for pos in (0, 37, 69):
        Th[:, pos] = th
    got = engine.tvl_smooth(KIND_TVL, Th)
    Th2 = np.asfortranarray(S.theta_batch(KIND_TVL, 70, 0.02, 92, bad_frac=0))
    Th2[:, 5] = th
    other = engine.tvl_smooth(KIND_TVL, Th2)
    for pos in (37, 69):
        for g in got:
            assert same_bits(g[..., pos], g[..., 0]), pos
    for g, o in zip(got, other):
        assert same_bits(g[..., 0], o[..., 5])
    TF.assert_candidate("T-n30", 70, 0, 0, got[0][..., 37], got[1][..., 37], got[2][..., 37])


def test_initialize_filter_throw_is_unavailable_and_leaves_its_neighbours(engine):
    """Φ = I: I − Φ is singular, initialize_filter throws — all-NaN outputs and an unavailable count of 1; the
    neighbours keep the bits of a batch of the same size without it."""
    c = n30(engine)
    Th = np.asfortranarray(np.stack([c["Theta_c"][:, 0], c["Theta_c"][:, 1], c["Theta_c"][:, 1]], axis=1))
    good = engine.tvl_smooth(KIND_TVL, Th, space=1)
    Th[15:31, 1] = np.eye(4).reshape(-1)
    got = engine.tvl_smooth(KIND_TVL, Th, space=1)
    assert engine.last_grad_unavailable() == 1
    assert engine.last_flags()[0] == 1
    for g, s in zip(got, good):
        assert np.isnan(g[..., 1]).all()
        assert same_bits(g[..., 0], s[..., 0])
        assert same_bits(g[..., 2], s[..., 2])


def test_a_minus_inf_loglik_is_unavailable(engine):
    """σ² = e^−800 = 0: the window's loglik is −Inf — NaN outputs, counted."""
    c = n30(engine)
    Th = np.asfortranarray(np.repeat(c["Theta"][:, :1], 2, axis=1))
    Th[0, 1] = -800.0
    bs, V, C = engine.tvl_smooth(KIND_TVL, Th)
    assert engine.last_grad_unavailable() == 1 and engine.last_flags() == (0, 1)
    assert np.isnan(bs[..., 1]).all() and np.isnan(V[..., 1]).all() and np.isnan(C[..., 1]).all()
    assert np.isfinite(bs[..., 0]).all() and np.isfinite(V[..., 0]).all() and np.isfinite(C[..., 0]).all()


def test_lag_one_array_is_optional_and_slots_past_a_window_are_nan(engine):
    c = n30(engine)
    tu = np.array([3, 64], dtype=np.int32)
    with_c = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=tu)
    bs, V, C = engine.tvl_smooth(KIND_TVL, c["Theta"], T_use=tu, lag_one=False)
    assert C is None
    assert same_bits(bs, with_c[0]) and same_bits(V, with_c[1])
    for b, n in enumerate(tu):
        assert np.isfinite(bs[:, :n, b]).all() and np.isnan(bs[:, n:, b]).all()
        assert np.isfinite(V[:, :, :n, b]).all() and np.isnan(V[:, :, n:, b]).all()
        assert np.isfinite(with_c[2][:, :, :n - 1, b]).all() and np.isnan(with_c[2][:, :, n - 1:, b]).all()


def test_device_pointer_call_gives_the_same_bits(engine):
    import torch
    c = n30(engine)
    Th = c["Theta"]
    P, B = Th.shape
    T = c["Y"].shape[1]
    host = engine.tvl_smooth(KIND_TVL, Th)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()  # B × P row-major = P × B column-major
    d_b = torch.zeros(B * T * 4, dtype=torch.float64, device="cuda")
    d_V = torch.zeros(B * T * 16, dtype=torch.float64, device="cuda")
    d_C = torch.zeros(B * (T - 1) * 16, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    engine.tvl_smooth_device(KIND_TVL, d_th.data_ptr(), P, B, d_b.data_ptr(), d_V.data_ptr(), d_C.data_ptr(),
                             stream=s.cuda_stream)
    s.synchronize()
    assert engine.last_grad_unavailable() == 0
    for d, h in zip((d_b, d_V, d_C), host):
        assert same_bits(d.cpu().numpy(), h.reshape(-1, order="F"))


def test_a_batch_of_more_than_one_chunk(engine):
    """T-E padded to T = 600 with NaN columns: the forward record of a candidate is 20 × 599 doubles, so a 128 MiB chunk
    holds 1,400 candidates and B = 1,403 runs as two chunks.  Candidates on both sides of the boundary (positions 1,399
    and 1,400) and at the batch's end carry the bits they have in the first chunk of another batch of the same B."""
    c = TF.cases()["T-E"]
    N, T0 = c["Y"].shape
    T, B = 600, 1403
    chunk = (128 << 20) // (8 * 20 * (T - 1))
    assert chunk == 1400 and chunk < B
    Y = np.full((N, T), np.nan, order="F")
    Y[:, :T0] = c["Y"]
    engine.set_panel(Y, c["maturities"])
    t0, t1, t2 = (c["Theta"][:, k] for k in range(3))
    A = np.asfortranarray(np.repeat(t0[:, None], B, axis=1))
    A[:, chunk - 1], A[:, chunk], A[:, B - 1] = t1, t2, t1
    R = np.asfortranarray(np.repeat(t0[:, None], B, axis=1))
    R[:, 0], R[:, 1] = t1, t2
    got = engine.tvl_smooth(KIND_TVL, A, lag_one=False)
    assert engine.last_grad_unavailable() == 0
    ref = engine.tvl_smooth(KIND_TVL, R, lag_one=False)
    for g, r in zip(got[:2], ref[:2]):
        assert same_bits(g[..., chunk - 1], r[..., 0])
        assert same_bits(g[..., chunk], r[..., 1])
        assert same_bits(g[..., B - 1], r[..., 0])
        assert same_bits(g[..., chunk + 1], r[..., 5])
        assert same_bits(g[..., 0], r[..., 5])
    assert np.isfinite(got[0][:, :, chunk]).all() and np.isfinite(got[1][:, :, :, chunk]).all()


def test_the_lambda_overflow_candidate_is_never_a_mixture(engine):
    """tests/golden/edge/tvl_lambda_overflow.npz: all NaN and counted, or finite throughout its window."""
    with np.load(GOLDEN / "edge" / "tvl_lambda_overflow.npz", allow_pickle=False) as z:
        Y, m, Th = np.asfortranarray(z["Y"]), z["maturities"], np.asfortranarray(z["Theta"])
    engine.set_panel(Y, m)
    arrays = engine.tvl_smooth(KIND_TVL, Th)
    nan_b = 0
    for b in range(Th.shape[1]):
        fin = [np.isfinite(a[..., b]).all() for a in arrays]
        nan = [np.isnan(a[..., b]).all() for a in arrays]
        assert all(fin) or all(nan), (b, fin, nan)
        nan_b += all(nan)
    assert engine.last_grad_unavailable() == nan_b


def test_empty_batch_succeeds(engine):
    n30(engine)
    bs, V, C = engine.tvl_smooth(KIND_TVL, np.empty((n_params(KIND_TVL), 0), order="F"))
    assert bs.shape[-1] == 0 and V.shape[-1] == 0 and C.shape[-1] == 0


@pytest.mark.parametrize("kind,word", ((KIND_DNS, "yfm_smooth_batch"), (KIND_SD_NS, "nothing to smooth"),
                                       (KIND_NNS, "nothing to smooth")))
def test_refused_kinds(engine, kind, word):
    """YFM_EUNSUPPORTED from the C ABI with a message naming where to go, and NotImplementedError from the host mirror."""
    c = n30(engine)
    P = n_params(kind)
    Th = np.zeros((P, 1), order="F")
    T = c["Y"].shape[1]
    bs, V = np.empty((4, T, 1), order="F"), np.empty((4, 4, T, 1), order="F")
    rc = engine.lib.yfm_tvl_smooth_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, _lib.dptr(bs), _lib.dptr(V),
                                         None)
    assert rc == -4
    assert word in engine.lib.yfm_last_error().decode()
    with pytest.raises(NotImplementedError):
        engine.tvl_smooth(kind, Th)
