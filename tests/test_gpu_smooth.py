"""The fixed-interval smoother on the device (include/yfm.h yfm_smooth_batch; csrc/yfm_smooth.hip) against the
committed checker and truth arrays of tests/golden/smooth/smooth_cases.npz.

Rule (tests/test_gpu_states.py, factor 1): per array, with a step's error measured normwise against the truth's
magnitude at that step, the device is within 1e-9 of the dense FP64 checker, or at least as close to the 40-digit truth
as the checker is.  Nothing is widened; every candidate of every case is compared.
"""
from __future__ import annotations

import numpy as np
import pytest

import smooth_fixture as SF
import smoother_reference as SR
from gpu_scenarios import same_bits
from yfm_amd import KIND_DNS, KIND_NNS, KIND_SD_NS, KIND_TVL, _lib, n_params
from yfm_amd import synthetic as S

pytestmark = pytest.mark.gpu


def n30(engine):
    c = SF.cases()["S-n30"]
    engine.set_panel(c["Y"], c["maturities"])
    return c


@pytest.mark.parametrize("space", (0, 1))
@pytest.mark.parametrize("name,n", SF.CASE_WINDOWS)
def test_parity_on_every_case_and_window(engine, name, n, space):
    c = SF.cases()[name]
    T = c["Y"].shape[1]
    n = SF.window_of(c, n)
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"] if space == 0 else c["Theta_c"]
    bs, V, C = engine.smooth(c["kind"], Th, space=space, T_use=None if n == T else n)
    assert bs.shape == (V.shape[0], T, Th.shape[1]) and C.shape[2] == T - 1
    assert engine.last_grad_unavailable() == 0 and engine.last_deferred() == 0
    for b in range(Th.shape[1]):
        SF.assert_candidate(name, n, b, space, bs[..., b], V[..., b], C[..., b])


def test_covariance_is_symmetric_to_the_bit_and_below_the_predicted_one(engine):
    """V_t = V_t' bitwise, and diag V_t ≤ diag P_t (1 + 1e-12): conditioning on more data cannot raise a variance.
    P_t for t ≥ 2 is slot t − 2 of filter_states."""
    c = n30(engine)
    bs, V, C = engine.smooth(c["kind"], c["Theta"])
    _, _, P = engine.filter_states(c["kind"], c["Theta"])
    assert same_bits(V, np.transpose(V, (1, 0, 2, 3)))
    dV = np.einsum("iitb->itb", V)[:, 1:, :]
    dP = np.einsum("iitb->itb", P)
    assert np.all(dV > 0) and np.all(dV <= dP * (1 + 1e-12))


def test_last_smoothed_state_propagates_to_predicts_forecast(engine):
    """δ + Φβ̂_n is a_{n+1|n}: column n − 1 (1-based) of yfm_predict's factors at horizon 1, within 1e-9 normwise."""
    c = n30(engine)
    T = c["Y"].shape[1]
    bs = engine.smooth(c["kind"], c["Theta"], lag_one=False)[0]
    fac = engine.predict(c["kind"], c["Theta"], space=0, horizon=1)["factors"]
    for b in range(c["Theta"].shape[1]):
        _, _, _, delta, Phi = SR.model_fp64(c["kind"], c["maturities"], c["Theta"][:, b])
        want = fac[:, T - 2, b]
        got = delta + Phi @ bs[:, T - 1, b]
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_a_candidate_does_not_depend_on_its_batch_or_position(engine):
    c = n30(engine)
    th = c["Theta"][:, :1]
    solo = engine.smooth(c["kind"], th)
    Th = np.asfortranarray(S.theta_batch(KIND_DNS, 70, 0.02, 91, bad_frac=0))
    for pos in (0, 37, 69):
        Th[:, pos] = th[:, 0]
    got = engine.smooth(c["kind"], Th)
    for pos in (0, 37, 69):
        for g, s in zip(got, solo):
            assert same_bits(np.ascontiguousarray(g[..., pos]), np.ascontiguousarray(s[..., 0])), pos


@pytest.mark.parametrize("n", (1, 3, 64, 65))  # one column, a partial chunk, a chunk exactly full, one column beyond it
def test_a_window_is_the_panel_cut_to_it(engine, n):
    c = SF.cases()["S-n30"]
    engine.set_panel(c["Y"], c["maturities"])
    full = engine.smooth(c["kind"], c["Theta"], T_use=n)
    engine.set_panel(c["Y"][:, :n], c["maturities"])
    cut = engine.smooth(c["kind"], c["Theta"])
    for f, k, m in zip(full, cut, (n, n, n - 1)):
        assert same_bits(np.ascontiguousarray(f[..., :m, :]), np.ascontiguousarray(k))
        assert np.isnan(f[..., m:, :]).all()


def test_initialize_filter_throw_is_unavailable_and_leaves_its_neighbours(engine):
    """Φ = I: I − Φ is singular, initialize_filter throws — all-NaN outputs and an unavailable count of 1."""
    c = n30(engine)
    good = engine.smooth(c["kind"], c["Theta_c"], space=1)
    Th = np.asfortranarray(np.repeat(c["Theta_c"][:, :1], 3, axis=1))
    Th[:, 2] = c["Theta_c"][:, 1]
    Th[-9:, 1] = np.eye(3).reshape(-1)
    got = engine.smooth(c["kind"], Th, space=1)
    assert engine.last_grad_unavailable() == 1
    assert engine.last_flags()[0] == 1
    for g, s in zip(got, good):
        assert np.isnan(g[..., 1]).all()
        assert same_bits(np.ascontiguousarray(g[..., 0]), np.ascontiguousarray(s[..., 0]))
        assert same_bits(np.ascontiguousarray(g[..., 2]), np.ascontiguousarray(s[..., 1]))


def test_a_deferred_candidate_is_unavailable_and_counted(engine):
    """Near-collinear loadings (λ = 0.01 + e⁴: the recipe of tests/test_gpu_deferred.py) put the candidate on the
    deferral list: NaN outputs, counted; its forward states stay available through filter_states."""
    c = n30(engine)
    Th = np.asfortranarray(np.repeat(c["Theta"][:, :1], 2, axis=1))
    Th[0, 1] = 4.0
    bs, V, C = engine.smooth(c["kind"], Th)
    assert engine.last_deferred() == 1 and engine.last_grad_unavailable() == 1
    assert np.isnan(bs[..., 1]).all() and np.isnan(V[..., 1]).all() and np.isnan(C[..., 1]).all()
    assert np.isfinite(bs[..., 0]).all() and np.isfinite(V[..., 0]).all() and np.isfinite(C[..., 0]).all()
    ll, beta, _ = engine.filter_states(c["kind"], Th)
    assert np.isfinite(ll).all() and np.isfinite(beta).all()


def test_lag_one_array_is_optional_and_slots_past_a_window_are_nan(engine):
    c = n30(engine)
    tu = np.array([3, 64], dtype=np.int32)
    with_c = engine.smooth(c["kind"], c["Theta"], T_use=tu)
    bs, V, C = engine.smooth(c["kind"], c["Theta"], T_use=tu, lag_one=False)
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
    host = engine.smooth(c["kind"], Th)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()  # B × P row-major = P × B column-major
    d_b = torch.zeros(B * T * 3, dtype=torch.float64, device="cuda")
    d_V = torch.zeros(B * T * 9, dtype=torch.float64, device="cuda")
    d_C = torch.zeros(B * (T - 1) * 9, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream()
    engine.smooth_device(c["kind"], d_th.data_ptr(), P, B, d_b.data_ptr(), d_V.data_ptr(), d_C.data_ptr(),
                         stream=s.cuda_stream)
    s.synchronize()
    assert engine.last_grad_unavailable() == 0
    for d, h in zip((d_b, d_V, d_C), host):
        assert same_bits(d.cpu().numpy(), h.reshape(-1, order="F"))


def test_record_scratch_of_more_than_one_chunk(engine):
    """B = 2,500 copies of S-E's θ on the panel padded to T = 600 with NaN columns: the forward record of a candidate
    is 12 × 599 doubles, so 2,500 of them exceed the 128 MiB chunk (2,334 candidates) and the batch runs as two chunks.
    Five candidates, on both sides of the chunk boundary, are bitwise equal to the solo run."""
    c = SF.cases()["S-E"]
    N, T0 = c["Y"].shape
    Y = np.full((N, 600), np.nan, order="F")
    Y[:, :T0] = c["Y"]
    engine.set_panel(Y, c["maturities"])
    th = c["Theta"][:, :1]
    solo = engine.smooth(c["kind"], th)
    got = engine.smooth(c["kind"], np.asfortranarray(np.repeat(th, 2500, axis=1)))
    assert engine.last_grad_unavailable() == 0
    for pos in (0, 1, 2333, 2334, 2499):
        for g, s in zip(got, solo):
            assert same_bits(np.ascontiguousarray(g[..., pos]), np.ascontiguousarray(s[..., 0])), pos
    # the columns with data are the unpadded panel's states conditioned on the same data: the padding adds none
    assert np.isfinite(got[0][:, :, 0]).all()


def test_empty_batch_succeeds(engine):
    n30(engine)
    bs, V, C = engine.smooth(KIND_DNS, np.empty((n_params(KIND_DNS), 0), order="F"))
    assert bs.shape[-1] == 0 and V.shape[-1] == 0 and C.shape[-1] == 0


@pytest.mark.parametrize("kind,word", ((KIND_TVL, "extended smoother"), (KIND_SD_NS, "lambda"), (KIND_NNS, "neural")))
def test_refused_kinds(engine, kind, word):
    """YFM_EUNSUPPORTED from the C ABI with a message naming the gap, and NotImplementedError from the host mirror."""
    c = n30(engine)
    P = n_params(kind)
    Th = np.zeros((P, 1), order="F")
    T = c["Y"].shape[1]
    bs, V = np.empty((3, T, 1), order="F"), np.empty((3, 3, T, 1), order="F")
    rc = engine.lib.yfm_smooth_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, _lib.dptr(bs), _lib.dptr(V), None)
    assert rc == -4
    assert word in engine.lib.yfm_last_error().decode()
    with pytest.raises(NotImplementedError):
        engine.smooth(kind, Th)
