"""GPU tests of the TVλ score series (csrc/yfm_tvl_score.hip tvl_score_kernel through yfm_tvl_loglik_scores_batch).

S[d, k, b] = ∂ℓ_k/∂θ_d, ℓ_k the term get_loss adds after column k (0-based), for 1 ≤ k ≤ T_use_b − 2 and exactly 0.0
elsewhere (include/yfm.h).  The checks:

  truth         on tests/golden/tvl_info/tvl_info_cases.npz (make_tvl_info.py: nested windows of the binary128 difference
                gradient), max |S − s_truth| ≤ 1e-9·‖g_fd‖∞ + e_fd for every stored candidate
  sum rule      |Σ_k S[d, k, b] − grad[d, b]| ≤ 4·T·2⁻⁵³·Σ_k |S[d, k, b]| against Engine.tvl_loglik_grad (the bound of a
                sum taken in another order)
  bits          ll is Engine.loglik's; the series is the same under both precisions, alone and in a batch of 9 (not a
                multiple of the 8 groups per block), and from the device twin on a side stream, which leaves the guard
                doubles around its output alone
  windows       T_use ∈ {1, 2, 3, T}: exact zeros past the window
  unavailable   a −Inf candidate and a λ-overflow candidate are NaN in all of S; the second is counted
  refusals      every other kind returns −4 from the C entry points.
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

sys.path.insert(0, str(GOLDEN / "tvl_info"))
import make_tvl_info as MI  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-9
U = 2.0 ** -53


@pytest.fixture(scope="module")
def cases():
    return MI.load_cases()


@pytest.fixture(scope="module")
def small(engine):
    """T = 12, N = 7, column 5 all NaN and one entry of column 9 missing (the fixture's S-nan panel); the first 9
    candidates of a pool of 16 whose loglik the library's value path gives as finite under both precisions (it is −Inf
    for some draws: their scores are NaN by rule, which test_unavailable_candidates_are_nan_in_all_of_s covers)."""
    Y, m, _, _ = MI.case_inputs("S-nan")
    pool = S.theta_batch(KIND_TVL, 16, 0.02, 61, bad_frac=0)
    engine.set_panel(Y, m)
    old = engine.lib.yfm_get_precision(engine.ctx)
    fin = np.ones(16, dtype=bool)
    try:
        for prec in (_lib.PREC_CERTIFIED, _lib.PREC_FP64):
            _lib.check(engine.lib.yfm_set_precision(engine.ctx, prec))
            fin &= np.isfinite(engine.loglik(KIND_TVL, pool))
    finally:
        _lib.check(engine.lib.yfm_set_precision(engine.ctx, old))
    keep = np.flatnonzero(fin)[:9]
    assert keep.size == 9, fin
    return Y, m, np.asfortranarray(pool[:, keep])


@pytest.mark.parametrize("name", MI.SCORE_CASES)
def test_scores_match_truth_differences_and_sum_to_the_gradient(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    T = c["Y"].shape[1]
    ll, Sc = engine.tvl_loglik_scores(KIND_TVL, c["Theta"], space=0)
    assert Sc.shape == (31, T - 1, c["Theta"].shape[1]) and engine.last_grad_unavailable() == 0
    err = np.abs(Sc - c["s_truth"]).max(axis=(0, 1))
    gn = np.abs(c["g_fd"]).max(axis=0)
    bound = REL * gn + c["e_fd"]
    print(f"case {name}: max err/bound {np.max(err / bound):.3e}, max err/|g| {np.max(err / gn):.3e}")
    assert np.all(err <= bound), err / bound  # every stored candidate
    assert np.all(Sc[:, 0, :] == 0.0)
    np.testing.assert_allclose(ll, c["loglik_truth"], rtol=REL)
    np.testing.assert_array_equal(ll, engine.loglik(KIND_TVL, c["Theta"], space=0))
    l2, g = engine.tvl_loglik_grad(KIND_TVL, c["Theta"], space=0)
    np.testing.assert_array_equal(ll, l2)
    gap = np.abs(Sc.sum(axis=1) - g)
    sb = 4 * T * U * np.abs(Sc).sum(axis=1)
    print(f"case {name}: sum rule worst gap/bound {np.max(gap[sb > 0] / sb[sb > 0]):.3e}")
    assert np.all(gap <= sb), np.argwhere(gap > sb)


def test_same_bits_under_both_precisions_in_both_spaces_alone_and_in_a_batch_of_nine(engine, small):
    Y, m, Th = small
    engine.set_panel(Y, m)
    assert Th.shape[1] == 9  # two blocks of 8 groups, the second with one live group
    old = engine.lib.yfm_get_precision(engine.ctx)
    try:
        for space in (0, 1):
            X = Th if space == 0 else np.asfortranarray(transform_params(KIND_TVL, Th))
            runs = []
            for prec in (_lib.PREC_CERTIFIED, _lib.PREC_FP64):
                _lib.check(engine.lib.yfm_set_precision(engine.ctx, prec))
                ll, Sc = engine.tvl_loglik_scores(KIND_TVL, X, space=space)
                np.testing.assert_array_equal(ll, engine.loglik(KIND_TVL, X, space=space))
                assert np.isfinite(Sc).all() and np.abs(Sc[:, 1:, :]).max() > 0
                for b in (0, 7, 8):
                    _, S1 = engine.tvl_loglik_scores(KIND_TVL, X[:, b], space=space)
                    np.testing.assert_array_equal(S1[:, :, 0], Sc[:, :, b])
                runs.append(Sc)
            np.testing.assert_array_equal(runs[0], runs[1])
            _, g = engine.tvl_loglik_grad(KIND_TVL, X, space=space)
            assert np.all(np.abs(runs[0].sum(axis=1) - g) <= 4 * Y.shape[1] * U * np.abs(runs[0]).sum(axis=1))
    finally:
        _lib.check(engine.lib.yfm_set_precision(engine.ctx, old))


def test_windows_end_in_exact_zeros(engine, small):
    Y, m, Th = small
    T = Y.shape[1]
    engine.set_panel(Y, m)
    X = np.asfortranarray(np.repeat(Th[:, :1], 4, axis=1))
    tu = np.array([1, 2, 3, T], dtype=np.int32)
    ll, Sc = engine.tvl_loglik_scores(KIND_TVL, X, T_use=tu)
    assert np.all(Sc[:, :, :2] == 0.0) and np.all(ll[:2] == 0.0)  # T_use ≤ 2: no term
    assert np.all(Sc[:, 2:, 2] == 0.0) and np.all(Sc[:, 0, :] == 0.0) and np.abs(Sc[:, 1, 2]).max() > 0
    np.testing.assert_array_equal(Sc[:, 1, 2], Sc[:, 1, 3])  # a step's term does not depend on the window's end
    assert np.abs(Sc[:, T - 2, 3]).max() > 0 and np.isfinite(Sc).all()
    np.testing.assert_array_equal(ll, engine.loglik(KIND_TVL, X, T_use=tu))


def test_unavailable_candidates_are_nan_in_all_of_s(engine, small):
    Y, m, Th = small
    engine.set_panel(Y, m)
    X = np.asfortranarray(Th[:, :3].copy())
    X[0, 1] = -800.0  # σ² = e⁻⁸⁰⁰ = 0: a −Inf loglik
    ll, Sc = engine.tvl_loglik_scores(KIND_TVL, X, T_use=np.array([12, 5, 12], dtype=np.int32))
    assert np.isneginf(ll[1]) and np.isnan(Sc[:, :, 1]).all() and np.isfinite(Sc[:, :, [0, 2]]).all()
    assert engine.last_grad_unavailable() == 0  # a −Inf loglik is counted by last_flags, as after the gradient call
    with np.load(GOLDEN / "edge" / "tvl_lambda_overflow.npz", allow_pickle=False) as z:
        Yo, mo, tho = np.asfortranarray(z["Y"]), z["maturities"], z["Theta"][:, 0]
    engine.set_panel(Yo, mo)
    nb = S.theta_batch(KIND_TVL, 2, 0.02, 11, bad_frac=0)
    X = np.asfortranarray(np.stack([nb[:, 0], tho, nb[:, 1]], axis=1))
    ll, Sc = engine.tvl_loglik_scores(KIND_TVL, X)
    n_un = engine.last_grad_unavailable()
    _, g = engine.tvl_loglik_grad(KIND_TVL, X)
    assert np.isnan(g[:, 1]).all() and np.isnan(Sc[:, :, 1]).all()
    assert np.isfinite(Sc[:, :, [0, 2]]).all() and np.isfinite(ll[[0, 2]]).all()
    assert n_un == engine.last_grad_unavailable() == (1 if np.isfinite(ll[1]) else 0)


def test_device_entry_point_on_a_side_stream_leaves_the_guards_alone(engine, small):
    Y, m, Th = small
    engine.set_panel(Y, m)
    T = Y.shape[1]
    tu = np.array([T, 1, 2, 3, 7, T, T - 1, 4, T], dtype=np.int32)
    assert_device_entry_matches(engine.tvl_loglik_scores, engine.tvl_loglik_scores_device, KIND_TVL, Th, tu, guard=64)


def test_other_kinds_are_refused_by_the_c_entry_points(engine, small):
    Y, m, _ = small
    engine.set_panel(Y, m)
    for kind in (KIND_DNS, KIND_GNS, KIND_SD_NS, KIND_NNS):
        P = n_params(kind)
        Th = np.zeros((P, 1), order="F")
        out = np.zeros(P * max(P, Y.shape[1] - 1))
        ll = np.zeros(1)
        rc = engine.lib.yfm_tvl_loglik_scores_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, _lib.dptr(ll),
                                                    _lib.dptr(out))
        assert rc == -4 and b"YFM_MODEL_TVL" in engine.lib.yfm_last_error(), (kind, rc)
        rc = engine.lib.yfm_tvl_loglik_scores_batch_device(engine.ctx, kind, 0, None, P, 1, None, None, None, None)
        assert rc == -4 and b"YFM_MODEL_TVL" in engine.lib.yfm_last_error(), (kind, rc)
        rc = engine.lib.yfm_tvl_loglik_info_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, 0,
                                                  ctypes.c_double(0.0), _lib.dptr(ll), _lib.dptr(out), _lib.dptr(out),
                                                  None)
        assert rc == -4 and b"YFM_MODEL_TVL" in engine.lib.yfm_last_error(), (kind, rc)
        with pytest.raises(NotImplementedError):
            engine.tvl_loglik_scores(kind, Th)
