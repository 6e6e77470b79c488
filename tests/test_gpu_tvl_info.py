"""GPU tests of the TVλ information matrices (opg31_kernel and the Hessian assembly of csrc/yfm_score.hip through
yfm_tvl_loglik_info_batch) and of the standard errors built on them (yfm_amd.inference.tvl_standard_errors_batch).

  OPG      J against the same formula in NumPy float64 on the library's own scores, entry by entry within the dot-product
           bound (n + 2)·2⁻⁵³·Σ|S_ik||S_jk| (n the number of summed products, Bartlett-weighted for the lags); J
           symmetric to the bit; T − 1 ∈ {2, 5, 7, 40} (k-step remainders 2, 1, 3, 0), lags ∈ {0, 1, 3, T}; row and
           column 30, the last live row of tile (1,1), inside the bound; guard cells after the 31 × 31 × B block untouched
  Hessian  on tests/golden/tvl_info/tvl_info_cases.npz (make_tvl_info.py: second differences of the 40-digit oracle),
           max |H − H_truth| ≤ ref_err[b] + e_fd[b] at the default step — at least as close to the truth as the plain
           FP64 reference of the same operation; H symmetric to the bit; H against the same stencil assembled in NumPy
           from Engine.tvl_loglik_grad on the 124 points; NaN and counted where a perturbed point is −Inf
  chunks   one call against the same candidates split 2 : 5 into two calls, to the bit
  end to end  tvl_standard_errors_batch at the fixture's T = 40 point and at θ₀.

Observed on MI355X: DESIGN.md §3.15.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from yfm_amd import KIND_TVL, _lib, create_model, tvl_standard_errors_, tvl_standard_errors_batch
from yfm_amd import inference as INF
from yfm_amd import synthetic as S
from yfm_amd.params import transform_params

sys.path.insert(0, str(GOLDEN / "tvl_info"))
import make_tvl_info as MI  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P = 31


@pytest.fixture(scope="module")
def cases():
    return MI.load_cases()


def finite_pool(engine, n, seed, T_use=None):
    """The first n candidates of θ₀ + 0.02·N(0, I) draws whose loglik the value path gives as finite on the panel set
    (on every window of T_use): some draws have a −Inf loglik, and those have no scores by rule."""
    pool = S.theta_batch(KIND_TVL, 4 * n + 8, 0.02, seed, bad_frac=0)
    fin = np.ones(pool.shape[1], dtype=bool)
    for w in (np.atleast_1d(T_use) if T_use is not None else [None]):
        fin &= np.isfinite(engine.loglik(KIND_TVL, pool, T_use=None if w is None else int(w)))
    keep = np.flatnonzero(fin)[:n]
    assert keep.size == n, fin
    return np.asfortranarray(pool[:, keep])


def opg_reference(Sb, lags):
    """(J, bound): Γ₀ + Σ_ℓ w_ℓ(Γ_ℓ + Γ_ℓ') in float64 over the columns that hold a term, and the dot-product bound."""
    terms = np.flatnonzero(np.any(Sb != 0.0, axis=0))
    if terms.size == 0:
        return np.zeros((Sb.shape[0],) * 2), np.zeros((Sb.shape[0],) * 2)
    X = Sb[:, terms[0]:terms[-1] + 1]  # the accumulated range (columns 1 … T_use − 2)
    A = np.abs(X)
    n = X.shape[1]
    J, mag, count = X @ X.T, A @ A.T, n
    for lag in range(1, min(lags, n - 1) + 1):
        w = 1.0 - lag / (lags + 1.0)
        G = X[:, lag:] @ X[:, :-lag].T
        M = A[:, lag:] @ A[:, :-lag].T
        J = J + w * (G + G.T)
        mag = mag + w * (M + M.T)
        count += 2 * (n - lag)
    return J, (count + 2) * U * mag


@pytest.mark.parametrize("T", [3, 6, 8, 41])
def test_opg_is_the_weighted_outer_product_of_the_scores(engine, T):
    m = S.maturities_30()[::5]
    engine.set_panel(S.simulate_panel(KIND_TVL, T, m, 40 + T), m)
    tu = np.array([T, T, max(T - 1, 1), min(3, T), 2], dtype=np.int32)  # two blocks of four waves; windows
    Th = finite_pool(engine, 5, 41, T_use=tu)
    _, Sc = engine.tvl_loglik_scores(KIND_TVL, Th, T_use=tu)
    assert np.isfinite(Sc).all()
    for lags in (0, 1, 3, T):
        r = engine.tvl_loglik_info(KIND_TVL, Th, T_use=tu, lags=lags, hessian=False)
        J = r["opg"]
        assert r["hess"] is None and J.shape == (P, P, 5) and engine.last_grad_unavailable() == 0
        np.testing.assert_array_equal(J, J.transpose(1, 0, 2))
        worst = 0.0
        for b in range(5):
            ref, bound = opg_reference(Sc[:, :, b], lags)
            gap = np.abs(J[:, :, b] - ref)
            assert np.all(gap <= bound), (T, lags, b, np.max(gap / np.maximum(bound, 1e-300)))
            if bound.max() > 0:
                worst = max(worst, np.max(gap[bound > 0] / bound[bound > 0]))
        assert np.all(J[:, :, 4] == 0.0)  # T_use = 2: no term
        # the last live row of tile (1,1): present (Φ₄₄'s scores are not zero) and inside the bound above
        assert J[30, 30, 0] > 0.0 and np.abs(J[30, :30, 0]).max() > 0.0
        print(f"T − 1 = {T - 1}, lags {lags}: worst |J − ref| / bound {worst:.3e}")
        ll, g = engine.tvl_loglik_grad(KIND_TVL, Th, T_use=tu)
        np.testing.assert_array_equal(r["ll"], ll)
        np.testing.assert_array_equal(r["grad"], g)


def test_opg_writes_nothing_outside_its_block(engine):
    """The C entry point with guard cells after the 31 × 31 × B block of opg_out (and of grad_out): untouched."""
    T, B, guard = 8, 5, 64
    m = S.maturities_30()[::5]
    engine.set_panel(S.simulate_panel(KIND_TVL, T, m, 48), m)
    Th = finite_pool(engine, B, 41)
    ll = np.empty(B)
    g = np.full(P * B + guard, 7.0)
    J = np.full(P * P * B + guard, 7.0)
    _lib.check(engine.lib.yfm_tvl_loglik_info_batch(engine.ctx, KIND_TVL, 0, _lib.dptr(Th), P, B, None, 1, 0.0,
                                                    _lib.dptr(ll), _lib.dptr(g), None, _lib.dptr(J)))
    assert np.all(J[P * P * B:] == 7.0) and np.all(g[P * B:] == 7.0)
    r = engine.tvl_loglik_info(KIND_TVL, Th, lags=1, hessian=False)
    np.testing.assert_array_equal(J[:P * P * B].reshape(B, P, P).transpose(2, 1, 0), r["opg"])
    assert np.all(np.isfinite(J)) and np.all(r["opg"][30, 30, :] > 0)


def numpy_stencil(engine, th, h):
    """H of the library's stencil from Engine.tvl_loglik_grad on the 124 points around th."""
    cols, den = [], np.empty((P, 2))
    for i in range(P):
        for k, mult in enumerate((1.0, 2.0)):
            up, dn = th.copy(), th.copy()
            up[i] = th[i] + mult * h
            dn[i] = th[i] - mult * h
            den[i, k] = up[i] - dn[i]
            cols += [up, dn]
    _, g = engine.tvl_loglik_grad(KIND_TVL, np.asfortranarray(np.stack(cols, axis=1)))
    g = g.reshape(P, P, 2, 2)  # [component, direction, h or 2h, up or down]
    c = (g[:, :, :, 0] - g[:, :, :, 1]) / den[None, :, :]
    D = ((4.0 * c[:, :, 0] - c[:, :, 1]) / 3.0).T
    return 0.5 * (D + D.T)


@pytest.mark.parametrize("name", MI.HESS_CASES)
def test_hessian_is_as_close_to_the_truth_as_the_fp64_reference(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"]
    r = engine.tvl_loglik_info(KIND_TVL, Th, opg=False)  # the default step
    H = r["hess"]
    assert r["opg"] is None and H.shape == (P, P, Th.shape[1]) and engine.last_grad_unavailable() == 0
    np.testing.assert_array_equal(H, H.transpose(1, 0, 2))
    scale = np.abs(c["H_truth"]).max(axis=(0, 1))
    err = np.abs(H - c["H_truth"]).max(axis=(0, 1))
    for b in range(Th.shape[1]):
        print(f"case {name} candidate {b}: err/|H|max {err[b] / scale[b]:.3e}, plain FP64 reference's "
              f"{c['ref_err'][b] / scale[b]:.3e} (its step {c['ref_step'][b]:g}), e_fd/|H|max {c['e_fd'][b] / scale[b]:.3e}")
    assert np.all(err <= c["ref_err"] + c["e_fd"]), err / (c["ref_err"] + c["e_fd"])  # every stored candidate
    ll, g = engine.tvl_loglik_grad(KIND_TVL, Th)
    np.testing.assert_array_equal(r["ll"], ll)
    np.testing.assert_array_equal(r["grad"], g)
    # the same stencil in NumPy on the gradient call's own outputs: a few ulp of ‖H‖max (the quotients are the same
    # operations; the assembly's order may differ)
    for b in range(Th.shape[1]):
        Hn = numpy_stencil(engine, Th[:, b], _lib.TVL_INFO_DEFAULT_STEP)
        gap = np.abs(H[:, :, b] - Hn).max()
        print(f"case {name} candidate {b}: |H − NumPy stencil| / |H|max {gap / scale[b]:.3e}")
        assert gap <= 16 * U * scale[b], gap / scale[b]
    # the same bits alone
    np.testing.assert_array_equal(engine.tvl_loglik_info(KIND_TVL, Th[:, 1], opg=False)["hess"][:, :, 0], H[:, :, 1])


def test_a_perturbed_point_at_minus_inf_makes_the_hessian_unavailable(engine, cases):
    """Constrained space, σ² = 2h: the point σ² − 2h is exactly 0, a −Inf loglik; the candidate's own loglik and
    gradient are finite."""
    c = cases["H-n4"]
    engine.set_panel(c["Y"], c["maturities"])
    h = 1e-3
    Tc = np.asfortranarray(transform_params(KIND_TVL, c["Theta"]))
    Tc[0, 1] = 2 * h
    assert np.isneginf(engine.loglik(KIND_TVL, np.r_[0.0, Tc[1:, 1]], space=1)[0])
    r = engine.tvl_loglik_info(KIND_TVL, Tc, space=1, step=h)
    assert engine.last_grad_unavailable() == 1
    assert engine.last_flags() == (0, 0)  # the batch's own counters, not those of its perturbed launches
    assert np.isfinite(r["ll"]).all() and np.isfinite(r["grad"]).all()
    assert np.isnan(r["hess"][:, :, 1]).all() and np.isfinite(r["hess"][:, :, 0]).all()
    assert np.isfinite(r["opg"]).all()  # the scores need the candidate's own point only
    # a candidate without a gradient of its own: NaN everywhere, counted once
    Tc[0, 0] = 0.0
    r = engine.tvl_loglik_info(KIND_TVL, Tc, space=1, step=h)
    assert engine.last_grad_unavailable() == 2 and np.isneginf(r["ll"][0]) and engine.last_flags() == (0, 1)
    assert np.isnan(r["hess"]).all() and np.isnan(r["opg"][:, :, 0]).all() and np.isfinite(r["opg"][:, :, 1]).all()
    # with the Hessian half skipped, the counter answers for the NaN J
    r = engine.tvl_loglik_info(KIND_TVL, Tc, space=1, hessian=False)
    assert engine.last_grad_unavailable() == 1 and np.isnan(r["opg"][:, :, 0]).all()
    for bad in (dict(lags=-1), dict(hessian=False, opg=False)):
        with pytest.raises(ValueError):
            engine.tvl_loglik_info(KIND_TVL, Tc, space=1, **bad)
    rc = engine.lib.yfm_tvl_loglik_info_batch(engine.ctx, KIND_TVL, 1, _lib.dptr(Tc), P, 2, None, 0, 0.0,
                                              _lib.dptr(r["ll"]), _lib.dptr(r["grad"]), None, None)
    assert rc == -1 and b"both null" in engine.lib.yfm_last_error()
    rc = engine.lib.yfm_tvl_loglik_info_batch(engine.ctx, KIND_TVL, 1, _lib.dptr(Tc), P, 2, None, -1, 0.0,
                                              _lib.dptr(r["ll"]), _lib.dptr(r["grad"]), _lib.dptr(r["opg"]), None)
    assert rc == -1 and b"lags" in engine.lib.yfm_last_error()


@pytest.mark.parametrize("half", ["opg", "hess"])
def test_batches_larger_than_one_chunk(engine, cases, half):
    """A large batch runs chunk by chunk.  The score scratch takes 8·31·(T − 1) bytes per candidate:
    at T = 600 a 128 MiB chunk holds 903 candidates, so B = 904 is the smallest batch with two chunks (T·B is what
    decides, so a shorter panel would need as many more candidates).  The Hessian's largest buffer per candidate is
    the work record of its 124 perturbed points' certified launch, 124·88·8 = 87,296 bytes, whatever T: 1,537 candidates
    per chunk, B = 1,538, run at the fixture's N = 4, T = 8.  A candidate's bits must not depend on the chunk it falls
    into: the whole batch against the same candidates split 2 : 5 into two calls, whose chunk boundary falls elsewhere."""
    m = cases["H-n4"]["maturities"]
    T, B, kw = (600, 904, dict(hessian=False, lags=2)) if half == "opg" else (8, 1538, dict(opg=False))
    engine.set_panel(S.simulate_panel(KIND_TVL, T, m, 50 + T), m)
    Th = np.asfortranarray(np.tile(finite_pool(engine, 7, 51), (1, B // 7 + 1))[:, :B])
    Th[0, 5] = -800.0  # σ² = 0: a −Inf loglik in the first chunk and one in the last
    Th[0, B - 1] = -800.0
    r = engine.tvl_loglik_info(KIND_TVL, Th, **kw)
    assert r[half].shape == (P, P, B) and engine.last_grad_unavailable() == 2 and engine.last_flags() == (0, 2)
    assert np.isnan(r[half][:, :, [5, B - 1]]).all() and np.isfinite(np.delete(r[half], [5, B - 1], axis=2)).all()
    cut = 2 * B // 7
    parts = [engine.tvl_loglik_info(KIND_TVL, Th[:, :cut], **kw), engine.tvl_loglik_info(KIND_TVL, Th[:, cut:], **kw)]
    for name in (half, "grad", "ll"):
        np.testing.assert_array_equal(r[name], np.concatenate([p[name] for p in parts], axis=-1))
    np.testing.assert_array_equal(r[half][:, :, B - 2], r[half][:, :, (B - 2) % 7])  # the same θ in the first chunk
    if half == "opg":  # the host-pointer scores call copies chunk by chunk too
        _, Sc = engine.tvl_loglik_scores(KIND_TVL, Th)
        _, Se = engine.tvl_loglik_scores(KIND_TVL, Th[:, 901:904])
        np.testing.assert_array_equal(Sc[:, :, 901:904], Se)


def test_standard_errors_at_the_recorded_point_and_far_from_it(cases):
    """The fixture's T = 40 point: the OPG path always; the Hessian and sandwich paths where the generator recorded a
    negative definite truth Hessian, with se_u from the device's H within 1e-6 relative of the one from the truth H."""
    c = cases["E2E"]
    Y, m = np.asfortranarray(c["Y"]), c["maturities"]
    model, _ = create_model("TVλ", m, len(m), 3)
    Tc = np.asfortranarray(transform_params(KIND_TVL, c["Theta"]))
    kinds = ("opg", "hessian", "sandwich") if bool(c["negdef"]) else ("opg",)
    for cov in kinds:
        se = tvl_standard_errors_batch(model, Y, Tc, cov=cov)
        print(cov, "se_u", se["se_u"][:, 0])
        assert se["pd"].tolist() == [True] and se["unavailable"] == 0
        assert np.all(np.isfinite(se["se_c"])) and np.all(se["se_c"] > 0) and np.all(se["se_u"] > 0)
        one = tvl_standard_errors_(model, Y, Tc[:, 0], cov=cov)
        np.testing.assert_array_equal(one["se_c"], se["se_c"][:, 0])
        assert one["pd"] is True
        if cov == "hessian":
            cov_t, pd_t = INF.covariance(c["H_truth"], None, "hessian")
            assert pd_t.tolist() == [True]
            se_t = np.sqrt(np.einsum("iib->ib", cov_t))
            rel = np.abs(se["se_u"] - se_t) / se_t
            print("se_u from the device's H against the truth H's: max rel", rel.max())
            assert np.all(rel <= 1e-6), rel.max()
    for cov in ("hessian", "sandwich"):  # θ₀ is no maximum: −H is not positive definite there
        se = tvl_standard_errors_batch(model, Y, transform_params(KIND_TVL, c["Theta0"]), cov=cov)
        assert se["pd"].tolist() == [False] and np.isnan(se["se_c"]).all() and np.isnan(se["cov_u"]).all()
        assert np.isfinite(se["ll"]).all() and np.isfinite(se["grad"]).all()
