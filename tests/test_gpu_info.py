"""GPU tests of the DNS information matrices (csrc/yfm_score.hip through yfm_loglik_info_batch) and of the standard
errors built on them (yfm_amd.inference).

  OPG      J against the same formula in NumPy float64 on the library's own scores, entry by entry within the dot-product
           bound (n + 2)·2⁻⁵³·Σ|S_ik||S_jk| (n the number of summed products, Bartlett-weighted for the lags); J
           symmetric to the bit; T − 1 ∈ {2, 5, 7, 40} (k-step remainders 2, 1, 3, 0), lags ∈ {0, 1, 3, T}
  Hessian  on tests/golden/info/info_cases.npz (make_info.py: second differences of the 40-digit oracle),
           max |H − H_truth| ≤ ref_err[b] + e_fd[b] — at least as close to the truth as the plain FP64 reference of the same
           operation; H symmetric to the bit, independent of the batch, NaN and counted where a perturbed point is −Inf
  end to end  standard_errors_batch at an L-BFGS optimum of the 80-month N = 10 panel and at θ₀.

Observed on MI355X: DESIGN.md §3.11.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from yfm_amd import KIND_DNS, _lib, create_model, estimate_lbfgs_batch, standard_errors_, standard_errors_batch
from yfm_amd import synthetic as S
from yfm_amd.params import transform_params

sys.path.insert(0, str(GOLDEN / "info"))
import make_info as MI  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def cases():
    return MI.load_cases()


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
    m = S.maturities_30()[::3]
    engine.set_panel(S.simulate_panel(KIND_DNS, T, m, 40 + T), m)
    Th = S.theta_batch(KIND_DNS, 5, 0.1, 41, bad_frac=0)
    tu = np.array([T, T, max(T - 1, 1), min(3, T), 2], dtype=np.int32)  # two blocks of four waves; windows
    _, Sc = engine.loglik_scores(KIND_DNS, Th, T_use=tu)
    for lags in (0, 1, 3, T):
        r = engine.loglik_info(KIND_DNS, Th, T_use=tu, lags=lags, hessian=False)
        J = r["opg"]
        assert r["hess"] is None and J.shape == (20, 20, 5) and engine.last_grad_unavailable() == 0
        np.testing.assert_array_equal(J, J.transpose(1, 0, 2))
        worst = 0.0
        for b in range(5):
            ref, bound = opg_reference(Sc[:, :, b], lags)
            gap = np.abs(J[:, :, b] - ref)
            assert np.all(gap <= bound), (T, lags, b, np.max(gap / np.maximum(bound, 1e-300)))
            if bound.max() > 0:
                worst = max(worst, np.max(gap[bound > 0] / bound[bound > 0]))
        assert np.all(J[:, :, 4] == 0.0)  # T_use = 2: no term
        print(f"T − 1 = {T - 1}, lags {lags}: worst |J − ref| / bound {worst:.3e}")
        ll, g = engine.loglik_grad(KIND_DNS, Th, T_use=tu)
        np.testing.assert_array_equal(r["ll"], ll)
        np.testing.assert_array_equal(r["grad"], g)


@pytest.mark.parametrize("name", MI.HESS_CASES)
def test_hessian_is_as_close_to_the_truth_as_the_fp64_reference(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"]
    r = engine.loglik_info(KIND_DNS, Th, opg=False)
    H = r["hess"]
    assert r["opg"] is None and engine.last_grad_unavailable() == 0
    np.testing.assert_array_equal(H, H.transpose(1, 0, 2))
    scale = np.abs(c["H_truth"]).max(axis=(0, 1))
    err = np.abs(H - c["H_truth"]).max(axis=(0, 1))
    for b in range(Th.shape[1]):
        print(f"case {name} candidate {b}: err/|H|max {err[b] / scale[b]:.3e}, plain FP64 reference's "
              f"{c['ref_err'][b] / scale[b]:.3e} (its step {c['ref_step'][b]:g}), e_fd/|H|max {c['e_fd'][b] / scale[b]:.3e}")
    assert np.all(err <= c["ref_err"] + c["e_fd"]), err / (c["ref_err"] + c["e_fd"])
    ll, g = engine.loglik_grad(KIND_DNS, Th)
    np.testing.assert_array_equal(r["ll"], ll)
    np.testing.assert_array_equal(r["grad"], g)
    # the same bits alone, and in a reversed batch with other candidates around
    for b in range(Th.shape[1]):
        np.testing.assert_array_equal(engine.loglik_info(KIND_DNS, Th[:, b], opg=False)["hess"][:, :, 0], H[:, :, b])
    big = np.asfortranarray(np.concatenate([S.theta_batch(KIND_DNS, 3, 0.1, 5, bad_frac=0), Th], axis=1)[:, ::-1])
    Hb = engine.loglik_info(KIND_DNS, big, opg=False)["hess"]
    np.testing.assert_array_equal(Hb[:, :, :Th.shape[1]][:, :, ::-1], H)


def test_a_perturbed_point_at_minus_inf_makes_the_hessian_unavailable(engine, cases):
    """Constrained space, σ² = 2h: the point σ² − 2h is exactly 0, a −Inf loglik; the candidate's own loglik and
    gradient are finite."""
    c = cases["H-E"]
    engine.set_panel(c["Y"], c["maturities"])
    h = 1e-3
    Tc = np.asfortranarray(transform_params(KIND_DNS, c["Theta"]))
    Tc[1, 1] = 2 * h
    assert np.isneginf(engine.loglik(KIND_DNS, np.r_[Tc[0, 1], 0.0, Tc[2:, 1]], space=1)[0])
    r = engine.loglik_info(KIND_DNS, Tc, space=1, step=h)
    assert engine.last_grad_unavailable() == 1
    assert engine.last_flags() == (0, 0)  # the batch's own counters, not those of its perturbed launches
    assert np.isfinite(r["ll"]).all() and np.isfinite(r["grad"]).all()
    assert np.isnan(r["hess"][:, :, 1]).all() and np.isfinite(r["hess"][:, :, 0]).all()
    assert np.isfinite(r["opg"]).all()  # the scores need the candidate's own point only
    # a candidate without a gradient of its own: NaN everywhere, counted once
    Tc[1, 0] = 0.0
    r = engine.loglik_info(KIND_DNS, Tc, space=1, step=h)
    assert engine.last_grad_unavailable() == 2 and np.isneginf(r["ll"][0]) and engine.last_flags() == (0, 1)
    assert np.isnan(r["hess"]).all() and np.isnan(r["opg"][:, :, 0]).all() and np.isfinite(r["opg"][:, :, 1]).all()
    for bad in (dict(lags=-1), dict(hessian=False, opg=False)):
        with pytest.raises(ValueError):
            engine.loglik_info(KIND_DNS, Tc, space=1, **bad)
    rc = engine.lib.yfm_loglik_info_batch(engine.ctx, KIND_DNS, 1, _lib.dptr(Tc), 20, 2, None, 0, 0.0,
                                          _lib.dptr(r["ll"]), _lib.dptr(r["grad"]), None, None)
    assert rc == -1 and b"both null" in engine.lib.yfm_last_error()
    rc = engine.lib.yfm_loglik_info_batch(engine.ctx, KIND_DNS, 1, _lib.dptr(Tc), 20, 2, None, -1, 0.0,
                                          _lib.dptr(r["ll"]), _lib.dptr(r["grad"]), _lib.dptr(r["hess"]), None)
    assert rc == -1 and b"lags" in engine.lib.yfm_last_error()


def test_batches_larger_than_one_chunk(engine, cases):
    """A large batch runs chunk by chunk (1,400 candidates per chunk of score scratch at T = 600, about
    3,800 per chunk of perturbed points, whose launch's work records are the largest buffer; the Hessian case runs at
    T = 3 to stay quick).  A candidate's bits must not depend on the chunk it falls into: the whole batch against the
    same candidates split 2 : 5 into two calls, whose chunk boundaries fall elsewhere."""
    m = cases["H-E"]["maturities"]
    for T, B, kw in ((600, 2 * 1400 + 3, dict(hessian=False, lags=2)), (3, 3 * 3900 + 4, dict(opg=False))):
        engine.set_panel(S.simulate_panel(KIND_DNS, T, m, 50 + T), m)
        Th = np.asfortranarray(np.tile(S.theta_batch(KIND_DNS, 7, 0.1, 51, bad_frac=0), (1, B // 7 + 1))[:, :B])
        Th[1, 5] = -800.0  # σ² = 0: one candidate per chunk or so is unavailable
        Th[1, B - 2] = -800.0
        r = engine.loglik_info(KIND_DNS, Th, **kw)
        key = "opg" if "lags" in kw else "hess"
        assert r[key].shape == (20, 20, B) and engine.last_grad_unavailable() == 2 and engine.last_flags() == (0, 2)
        assert np.isnan(r[key][:, :, [5, B - 2]]).all() and np.isfinite(np.delete(r[key], [5, B - 2], axis=2)).all()
        cut = 2 * B // 7
        parts = [engine.loglik_info(KIND_DNS, Th[:, :cut], **kw), engine.loglik_info(KIND_DNS, Th[:, cut:], **kw)]
        for name in (key, "grad", "ll"):
            np.testing.assert_array_equal(r[name], np.concatenate([p[name] for p in parts], axis=-1))
        np.testing.assert_array_equal(r[key][:, :, B - 1], r[key][:, :, (B - 1) % 7])  # the same θ in the first chunk
        if T == 600:  # the host-pointer scores call copies chunk by chunk too
            _, Sc = engine.loglik_scores(KIND_DNS, Th)
            _, Se = engine.loglik_scores(KIND_DNS, Th[:, 1398:1403])
            np.testing.assert_array_equal(Sc[:, :, 1398:1403], Se)


@pytest.fixture(scope="module")
def optimum():
    """One L-BFGS chain of tests/test_gpu_lbfgs.py's problem."""
    mats = S.maturities_30()[::3]
    Y = S.simulate_panel(KIND_DNS, 80, mats, seed=21)
    rng = np.random.Generator(np.random.PCG64(31))
    th0 = S.theta0(KIND_DNS)
    X0 = np.asfortranarray(th0[:, None] + 0.05 * rng.standard_normal((th0.size, 4)))
    model, _ = create_model("1C", mats, len(mats), 3)
    r = estimate_lbfgs_batch(model, Y, X0[:, :1], space=0, g_tol=1e-4, f_abstol=0.0)
    return model, Y, th0, r


def test_standard_errors_at_an_optimum_and_far_from_it(optimum):
    model, Y, th0, r = optimum
    assert r["ll"][0] >= 409.8591 - 1e-4
    for cov in ("hessian", "opg", "sandwich"):
        se = standard_errors_batch(model, Y, r["theta_c"], cov=cov)
        print(cov, "se_c", se["se_c"][:, 0])
        assert se["pd"].tolist() == [True] and se["unavailable"] == 0
        assert np.all(np.isfinite(se["se_c"])) and np.all(se["se_c"] > 0) and np.all(se["se_u"] > 0)
        np.testing.assert_array_equal(se["ll"], r["ll"])
        one = standard_errors_(model, Y, r["theta_c"][:, 0], cov=cov)
        np.testing.assert_array_equal(one["se_c"], se["se_c"][:, 0])
        assert one["pd"] is True
    for cov in ("hessian", "sandwich"):  # θ₀ is no maximum: −H is not positive definite there
        se = standard_errors_batch(model, Y, transform_params(KIND_DNS, th0), cov=cov)
        assert se["pd"].tolist() == [False] and np.isnan(se["se_c"]).all() and np.isnan(se["cov_u"]).all()
        assert np.isfinite(se["ll"]).all() and np.isfinite(se["grad"]).all()
