"""GPU test of the batched L-BFGS estimate on the TVλ model (yfm_amd.lbfgs over yfm_tvl_loglik_grad_batch;
models.estimate_ mirrors estimate!, optimization.jl:329-410) — the TVλ twin of tests/test_gpu_lbfgs.py.

Panel simulate_panel(TVλ, 80, maturities_30()[::3], seed 21); four starts θ₀ + 0.02·N(0, I) from PCG64(31);
g_tol = 1e-4, f_abstol = 0.  LL_OPT is the best that scipy's L-BFGS-B, driven by forward differences (eps = 1e-6)
of the dense FP64 C oracle, reaches from the same four starts on the CPU (its optima: 294.2346 and −2696.0090 —
two starts where the differences give it no descent direction —, 398.5098 and 386.0101; ll(θ₀) = 368.0633):

    python - <<'PY'
    import numpy as np; from scipy.optimize import minimize
    from oracle import truth as TR; from yfm_amd import KIND_TVL, synthetic as S
    m = S.maturities_30()[::3]; Y = S.simulate_panel(KIND_TVL, 80, m, 21); th0 = S.theta0(KIND_TVL)
    X0 = th0[:, None] + 0.02 * np.random.Generator(np.random.PCG64(31)).standard_normal((th0.size, 4))
    f = lambda x: -TR.loglik_oracle(KIND_TVL, Y, m, x[:, None], space=0)[0]
    for k in range(4):
        print(-minimize(f, X0[:, k], method="L-BFGS-B", options=dict(maxiter=3000, maxfun=400000, ftol=1e-15,
                                                                     gtol=1e-6, eps=1e-6)).fun)
    PY

No parity with Optim.jl's iterates is claimed: the driver is judged on the optimum.
"""
from __future__ import annotations

import numpy as np
import pytest

from grad_rule import SPACE_ROWS
from yfm_amd import KIND_TVL, create_model, estimate_, estimate_lbfgs_batch
from yfm_amd import synthetic as S
from yfm_amd.params import transform_params

pytestmark = pytest.mark.gpu

LL_THETA0, LL_OPT = 368.0633, 398.5098
OPTS = dict(g_tol=1e-4, f_abstol=0.0)
POS, R11 = (list(rows) for rows in SPACE_ROWS[KIND_TVL][:2])


@pytest.fixture(scope="module")
def problem():
    mats = S.maturities_30()[::3]
    Y = S.simulate_panel(KIND_TVL, 80, mats, seed=21)
    rng = np.random.Generator(np.random.PCG64(31))
    th0 = S.theta0(KIND_TVL)
    X0 = np.asfortranarray(th0[:, None] + 0.02 * rng.standard_normal((th0.size, 4)))
    model, _ = create_model("TVλ", mats, len(mats), 4)
    return model, Y, th0, X0


@pytest.fixture(scope="module")
def chains(problem):
    # from the constrained starts, as estimate_ passes them: the chains have not converged at the iteration limit,
    # so a start that differs in its last bit (θ → θ_c → θ) ends a little elsewhere
    model, Y, th0, X0 = problem
    return estimate_lbfgs_batch(model, Y, transform_params(KIND_TVL, X0), space=1, **OPTS)


def test_chains_reach_the_optimum(engine, problem, chains):
    model, Y, th0, X0 = problem
    engine.set_panel(Y, model.base.maturities)
    ll_th0 = engine.loglik(KIND_TVL, th0)[0]
    print("ll(theta0)", ll_th0, "starts", chains["ll0"], "optima", chains["ll"], "iterations", chains["iterations"],
          "status", chains["status"], "evals", chains["n_evals"], "rounds", chains["rounds"])
    assert abs(ll_th0 - LL_THETA0) <= 1e-4
    assert np.all(chains["ll"] >= chains["ll0"])
    assert chains["ll"].max() >= LL_OPT - 1e-4
    # the returned optimum is what the library evaluates there
    np.testing.assert_array_equal(engine.loglik(KIND_TVL, chains["p"]), chains["ll"])
    np.testing.assert_array_equal(chains["theta_c"], transform_params(KIND_TVL, chains["p"]))


def test_estimate_returns_the_best_start_constrained(problem, chains):
    model, Y, th0, X0 = problem
    init_p, ll, best_p, ir = estimate_(model, Y, transform_params(KIND_TVL, X0), **OPTS)
    j = int(np.argmax(chains["ll"]))
    assert ll >= LL_OPT - 1e-4 and abs(ll - chains["ll"][j]) <= 1e-4
    assert ir in (0, 1)
    # constrained outputs: σ² and the U diagonal positive, the Φ diagonal inside (−1, 1)
    assert np.all(best_p[POS] > 0) and np.all(np.abs(best_p[R11]) < 1)
    np.testing.assert_array_equal(init_p, chains["init_c"][:, j])
    np.testing.assert_array_equal(best_p, chains["theta_c"][:, j])


def test_one_chain_per_window(problem):
    """T_use runs chain r on data[:, :T_use[r]]: the full-window chain repeats the plain call, bit for bit."""
    model, Y, th0, X0 = problem
    opts = dict(OPTS, iterations=3)
    a = estimate_lbfgs_batch(model, Y, X0[:, :2], space=0, **opts)
    b = estimate_lbfgs_batch(model, Y, X0[:, :2], space=0, T_use=np.array([80, 40]), **opts)
    np.testing.assert_array_equal(a["ll"][0], b["ll"][0])
    np.testing.assert_array_equal(a["p"][:, 0], b["p"][:, 0])
    assert b["ll"][1] != a["ll"][1] and b["ll"][1] >= b["ll0"][1]
