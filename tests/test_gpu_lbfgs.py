"""GPU test of the batched L-BFGS estimate (yfm_amd.lbfgs over yfm_loglik_grad_batch; models.estimate_ mirrors
estimate!, optimization.jl:329-410).

Panel simulate_panel(DNS, 80, maturities_30()[::3], seed 21); four starts θ₀ + 0.05·N(0, I) from PCG64(31);
g_tol = 1e-4, f_abstol = 0.  ll(θ₀) = 387.1434; scipy's L-BFGS driven by differences of the dense C oracle
reaches 409.8591 from all four starts in about 600 iterations (a CPU run), which the driver must reach or beat.
No parity with Optim.jl's iterates is claimed: the driver is judged on the optimum.
"""
from __future__ import annotations

import numpy as np
import pytest

from yfm_amd import KIND_DNS, create_model, estimate_, estimate_lbfgs_batch
from yfm_amd import synthetic as S
from yfm_amd.params import transform_params

pytestmark = pytest.mark.gpu

LL_THETA0, LL_OPT = 387.1434, 409.8591
OPTS = dict(g_tol=1e-4, f_abstol=0.0)


@pytest.fixture(scope="module")
def problem():
    mats = S.maturities_30()[::3]
    Y = S.simulate_panel(KIND_DNS, 80, mats, seed=21)
    rng = np.random.Generator(np.random.PCG64(31))
    th0 = S.theta0(KIND_DNS)
    X0 = np.asfortranarray(th0[:, None] + 0.05 * rng.standard_normal((th0.size, 4)))
    model, _ = create_model("1C", mats, len(mats), 3)
    return model, Y, th0, X0


@pytest.fixture(scope="module")
def chains(problem):
    model, Y, th0, X0 = problem
    return estimate_lbfgs_batch(model, Y, X0, space=0, **OPTS)


def test_chains_reach_the_optimum(engine, problem, chains):
    model, Y, th0, X0 = problem
    engine.set_panel(Y, model.base.maturities)
    ll_th0 = engine.loglik(KIND_DNS, th0)[0]
    print("ll(theta0)", ll_th0, "starts", chains["ll0"], "optima", chains["ll"], "iterations", chains["iterations"],
          "status", chains["status"], "evals", chains["n_evals"], "rounds", chains["rounds"])
    assert abs(ll_th0 - LL_THETA0) <= 1e-4
    assert np.all(chains["ll"] >= chains["ll0"]) and np.all(chains["ll"] > ll_th0)
    assert chains["ll"].max() - chains["ll"].min() <= 1e-4
    assert chains["ll"].max() >= LL_OPT - 1e-4
    # every live chain's trial point shares one launch per round
    assert chains["rounds"] < chains["n_evals"] / 2
    # the returned optimum is what the library evaluates there
    np.testing.assert_array_equal(engine.loglik(KIND_DNS, chains["p"]), chains["ll"])
    np.testing.assert_array_equal(chains["theta_c"], transform_params(KIND_DNS, chains["p"]))


def test_estimate_returns_the_best_start_constrained(problem, chains):
    model, Y, th0, X0 = problem
    init_p, ll, best_p, ir = estimate_(model, Y, transform_params(KIND_DNS, X0), **OPTS)
    j = int(np.argmax(chains["ll"]))
    assert ll >= LL_OPT - 1e-4 and abs(ll - chains["ll"][j]) <= 1e-4
    assert ir in (0, 1)
    # constrained outputs: σ² and the U diagonal positive, the Φ diagonal inside (−1, 1)
    assert np.all(best_p[[1, 2, 4, 7]] > 0) and np.all(np.abs(best_p[[11, 15, 19]]) < 1)
    k = int(np.argmin(np.abs(transform_params(KIND_DNS, X0) - init_p[:, None]).max(axis=0)))
    np.testing.assert_allclose(init_p, transform_params(KIND_DNS, X0[:, k]), rtol=1e-12)
