"""CPU test of the batched L-BFGS driver (yfm_amd/lbfgs.py) on a host objective: the 20-dimensional convex
quadratic with the coupling terms of test_nm_tree_cpu.py's objective, +Inf (and a NaN gradient) for x[0] > 5.

* Six chains, one of which starts in the infinite region (it is rescaled ×0.95 into the finite one): every
  chain reaches the known minimiser — the solution of the quadratic's linear system — to 1e-8.
* A chain's result is bitwise the same whether the chains run together or alone.
"""
from __future__ import annotations

import numpy as np

from yfm_amd import lbfgs

R, N = 6, 20
W = np.array([1.0 + 0.25 * (i % 3) for i in range(N)])


CENTRE = np.array([0.1 * (i % 5) for i in range(N)])


def objective(X):
    """value_and_grad over the columns of X (one column at a time: a column's result is its own)"""
    f = np.empty(X.shape[1])
    G = np.empty_like(X)
    for k in range(X.shape[1]):
        x = X[:, k]
        if x[0] > 5.0:
            f[k], G[:, k] = np.inf, np.nan
            continue
        d = x - CENTRE
        f[k] = np.sum(W * d * d) + 0.05 * np.sum(x[:-1] * x[1:])
        g = 2.0 * W * d
        g[:-1] += 0.05 * x[1:]
        g[1:] += 0.05 * x[:-1]
        G[:, k] = g
    return f, G


def minimiser():
    A = np.diag(2.0 * W)
    for i in range(N - 1):
        A[i, i + 1] += 0.05
        A[i + 1, i] += 0.05
    return np.linalg.solve(A, 2.0 * W * CENTRE)


def start(r):
    p = np.array([(0.2 * ((i * 7 + r * 3) % 11)) / 11.0 - 0.1 for i in range(N)])
    if r == 0:
        p[0] = 6.0
    return p


OPTS = dict(g_tol=1e-11, f_abstol=0.0)


def test_chains_reach_the_minimiser_together_and_alone():
    X0 = np.stack([start(r) for r in range(R)], axis=1)
    assert np.isinf(objective(X0)[0][0])
    res = lbfgs.minimize_batch(objective, X0, **OPTS)
    assert res["converged"].all(), res["status"]
    assert res["x0"][0, 0] < 5.0 and np.array_equal(res["x0"][:, 1:], X0[:, 1:])
    for r in range(R):
        assert np.max(np.abs(res["x"][:, r] - minimiser())) <= 1e-8, r
        alone = lbfgs.minimize_batch(objective, X0[:, r:r + 1], **OPTS)
        assert np.array_equal(alone["x"][:, 0], res["x"][:, r]) and alone["f"][0] == res["f"][r], r
        assert alone["iterations"][0] == res["iterations"][r]
    # one objective call per round for all live chains
    assert res["rounds"] < res["n_evals"]


def test_defaults_are_the_references():
    import inspect
    d = {k: v.default for k, v in inspect.signature(lbfgs.minimize_batch).parameters.items()}
    assert (d["iterations"], d["g_tol"], d["f_abstol"], d["allow_f_increases"]) == (1000, 1e-6, 1e-6, True)
    assert (lbfgs.MEMORY, lbfgs.C1, lbfgs.RHO_LO, lbfgs.RHO_HI) == (10, 1e-4, 0.1, 0.5)


def test_line_search_failure_and_bad_start_are_reported():
    # a start that stays infinite after ten rescalings
    res = lbfgs.minimize_batch(lambda X: (np.full(X.shape[1], np.inf), np.full_like(X, np.nan)), np.ones((3, 1)))
    assert res["status"][0] == lbfgs.BAD_START and not res["converged"][0]
    # a finite value whose gradient is NaN away from the start: every trial fails, the chain keeps its start
    def vg(X):
        at0 = np.all(X == 1.0, axis=0)
        return np.sum(X * X, axis=0), np.where(at0[None, :], 2.0 * X, np.nan)
    res = lbfgs.minimize_batch(vg, np.ones((3, 1)), max_linesearch=30)
    assert res["status"][0] == lbfgs.LINESEARCH_FAILED and np.array_equal(res["x"][:, 0], np.ones(3))
