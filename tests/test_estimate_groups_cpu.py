"""CPU test of the block-coordinate descent over parameter groups (yfm_amd/groups.py: the outer loop of
estimate_steps!, src/optimization.jl:137-312) on stub evaluators: a separable quadratic f(x) = Σ wᵢ(xᵢ − tᵢ)² per
chain, a Nelder–Mead stand-in that moves its block a set fraction of the way to the target and records every call,
and the real batched L-BFGS on the quadratic's gradient."""
from __future__ import annotations

import numpy as np
import pytest

from yfm_amd import groups as G
from yfm_amd import models as M

P, N_LEAD = 6, 2
W = np.array([1.0, 2.0, 0.5, 1.5, 1.0, 3.0])


class Stub:
    """The three evaluators over R chains with targets T (P×R)."""

    def __init__(self, targets, nm_step=1.0, nm_fail=()):
        self.T = np.asarray(targets, dtype=np.float64)
        self.nm_step = np.broadcast_to(nm_step, (self.T.shape[1],)).astype(np.float64)
        self.nm_fail = set(nm_fail)  # (call number, chain) whose Nelder–Mead throws
        self.calls = []              # (what, rows, cols)
        self.nm_calls = 0
        self.infinite = lambda X, cols: np.zeros(X.shape[1], dtype=bool)

    def f(self, X, cols):
        v = np.sum(W[:, None] * (X - self.T[:, cols]) ** 2, axis=0)
        return np.where(self.infinite(X, cols), np.inf, v)

    def value(self, X, cols):
        self.calls.append(("value", None, tuple(cols)))
        return self.f(X, cols)

    def value_grad(self, X, cols, rows):
        self.calls.append(("grad", tuple(rows), tuple(cols)))
        return self.f(X, cols), (2 * W[:, None] * (X - self.T[:, cols]))[rows]

    def nelder_mead(self, X, cols, rows, iterations, g_tol):
        self.nm_calls += 1
        self.calls.append(("nm", tuple(rows), tuple(cols)))
        assert iterations == 500 and g_tol == 1e-6  # opt1
        X = X.copy()
        X[rows] += self.nm_step[cols] * (self.T[np.ix_(rows, cols)] - X[rows])
        f = self.f(X, cols)
        for k, c in enumerate(cols):
            if (self.nm_calls, int(c)) in self.nm_fail:
                f[k] = np.nan
        return X, f, 7 * len(cols)


def run(stub, p0, groups, **kw):
    return G.descend(p0, groups, stub.value, stub.value_grad, stub.nelder_mead, N_LEAD, **kw)


def test_sorted_group_order_and_placeholder_skip():
    """Group ids run in sorted order whatever their order in param_groups; "-1" coordinates are never touched; an
    id without an optimiser of its own falls back to Nelder–Mead (optimization.jl:501-508)."""
    T = np.arange(1.0, 7.0)[:, None]
    stub = Stub(T)
    groups = ["4", "1", "2", "-1", "2", "9"]
    r = run(stub, np.zeros((P, 1)), groups, max_group_iters=1)
    opt = [(w, rows) for w, rows, _ in stub.calls if w == "nm" or (w == "grad" and rows)]
    seq = []
    for w, rows in opt:
        if not seq or seq[-1] != (w, rows):
            seq.append((w, rows))
    assert seq == [("nm", (1,)), ("grad", (2, 4)), ("nm", (0,)), ("nm", (5,))]  # "1", "2", "4", "9"
    assert r["p"][3, 0] == 0.0  # "-1"
    np.testing.assert_allclose(r["p"][[0, 1, 5], 0], T[[0, 1, 5], 0])
    np.testing.assert_allclose(r["p"][[2, 4], 0], T[[2, 4], 0], atol=1e-3)
    assert set(r["evals_by_group"]) == {"1", "2", "4", "9"} and r["evals_by_group"]["1"] == 7


@pytest.mark.parametrize("code,lead", [("NS", 1), ("SD-NS", 3), ("RWSD-NS", 2), ("SSD-NS", 3), ("SRWSD-NS", 2)])
def test_default_groups_per_kind(code, lead):
    """msebasemodel.jl:153-162, staticbasemodel.jl:103-112: "1" for the leading parameters, "2" for δ and Φ."""
    mats = np.array([3.0, 12.0, 60.0, 120.0])
    model, _ = M.create_model(code, mats, 4, 3)
    groups = M.get_param_groups(model)
    assert groups == ["1"] * lead + ["2"] * 12
    assert G.check_groups(groups, lead) == ["1", "2"]
    custom = ["4"] * lead + ["-1"] * 12
    assert M.get_param_groups(model, custom) == custom


def test_converged_chain_drops_out_while_others_go_on():
    """Chain 0 reaches its optimum in iteration 1, so |ΔLL| < tol stops it after iteration 2; chain 1's Nelder–Mead
    only moves half-way each time and keeps going: later calls carry chain 1 alone."""
    T = np.stack([np.arange(1.0, 7.0), -np.arange(1.0, 7.0)], axis=1)
    stub = Stub(T, nm_step=[1.0, 0.5])
    groups = ["1"] * N_LEAD + ["2"] * (P - N_LEAD)
    r = run(stub, np.zeros((P, 2)), groups, max_group_iters=6, tol=1e-8)
    assert r["group_iters"][0] == 2 and r["group_iters"][1] == 6
    nm_cols = [cols for w, _, cols in stub.calls if w == "nm"]
    assert nm_cols == [(0, 1), (0, 1), (1,), (1,), (1,), (1,)]
    assert np.all(r["status"] == 0)
    # ll is −loss at the returned parameters, for both
    np.testing.assert_array_equal(r["ll"], -stub.f(r["p"], np.array([0, 1])))
    assert r["ll"][0] > -1e-5 and r["ll"][1] < r["ll"][0]


def test_sanitising_and_rescaling():
    """Non-finite entries of the start become 0; a start whose loss is not finite is multiplied by 0.95 until it is,
    at most 10 times; the result's `init` is that start."""
    T = np.ones((P, 3))
    stub = Stub(T)
    stub.infinite = lambda X, cols: np.abs(X[0]) > 1.5
    p0 = np.ones((P, 3))
    p0[0] = [2.0, 1.0, 1e6]
    p0[1, 1] = np.nan
    p0[2, 1] = -np.inf
    r = run(stub, p0, ["1"] * P, max_group_iters=1)
    k = int(np.ceil(np.log(1.5 / 2.0) / np.log(0.95)))  # 6 rescalings bring 2.0 under 1.5
    np.testing.assert_allclose(r["init"][:, 0], np.r_[2.0, 1, 1, 1, 1, 1] * 0.95 ** k)
    np.testing.assert_array_equal(r["init"][:, 1], [1.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    np.testing.assert_allclose(r["init"][:, 2], np.r_[1e6, 1, 1, 1, 1, 1] * 0.95 ** 10)  # never finite: 10, then on
    first = [cols for w, _, cols in stub.calls if w == "value"][:11]
    assert first[0] == (0, 1, 2) and first[1] == (0, 2) and first[k] == (0, 2) and first[k + 1] == (2,)
    assert len(first) == 11 and first[10] == (2,)


def test_abort_after_first_iteration_keeps_parameters():
    """An optimiser that throws after iteration 1 ends the chain with the parameters and the ll it has
    (optimization.jl:249-257): status 2; the other chain is unaffected."""
    T = np.stack([np.arange(1.0, 7.0), -np.arange(1.0, 7.0)], axis=1)
    stub = Stub(T, nm_step=0.5, nm_fail={(2, 1)})  # the second Nelder–Mead call throws for chain 1
    groups = ["1"] * N_LEAD + ["2"] * (P - N_LEAD)
    r = run(stub, np.zeros((P, 2)), groups, max_group_iters=3)
    assert r["status"].tolist() == [0, 2]
    # chain 1: the leading block after one half-step, δ/Φ from iteration 1's L-BFGS, ll of iteration 1
    np.testing.assert_allclose(r["p"][:N_LEAD, 1], 0.5 * T[:N_LEAD, 1])
    assert r["group_iters"][1] == 2
    after_one = r["p"][:, 1].copy()
    assert r["ll"][1] == -stub.f(after_one[:, None], np.array([1]))[0]
    assert r["group_iters"][0] == 3


def test_error_on_first_iteration_raises():
    T = np.ones((P, 2))
    stub = Stub(T, nm_fail={(1, 0)})
    with pytest.raises(G.EstimationError):
        run(stub, np.zeros((P, 2)), ["1"] * P)
    assert M.EstimationError is G.EstimationError


@pytest.mark.parametrize("groups,why", [
    (["1", "1", "3", "2", "2", "2"], "Adam"),
    (["1", "1", "2", "2", "2", "5"], "Adam"),
    (["1", "2", "2", "2", "2", "2"], "leading"),
])
def test_unsupported_groups_raise(groups, why):
    stub = Stub(np.ones((P, 1)))
    with pytest.raises(NotImplementedError, match=why):
        run(stub, np.zeros((P, 1)), groups)
    assert not stub.calls  # refused before any evaluation


def test_lambda_model_refusals_need_no_device():
    """estimate_steps_batch refuses unsupported groups and Kalman models before it touches the engine."""
    mats = np.array([3.0, 12.0, 60.0, 120.0])
    model, _ = M.create_model("SD-NS", mats, 4, 3)
    Y = np.zeros((4, 8))
    with pytest.raises(NotImplementedError, match="Adam"):
        M.estimate_steps_batch(model, Y, np.zeros((15, 1)), param_groups=["1"] * 3 + ["3"] * 12)
    with pytest.raises(NotImplementedError, match="leading"):
        M.estimate_steps_batch(model, Y, np.zeros((15, 1)), param_groups=["2"] * 15)
    dns, _ = M.create_model("1C", mats, 4, 3)
    with pytest.raises(NotImplementedError):
        M.estimate_steps_batch(dns, Y, np.zeros((20, 1)))
