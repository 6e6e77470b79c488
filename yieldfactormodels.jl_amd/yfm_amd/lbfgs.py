"""Batched L-BFGS with a backtracking line search: the optimiser of the reference's ``estimate!``
(``src/optimization.jl:329-410``: ``Optim.LBFGS(linesearch = BackTracking(order=3))``), run for many
chains in lockstep over one batched objective

    value_and_grad(X: P×B) -> (f[B], G[P, B])          (minimised; column b belongs to chain b)

so that every round costs one device launch whatever the number of chains.

* Memory 10; the initial inverse Hessian of every two-loop recursion is (s'y / y'y)·I of the newest pair;
  the first direction of a chain is −g.  Every line search starts at α = 1.
* Backtracking Armijo (c₁ = 1e-4): the first backtrack interpolates quadratically, later ones cubically
  through the last two trials, and the new step is clamped to [0.1, 0.5]·α.  α is halved while the trial
  value is not finite; a NaN gradient at a finite value is a failed trial too (halve, not interpolate).
* Stopping, per chain: ‖g‖∞ ≤ g_tol, |Δf| ≤ f_abstol, `iterations`, or a line search that finds no step
  (``max_linesearch`` trials).  A finished chain drops out of the batch.
* A start whose value is not finite is rescaled x ← 0.95·x (at most 10 times), the sanitising step of the
  reference's ``estimate_steps!`` (``optimization.jl:173-184``); ``estimate!`` itself has none.

The iterates are not claimed to equal Optim.jl's (its initial step, its interpolation safeguards and its
convergence bookkeeping differ in detail); the driver is judged on the optimum it reaches.  Every chain's
arithmetic uses its own column only, so a chain's result does not depend on which chains run beside it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

MEMORY = 10
C1 = 1e-4
RHO_LO, RHO_HI = 0.1, 0.5

# chain status
RUNNING, CONVERGED, MAX_ITER, LINESEARCH_FAILED, BAD_START = -1, 0, 1, 2, 3


@dataclass
class _Chain:
    x: np.ndarray
    f: float = math.nan
    g: np.ndarray = None
    S: list = field(default_factory=list)
    Y: list = field(default_factory=list)
    d: np.ndarray = None
    dphi0: float = 0.0
    alpha: float = 1.0
    prev: tuple = None  # (α, φ) of the last finite trial that failed Armijo
    trials: int = 0
    it: int = 0
    rescales: int = 0
    status: int = RUNNING
    x_try: np.ndarray = None

    def direction(self):
        """d = −H g by the two-loop recursion; steepest descent when there is no (usable) history."""
        q = self.g.copy()
        k = len(self.S)
        a = [0.0] * k
        rho = [1.0 / float(np.dot(self.Y[i], self.S[i])) for i in range(k)]
        for i in range(k - 1, -1, -1):
            a[i] = rho[i] * float(np.dot(self.S[i], q))
            q -= a[i] * self.Y[i]
        if k:
            q *= float(np.dot(self.S[-1], self.Y[-1])) / float(np.dot(self.Y[-1], self.Y[-1]))
        for i in range(k):
            b = rho[i] * float(np.dot(self.Y[i], q))
            q += (a[i] - b) * self.S[i]
        d = -q
        dphi0 = float(np.dot(self.g, d))
        if not (dphi0 < 0.0) or not np.all(np.isfinite(d)):
            self.S.clear()
            self.Y.clear()
            d = -self.g
            dphi0 = float(np.dot(self.g, d))
        self.d, self.dphi0 = d, dphi0
        self.alpha, self.prev, self.trials = 1.0, None, 0

    def backtrack(self, phi: float):
        """the next α after a finite trial value φ(α) that failed the Armijo test"""
        a2, f0, g0 = self.alpha, self.f, self.dphi0
        if self.prev is None:
            tmp = -(g0 * a2 * a2) / (2.0 * (phi - f0 - g0 * a2))
        else:
            a1, p1 = self.prev
            div = 1.0 / (a1 * a1 * a2 * a2 * (a2 - a1))
            r2, r1 = phi - f0 - g0 * a2, p1 - f0 - g0 * a1
            a = (a1 * a1 * r2 - a2 * a2 * r1) * div
            b = (-a1 * a1 * a1 * r2 + a2 * a2 * a2 * r1) * div
            if a == 0.0:
                tmp = g0 / (2.0 * b)
            else:
                tmp = (-b + math.sqrt(max(b * b - 3.0 * a * g0, 0.0))) / (3.0 * a)
        self.prev = (a2, phi)
        if not math.isfinite(tmp):
            tmp = a2 * RHO_HI
        self.alpha = max(min(tmp, a2 * RHO_HI), a2 * RHO_LO)


def minimize_batch(value_and_grad, X0, iterations: int = 1000, g_tol: float = 1e-6, f_abstol: float = 1e-6,
                   allow_f_increases: bool = True, max_linesearch: int = 60, with_index: bool = False) -> dict:
    """Minimise from every column of X0 (P×B).  Returns x (P×B), f (B), g (P×B), x0 (P×B: the starts after
    any rescaling), iterations (B), status (B: 0 converged, 1 iteration limit, 2 line search failed, 3 no finite
    start), converged (B), n_evals, rounds.  `allow_f_increases` is accepted for the reference's option set;
    the Armijo test never accepts an increase.  `with_index`: the objective is called as
    value_and_grad(X, idx), idx naming the chain of every column of X (finished chains drop out of the batch)."""
    X0 = np.array(X0, dtype=np.float64, order="F")
    if X0.ndim == 1:
        X0 = X0[:, None]
    P, B = X0.shape
    chains = [_Chain(x=X0[:, b].copy()) for b in range(B)]
    n_evals = rounds = 0

    def evaluate(idx, cols):
        nonlocal n_evals, rounds
        X = np.asfortranarray(np.stack(cols, axis=1))
        f, G = value_and_grad(X, idx) if with_index else value_and_grad(X)
        n_evals += len(idx)
        rounds += 1
        return np.asarray(f, dtype=np.float64), np.asarray(G, dtype=np.float64)

    # starts: rescale the ones whose value is not finite
    todo = list(range(B))
    while todo:
        f, G = evaluate(todo, [chains[b].x for b in todo])
        nxt = []
        for k, b in enumerate(todo):
            c = chains[b]
            if math.isfinite(f[k]) and np.all(np.isfinite(G[:, k])):
                c.f, c.g = float(f[k]), G[:, k].copy()
            elif c.rescales < 10:
                c.rescales += 1
                c.x = c.x * 0.95
                nxt.append(b)
            else:
                c.f, c.g, c.status = float(f[k]), G[:, k].copy(), BAD_START
        todo = nxt
    x0 = np.stack([c.x.copy() for c in chains], axis=1)
    for c in chains:
        if c.status == RUNNING:
            if float(np.max(np.abs(c.g))) <= g_tol:
                c.status = CONVERGED
            elif iterations <= 0:
                c.status = MAX_ITER
            else:
                c.direction()

    while True:
        live = [b for b in range(B) if chains[b].status == RUNNING]
        if not live:
            break
        for b in live:
            c = chains[b]
            c.x_try = c.x + c.alpha * c.d
        f, G = evaluate(live, [chains[b].x_try for b in live])
        for k, b in enumerate(live):
            c = chains[b]
            phi, gk = float(f[k]), G[:, k]
            c.trials += 1
            usable = math.isfinite(phi) and bool(np.all(np.isfinite(gk)))
            if usable and phi <= c.f + C1 * c.alpha * c.dphi0:
                s, y = c.x_try - c.x, gk - c.g
                df = abs(phi - c.f)
                c.x, c.f, c.g = c.x_try, phi, gk.copy()
                c.it += 1
                if float(np.dot(s, y)) > 0.0:
                    c.S.append(s)
                    c.Y.append(y)
                    if len(c.S) > MEMORY:
                        c.S.pop(0)
                        c.Y.pop(0)
                if float(np.max(np.abs(c.g))) <= g_tol or df <= f_abstol:
                    c.status = CONVERGED
                elif c.it >= iterations:
                    c.status = MAX_ITER
                else:
                    c.direction()
                continue
            if c.trials >= max_linesearch:
                c.status = LINESEARCH_FAILED
            elif usable:
                c.backtrack(phi)
            else:
                c.alpha *= 0.5
    status = np.array([c.status for c in chains], dtype=np.int32)
    return dict(x=np.asfortranarray(np.stack([c.x for c in chains], axis=1)), f=np.array([c.f for c in chains]),
                g=np.asfortranarray(np.stack([c.g for c in chains], axis=1)), x0=np.asfortranarray(x0),
                iterations=np.array([c.it for c in chains], dtype=np.int32), status=status,
                converged=status == CONVERGED, n_evals=n_evals, rounds=rounds)
