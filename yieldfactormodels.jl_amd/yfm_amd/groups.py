"""Block-coordinate descent over parameter groups: the outer loop of the reference's ``estimate_steps!``
(``src/optimization.jl:137-312``) for R chains advancing in lockstep, with the objective behind three callables so
that the group logic runs — and is tested — without a device.

Per chain the reference does (after ``try_initializations`` and ``untransform_params``, which the caller does):

* ``_sanitize_parameters`` (:157-162, :422-432): non-finite entries become 0;
* while the loss at the start is not finite, at most 10 times: ``p .*= 0.95`` (:170-184);
* for ``iter in 1:max_group_iters`` and each group id in sorted order, skipping ``"-1"`` (:218-261): optimise the
  group's coordinates with the group's optimiser (``_create_optimizer_dict`` :439-494) — ``"2"`` L-BFGS with
  BackTracking(order = 3) and ``opt2``, ``"3"`` / ``"5"`` Adam, every other id Nelder–Mead with ``opt1`` (``"1"``,
  ``"4"``, and the fallback of ``_get_optimizer_for_group`` :501-508);
* an optimiser that throws is rethrown on iteration 1 and otherwise ends the chain with the parameters it has
  (:249-257);
* after the groups: ``ll = -loss(p)``, stop when ``|ll - prev_ll| < tol`` (:268-279).

Here every step is taken for all unfinished chains at once; a finished chain drops out of the later calls.
"""
from __future__ import annotations

import numpy as np

from . import lbfgs as _lbfgs

# _create_optimizer_dict (optimization.jl:442-462)
NM_ITERATIONS, NM_G_TOL = 500, 1e-6
LBFGS_OPTIONS = dict(iterations=250, g_tol=1e-6, f_abstol=1e-6, allow_f_increases=False)
ADAM_GROUPS = ("3", "5")

OK, ABORTED = 0, 2  # chain status, as yfm_estimate's (its 1, "the reference throws", is raised here)


class EstimationError(RuntimeError):
    """estimate_steps! rethrows from the first group iteration (optimization.jl:249-253); estimate! throws
    where compute_loss does."""


def check_groups(param_groups, n_lead: int) -> list:
    """The sorted group ids estimate_steps! walks (optimization.jl:150, "-1" skipped), after refusing what is not
    built: the Adam groups, and an L-BFGS group that holds one of the n_lead leading parameters."""
    groups = [str(g) for g in param_groups]
    ids = [g for g in sorted(set(groups)) if g != "-1"]
    for g in ids:
        if g in ADAM_GROUPS:
            raise NotImplementedError(f"parameter group \"{g}\" uses Optim.Adam (optimization.jl:481-489), which is "
                                      "not built")
        if g == "2" and any(k < n_lead for k, x in enumerate(groups) if x == "2"):
            raise NotImplementedError("an L-BFGS group (\"2\") that holds a leading parameter needs the tangent of "
                                      "the score recursion with respect to it, which is not built: only δ and Φ "
                                      "have a gradient")
    return ids


def sanitize(p: np.ndarray) -> np.ndarray:
    """_sanitize_parameters (optimization.jl:422-432)"""
    return np.where(np.isfinite(p), p, 0.0)


def descend(p0, param_groups, value, value_grad, nelder_mead, n_lead: int, max_group_iters: int = 10,
            tol: float = 1e-8, nm_iterations: int = NM_ITERATIONS, lbfgs_options: dict | None = None) -> dict:
    """p0: P×R unconstrained starts.  Evaluators, each told which chains (``cols``, indices into R — a chain's
    window is the evaluator's business) the columns of its batch belong to:

    * ``value(X, cols) -> f[B]``: compute_loss;
    * ``value_grad(X, cols, rows) -> (f[B], G[len(rows), B])``: compute_loss and its gradient rows ``rows``;
    * ``nelder_mead(X, cols, rows, iterations, g_tol) -> (X', f[B], n_evals)``: Optim.NelderMead on the coordinates
      ``rows`` of every column, f NaN where the objective threw.

    Returns p (P×R), init (P×R: the sanitised, rescaled starts), ll (R), status (R), n_evals, evals_by_group
    ({id: evaluations}), rounds_by_group ({id: launches of an L-BFGS group, calls of a Nelder–Mead group}) and
    group_iters (R: outer iterations a chain ran)."""
    p = sanitize(np.array(p0, dtype=np.float64, order="F"))
    if p.ndim == 1:
        p = p[:, None]
    P, R = p.shape
    groups = [str(g) for g in param_groups]
    if len(groups) != P:
        raise ValueError(f"{len(groups)} parameter groups for {P} parameters")
    ids = check_groups(groups, n_lead)
    opts = dict(LBFGS_OPTIONS if lbfgs_options is None else lbfgs_options)
    n_evals = 0
    evals_by_group = {g: 0 for g in ids}
    rounds_by_group = {g: 0 for g in ids}

    # the start: ×0.95 while the loss is not finite, at most 10 times (optimization.jl:170-184)
    todo = np.arange(R)
    for k in range(11):
        f = np.asarray(value(p[:, todo], todo), dtype=np.float64)
        n_evals += len(todo)
        todo = todo[~np.isfinite(f)]
        if k == 10 or todo.size == 0:
            break
        p[:, todo] *= 0.95
    init = p.copy()

    status = np.zeros(R, dtype=np.int32)
    prev_ll = np.full(R, -np.inf)
    group_iters = np.zeros(R, dtype=np.int32)
    live = np.arange(R)
    for it in range(1, max_group_iters + 1):
        if live.size == 0:
            break
        group_iters[live] = it
        for g in ids:
            if live.size == 0:
                break
            rows = np.array([k for k, x in enumerate(groups) if x == g])
            if g == "2":
                def fun(Xsub, idx, cols=live, rows=rows):
                    c = cols[np.asarray(idx)]
                    X = p[:, c].copy(order="F")
                    X[rows] = Xsub
                    return value_grad(X, c, rows)
                r = _lbfgs.minimize_batch(fun, p[np.ix_(rows, live)], with_index=True, **opts)
                bad = r["status"] == _lbfgs.BAD_START
                block = r["x"]
                evals_by_group[g] += r["n_evals"]
                rounds_by_group[g] += r["rounds"]
                n_evals += r["n_evals"]
            else:
                X, f, ne = nelder_mead(p[:, live].copy(order="F"), live, rows, nm_iterations, NM_G_TOL)
                bad = np.isnan(np.asarray(f, dtype=np.float64))
                block = np.asarray(X)[rows]
                evals_by_group[g] += int(ne)
                rounds_by_group[g] += 1
                n_evals += int(ne)
            if bad.any():
                # the optimiser threw: rethrown on the first iteration, later the chain keeps its parameters
                # and stops (optimization.jl:249-257)
                if it == 1:
                    raise EstimationError(f"optimising group \"{g}\" failed on the first group iteration "
                                          f"(chains {live[bad].tolist()})")
                status[live[bad]] = ABORTED
            good = ~bad
            p[np.ix_(rows, live[good])] = block[:, good]
            live = live[good]
        if live.size == 0:
            break
        ll = -np.asarray(value(p[:, live], live), dtype=np.float64)
        n_evals += len(live)
        with np.errstate(invalid="ignore"):
            done = np.abs(ll - prev_ll[live]) < tol
        prev_ll[live] = ll
        live = live[~done]
    return dict(p=np.asfortranarray(p), init=np.asfortranarray(init), ll=prev_ll, status=status, n_evals=n_evals,
                evals_by_group=evals_by_group, rounds_by_group=rounds_by_group, group_iters=group_iters)
