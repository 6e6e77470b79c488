"""The gradient rule of the fixtures of central differences, once, and the chain factor between the parameter spaces.

    max_i |g − g_fd| ≤ rel·‖g_fd‖∞ + e_fd[b]

g_fd are central differences of the high-precision truth, e_fd the bound of their own error (tests/golden/*/make_*.py).
The batch form reads a case of the DNS and TVλ fixtures (fields g_fd, e_fd, compared, …); the per-candidate form is the
λ and neural fixtures', where a −Inf loss is stored as a NaN column.  What a family asserts beyond the bound is a
keyword its call site passes (DESIGN.md §3.14a holds the map)."""
from __future__ import annotations

import numpy as np

from yfm_amd import KIND_DNS, KIND_TVL

REL = 1e-9  # the project's parity bar, norm-wise


def assert_gradient_rule(g, c, *, label="", sel=None, rel=REL, min_compared=0.75, second_clause=None,
                         short_windows_zero=False, primal=None, primal_mask=None, primal_asserted=True):
    """The rule on g[P, B] over the candidates of `sel` (default: the case's `compared`, of which there must be at
    least min_compared), and exact zeros where g_fd == 0.  The observations are printed before anything is asserted.

    second_clause       a mask of candidates that may instead have err ≤ ref_err[b] (the `hard` ones of L-hard)
    short_windows_zero  every row of a candidate with T_use ≤ 2 is exactly 0.0, compared or not
    primal              the FP64 loglik beside the gradient: within rel of loglik_truth over primal_mask (default: where
                        the truth is finite), asserted unless primal_asserted=False (then printed only)"""
    cmp_ = c["compared"]
    assert cmp_.mean() >= min_compared
    sel = cmp_ if sel is None else sel
    gn = np.abs(c["g_fd"]).max(axis=0)
    err = np.abs(g - c["g_fd"]).max(axis=0)
    bound = rel * gn + c["e_fd"]
    nz = sel & (gn > 0)
    print(f"{label}: compared {int(cmp_.sum())}/{cmp_.size}, checked {int(sel.sum())}, max err/bound "
          f"{np.max(err[nz] / bound[nz]):.3e}, max err/|g| {np.max(err[nz] / gn[nz]):.3e}")
    ok = err <= bound
    if second_clause is not None:
        for b in np.flatnonzero(second_clause & sel):
            print(f"{label}: hard candidate {b}: err/|g| {err[b] / gn[b]:.3e}, err/bound {err[b] / bound[b]:.3e}, "
                  f"plain FP64 reference's err/|g| {c['ref_err'][b] / gn[b]:.3e}")
        ok = ok | (second_clause & (err <= c["ref_err"]))
    assert np.all(ok[sel]), (np.flatnonzero(sel & ~ok), (err / gn)[sel & ~ok])
    assert np.all(g[(c["g_fd"] == 0.0) & sel[None, :]] == 0.0)
    if short_windows_zero:
        assert np.all(g[:, c["T_use"] <= 2] == 0.0)
    if primal is not None:
        truth = c["loglik_truth"]
        fin = np.isfinite(truth) & (True if primal_mask is None else primal_mask)
        r = np.abs(primal[fin] - truth[fin]) / np.maximum(np.abs(truth[fin]), 1e-300)
        print(f"{label}: FP64 primal, max |ll − truth| / |truth| over {int(fin.sum())} candidates {r.max():.3e}")
        assert not primal_asserted or np.all(r <= rel)


def assert_candidate_rule(g, g_fd, e_fd, loss, label="", rel=REL):
    """The rule per candidate (column) over the rows the fixture stores (the leading g_fd.shape[0] of g); the NaN
    pattern of g must be the fixture's, which is the −Inf pattern of the loss.  Returns the worst error relative to
    ‖g_fd‖∞."""
    worst = 0.0
    nl = g_fd.shape[0]
    for b in range(g.shape[1]):
        if np.isnan(g_fd[:, b]).any():
            assert np.isneginf(loss[b]) and np.isnan(g[:, b]).all(), (label, b, loss[b], g[:, b])
            continue
        assert np.isfinite(loss[b]) and np.isfinite(g[:, b]).all(), (label, b, loss[b], g[:, b])
        err = np.max(np.abs(g[:nl, b] - g_fd[:, b]))
        scale = np.max(np.abs(g_fd[:, b]))
        bound = rel * scale + e_fd[b]
        print(f"{label} b={b}: max|g - g_fd| = {err:.3e}, bound {bound:.3e}, |g|inf = {scale:.3e}")
        assert err <= bound, (label, b, err, bound)
        worst = max(worst, err / scale)
    return worst


# kind → (rows of θ the constrained space takes exp of, rows of the diagonal of Φ: 2eˣ/(1+eˣ) − 1, row of σ²)
SPACE_ROWS = {
    KIND_DNS: ((1, 2, 4, 7), (11, 15, 19), 1),
    KIND_TVL: ((0, 1, 3, 6, 10), (15, 20, 25, 30), 0),
}


def chain_factor(kind, Theta_c):
    """dθ_c/dθ at the constrained Theta_c[P, …]: θ_c on the exp rows, (1 − θ_c²)/2 on the Φ diagonal, 1 elsewhere, so
    that grad(space 0, θ) = grad(space 1, θ_c) · chain_factor."""
    exp_rows, phi_rows, _ = SPACE_ROWS[kind]
    f = np.ones_like(Theta_c)
    for i in exp_rows:
        f[i] = Theta_c[i]
    for i in phi_rows:
        f[i] = (1.0 - Theta_c[i] ** 2) / 2.0
    return f


def bad_sigma(kind, th):
    th = th.copy()
    th[SPACE_ROWS[kind][2]] = -800.0  # σ² = e^-800 = 0: −Inf
    return th


def collinear(th):
    th = th.copy()
    th[0] = 5.0  # DNS, λ ≈ 148: slope and curvature loadings coincide, Z'Z singular to working precision
    return th
