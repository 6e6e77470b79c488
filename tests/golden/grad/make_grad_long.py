"""Generator of tests/golden/grad/grad_long_cases.npz: reference gradients of the DNS log-likelihood at estimation
length (T up to 600), made as tests/golden/grad/make_grad.py makes the short ones — fourth-order central differences of
the binary128 truth (make_grad.fd_gradient) — with one addition, the step ladder of
tests/golden/tvl_grad/make_tvl_grad.py: per candidate the better of the step pairs (1e-4, 3e-4) and (3e-5, 9e-5) is
kept (the smaller e(h)/‖g_h‖∞, e(h) = max_i |g_h − g_{3h}|): g_fd = g_h, e_fd = e(h), h_used = h.  A candidate is
`compared` when every truth evaluation is finite and e_fd ≤ 1e-9·‖g_fd‖∞.  All cases are in the unconstrained space.

Cases
    L          the bench panel (T = 600, N = 30) with the first 48 columns of the bench batch
    L-windows  the same panel with column 450 all NaN and one NaN entry in each of columns 598 and 599, 16 columns,
               T_use cycling through (200, 333, 599, 600): the stale term and the unused last column, late
    L-hard     the same panel with bench columns 10283, 1679, 5390, 22413, 0, 1 (tests/golden/dns_hard_T600.npz)
    L-n64      64 maturities, T = 200, 8 candidates
    L-band     T = 120, N = 30, θ₀ with γ moved through GAMMAS towards collinear loadings; `kappa1` is NumPy's
               κ₁(Z'Z) per candidate (the library defers a candidate at κ₁ ≥ 1e6)

Beside make_grad.py's fields:
    h_used     the kept step
    hard[b]    |oracle − truth| > 1e-9·max(1, |truth|) for the loglik: the dense FP64 recursion is itself outside the
               project's bar there (this reads the reference only)
    ref_err[b] for a hard candidate, the error of a plain FP64 gradient of the same operation: central differences of
               the dense FP64 oracle at h ∈ REF_STEPS, the best step per candidate, max_i |g − g_fd|; NaN elsewhere

Run from the repository root:  python tests/golden/grad/make_grad_long.py      # minutes; it prints its own time
"""
from __future__ import annotations

import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_grad as MG  # noqa: E402  (fd_gradient; it puts the repository on sys.path)
from oracle import truth as TR  # noqa: E402
from yfm_amd import KIND_DNS  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "grad_long_cases.npz"
LADDER = (1e-4, 3e-5)
REL = 1e-9
ORACLE_REL = 1e-9
REF_STEPS = (1e-3, 1e-4, 1e-5, 1e-6, 1e-7)
CASE_NAMES = ("L", "L-windows", "L-hard", "L-n64", "L-band")
HARD_COLUMNS = (10283, 1679, 5390, 22413, 0, 1)
WINDOWS = (200, 333, 599, 600)
GAMMAS = (0.0, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6)


def case_inputs(name: str):
    """(Y, maturities, Theta, T_use or None) of a case."""
    m30 = S.maturities_30()
    if name in ("L", "L-windows", "L-hard"):
        Y = S.simulate_panel(KIND_DNS, 600)
        bench = S.theta_batch(KIND_DNS, 65536)
        if name == "L":
            return Y, m30, np.asfortranarray(bench[:, :48]), None
        if name == "L-hard":
            return Y, m30, np.asfortranarray(bench[:, list(HARD_COLUMNS)]), None
        Y = Y.copy(order="F")
        Y[:, 450] = np.nan
        Y[3, 598] = np.nan
        Y[7, 599] = np.nan
        return Y, m30, np.asfortranarray(bench[:, :16]), np.array(WINDOWS * 4, dtype=np.int32)
    if name == "L-n64":
        m = np.linspace(3, 360, 64)
        return S.simulate_panel(KIND_DNS, 200, m, 8), m, S.theta_batch(KIND_DNS, 8, 0.1, 14, bad_frac=0), None
    if name == "L-band":
        Th = np.asfortranarray(np.repeat(S.theta0(KIND_DNS)[:, None], len(GAMMAS), axis=1))
        Th[0] = GAMMAS
        return S.simulate_panel(KIND_DNS, 120), m30, Th, None
    raise KeyError(name)


def kappa1(gamma: float, m) -> float:
    """NumPy's 1-norm condition number of Z'Z at λ = 0.01 + e^γ."""
    Z = S._loadings([gamma], np.asarray(m, dtype=np.float64), 3)
    return float(np.linalg.cond(Z.T @ Z, 1))


def oracle_difference_error(Y, m, th, tu, g_fd):
    """min over REF_STEPS of max_i |g_h − g_fd|, g_h the plain central differences of the dense FP64 oracle."""
    P = th.size
    best = np.inf
    for h in REF_STEPS:
        X = np.repeat(th[:, None], 2 * P, axis=1)
        for i in range(P):
            X[i, 2 * i] += h
            X[i, 2 * i + 1] -= h
        den = X[np.arange(P), 2 * np.arange(P)] - X[np.arange(P), 2 * np.arange(P) + 1]
        f = TR.loglik_oracle(KIND_DNS, Y, m, X, space=0, T_use=None if tu is None else np.full(2 * P, tu, np.int32))
        g = (f[0::2] - f[1::2]) / den
        e = np.abs(g - g_fd).max()
        if np.isfinite(e):
            best = min(best, float(e))
    return best


def make_case(name: str) -> dict:
    Y, m, Th, tu = case_inputs(name)
    B = Th.shape[1]
    t0 = time.time()
    with np.errstate(all="ignore"):
        g_fd = np.zeros_like(Th)
        e_fd = np.full(B, np.inf)
        h_used = np.zeros(B)
        ratio = np.full(B, np.inf)
        ok = np.ones(B, dtype=bool)
        for h in LADDER:
            g1, ok1 = MG.fd_gradient(Y, m, Th, tu, h)
            g3, ok3 = MG.fd_gradient(Y, m, Th, tu, 3.0 * h)
            ok &= ok1 & ok3
            e = np.abs(g1 - g3).max(axis=0)
            gn = np.abs(g1).max(axis=0)
            r = np.where(gn > 0, e / np.where(gn > 0, gn, 1.0), np.where(e == 0, 0.0, np.inf))
            r = np.where(np.isfinite(r), r, np.inf)
            better = (r < ratio) | ((h_used == 0) & (r <= ratio))
            g_fd[:, better] = g1[:, better]
            e_fd[better] = e[better]
            h_used[better] = h
            ratio[better] = r[better]
        truth = TR.loglik_truth(KIND_DNS, Y, m, Th, space=0, T_use=tu)
        oracle = TR.loglik_oracle(KIND_DNS, Y, m, Th, space=0, T_use=tu)
        compared = ok & np.isfinite(truth) & np.isfinite(e_fd) & (e_fd <= REL * np.abs(g_fd).max(axis=0))
        oracle_err = np.abs(oracle - truth) / np.maximum(1.0, np.abs(truth))
        hard = np.isfinite(truth) & ~(oracle_err <= ORACLE_REL)
        ref_err = np.full(B, np.nan)
        for b in np.flatnonzero(hard):
            ref_err[b] = oracle_difference_error(Y, m, Th[:, b], None if tu is None else int(tu[b]), g_fd[:, b])
    print(f"{name}: compared {int(compared.sum())}/{B}, hard {np.flatnonzero(hard).tolist()}, "
          f"worst e_fd/|g| over the compared {np.max(ratio[compared]):.2e}, {time.time() - t0:.0f} s")
    out = dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Th,
               T_use=np.full(B, Y.shape[1], dtype=np.int32) if tu is None else tu,
               g_fd=g_fd, e_fd=e_fd, h_used=h_used, compared=compared, hard=hard, ref_err=ref_err,
               loglik_oracle=oracle, loglik_truth=truth)
    if name == "L-band":
        out["kappa1"] = np.array([kappa1(g, m) for g in GAMMAS])
    return out


def load_cases(path=FILE) -> dict:
    """{case name: {field: array}} of the committed file.  The bench panel is stored once, under L: L-hard shares it
    and L-windows is that panel with NaN at its stored `nan_index` (row, column) pairs."""
    out: dict = {}
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            name, field = k.split("/", 1)
            out.setdefault(name, {})[field] = z[k]
    out["L-hard"]["Y"] = out["L"]["Y"]
    out["L-hard"]["maturities"] = out["L-windows"]["maturities"] = out["L"]["maturities"]
    Yw = out["L"]["Y"].copy(order="F")
    idx = out["L-windows"].pop("nan_index")
    Yw[idx[:, 0], idx[:, 1]] = np.nan
    out["L-windows"]["Y"] = Yw
    return {name: out[name] for name in CASE_NAMES}


def main():
    t0 = time.time()
    flat = {}
    for name in CASE_NAMES:
        c = make_case(name)
        if name == "L-windows":  # the panel of L with these entries missing
            c["nan_index"] = np.argwhere(np.isnan(c["Y"]))
        if name in ("L-hard", "L-windows"):  # the panel of L
            del c["Y"], c["maturities"]
        for k, v in c.items():
            flat[f"{name}/{k}"] = v
    np.savez_compressed(FILE, **flat)
    print(f"generated in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
