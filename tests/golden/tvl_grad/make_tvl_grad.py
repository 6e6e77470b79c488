"""Generator of tests/golden/tvl_grad/tvl_grad_cases.npz: reference gradients of the TVλ log-likelihood that use
no derivative code — fourth-order central differences of the binary128 truth (oracle.truth.loglik_truth), as
tests/golden/grad/make_grad.py makes them for DNS, with one difference: a ladder of steps.

Per component i and step h, g_h = (4·D(h) − D(2h))/3 with D the central quotient over the realised step.  The DNS
steps (1e-4 / 3e-4) do not converge on the EKF (median e_fd/‖g‖∞ ≈ 5e-3), so for every h of LADDER
e(h) = max_i |g_h − g_{3h}| is formed, and per candidate the h with the smallest e(h)/‖g_h‖∞ is kept:
g_fd = g_h, e_fd = e(h), h_used = h.  A candidate is `compared` when every truth evaluation is finite,
e_fd ≤ 1e-9·‖g_fd‖∞ and |oracle − truth| ≤ ORACLE_REL·max(1, |truth|) (the dense FP64 recursion itself is inside
the project's bar there; this condition reads the reference only).  All cases are in the unconstrained space.

Run from the repository root:  python tests/golden/tvl_grad/make_tvl_grad.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
for p in (str(ROOT / "yieldfactormodels.jl_amd"), str(ROOT)):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import truth as TR  # noqa: E402
from yfm_amd import KIND_TVL  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

LADDER = (3e-6, 1e-6, 3e-7, 1e-7)
REL = 1e-9
ORACLE_REL = 1e-9
CASE_NAMES = ("A", "A-windows", "A-nan", "B", "C", "D")


def case_inputs(name: str):
    """(Y, maturities, Theta, T_use or None) of a case."""
    m30 = S.maturities_30()
    if name in ("A", "A-windows", "A-nan"):
        m = m30
        Y = S.simulate_panel(KIND_TVL, 40, m, 5)
        Th = S.theta_batch(KIND_TVL, 24, 0.02, 11, bad_frac=0)
        tu = None
        if name == "A-windows":
            tu = np.array(([1, 2, 3, 17, 40] * 5)[:24], dtype=np.int32)
        if name == "A-nan":
            Th = Th[:, :16]
            Y = Y.copy()
            Y[2, 5] = np.nan
            Y[:, 6] = np.nan
            Y[0, 20] = np.nan
            Y[1, 39] = np.nan
        return Y, m, Th, tu
    if name == "B":
        m = m30[::3]
        return S.simulate_panel(KIND_TVL, 24, m, 5), m, S.theta_batch(KIND_TVL, 16, 0.02, 12, bad_frac=0), None
    if name == "C":
        m = m30[:7]
        return S.simulate_panel(KIND_TVL, 12, m, 5), m, S.theta_batch(KIND_TVL, 16, 0.02, 13, bad_frac=0), None
    if name == "D":
        m = np.linspace(3, 360, 67)
        return S.simulate_panel(KIND_TVL, 16, m, 5), m, S.theta_batch(KIND_TVL, 16, 0.02, 14, bad_frac=0), None
    raise KeyError(name)


def fd_gradient(Y, m, Th, tu, h):
    """(g[P, B], finite[B]): the fourth-order difference gradient of the truth at step h."""
    P, B = Th.shape
    pts, den = [], np.empty((2, P, B))
    for k, mult in enumerate((1.0, 2.0)):
        for i in range(P):
            up, dn = Th.copy(), Th.copy()
            up[i] += mult * h
            dn[i] -= mult * h
            den[k, i] = up[i] - dn[i]
            pts += [up, dn]
    X = np.concatenate(pts, axis=1)
    tux = None if tu is None else np.tile(tu, len(pts))
    f = TR.loglik_truth(KIND_TVL, Y, m, X, space=0, T_use=tux).reshape(2, P, 2, B)
    D = (f[:, :, 0, :] - f[:, :, 1, :]) / den
    return (4.0 * D[0] - D[1]) / 3.0, np.isfinite(f).all(axis=(0, 1, 2))


def make_case(name: str) -> dict:
    Y, m, Th, tu = case_inputs(name)
    B = Th.shape[1]
    with np.errstate(all="ignore"):
        steps = sorted({h for h0 in LADDER for h in (h0, 3.0 * h0)})
        gs = {h: fd_gradient(Y, m, Th, tu, h) for h in steps}
        g_fd = np.zeros_like(Th)
        e_fd = np.full(B, np.inf)
        h_used = np.zeros(B)
        ratio = np.full(B, np.inf)
        ok = np.ones(B, dtype=bool)
        for h in steps:
            ok &= gs[h][1]
        for h in LADDER:
            g1, g3 = gs[h][0], gs[3.0 * h][0]
            e = np.abs(g1 - g3).max(axis=0)
            gn = np.abs(g1).max(axis=0)
            r = np.where(gn > 0, e / np.where(gn > 0, gn, 1.0), np.where(e == 0, 0.0, np.inf))
            r = np.where(np.isfinite(r), r, np.inf)
            # a window with no accumulated term: every difference is exactly zero at every step
            better = (r < ratio) | ((h_used == 0) & (r <= ratio))
            g_fd[:, better] = g1[:, better]
            e_fd[better] = e[better]
            h_used[better] = h
            ratio[better] = r[better]
        truth = TR.loglik_truth(KIND_TVL, Y, m, Th, space=0, T_use=tu)
        oracle = TR.loglik_oracle(KIND_TVL, Y, m, Th, space=0, T_use=tu)
        fd_ok = ok & np.isfinite(truth) & np.isfinite(e_fd) & (e_fd <= REL * np.abs(g_fd).max(axis=0))
        oracle_err = np.abs(oracle - truth) / np.maximum(1.0, np.abs(truth))
        compared = fd_ok & (oracle_err <= ORACLE_REL)
    print(f"{name}: finite-and-e_fd {int(fd_ok.sum())}/{B}, compared {int(compared.sum())}/{B}, "
          f"worst |oracle − truth| {np.nanmax(oracle_err):.2e}")
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Th,
                T_use=np.full(B, Y.shape[1], dtype=np.int32) if tu is None else tu,
                g_fd=g_fd, e_fd=e_fd, h_used=h_used, compared=compared, loglik_oracle=oracle, loglik_truth=truth)


def load_cases(path=HERE / "tvl_grad_cases.npz") -> dict:
    """{case name: {field: array}} of the committed file."""
    out: dict = {}
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            name, field = k.split("/", 1)
            out.setdefault(name, {})[field] = z[k]
    return out


def main():
    flat = {}
    for name in CASE_NAMES:
        for k, v in make_case(name).items():
            flat[f"{name}/{k}"] = v
    np.savez_compressed(HERE / "tvl_grad_cases.npz", **flat)


if __name__ == "__main__":
    main()
