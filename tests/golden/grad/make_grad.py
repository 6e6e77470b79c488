"""Generator of tests/golden/grad/grad_cases.npz: reference gradients of the DNS log-likelihood that use no
derivative code — fourth-order central differences of the binary128 truth (oracle.truth.loglik_truth).

Per component i, g = (4·D(h) − D(2h))/3 with D the central quotient over the realised step, evaluated at
h = 1e-4 and at h = 3e-4; e_fd[b] = max_i |g_{1e-4} − g_{3e-4}| bounds the error of the h = 1e-4 value (the
truncation term falls 81× between the two).  A candidate is compared when every truth evaluation is finite
and e_fd ≤ 1e-9·‖g_fd‖∞ (`compared`).  All cases are in the unconstrained space.

Run from the repository root:  python tests/golden/grad/make_grad.py
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
from yfm_amd import KIND_DNS  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

H1, H2 = 1e-4, 3e-4
REL = 1e-9
CASE_NAMES = ("A", "A-windows", "A-nan", "B", "C", "D", "E")


def case_inputs(name: str):
    """(Y, maturities, Theta, T_use or None) of a case."""
    m30 = S.maturities_30()
    if name in ("A", "A-windows", "A-nan"):
        m = m30
        Y = S.simulate_panel(KIND_DNS, 40, m, 5)
        Th = S.theta_batch(KIND_DNS, 70, 0.1, 11, bad_frac=0)
        tu = None
        if name == "A-windows":
            tu = np.array([1, 2, 3, 17, 40] * 14, dtype=np.int32)
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
        Y = S.simulate_panel(KIND_DNS, 24, m, 6).copy()
        Y[1, 3] = np.nan
        return Y, m, S.theta_batch(KIND_DNS, 16, 0.1, 12, bad_frac=0), None
    if name == "C":
        m = np.concatenate([m30, [420.0, 480.0, 540.0]])
        return S.simulate_panel(KIND_DNS, 20, m, 7), m, S.theta_batch(KIND_DNS, 16, 0.1, 13, bad_frac=0), None
    if name == "D":
        m = np.linspace(3, 360, 64)
        return S.simulate_panel(KIND_DNS, 12, m, 8), m, S.theta_batch(KIND_DNS, 16, 0.1, 14, bad_frac=0), None
    if name == "E":
        m = m30[[0, 7, 15, 29]]
        return S.simulate_panel(KIND_DNS, 8, m, 9), m, S.theta_batch(KIND_DNS, 16, 0.1, 15, bad_frac=0), None
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
    f = TR.loglik_truth(KIND_DNS, Y, m, X, space=0, T_use=tux).reshape(2, P, 2, B)
    D = (f[:, :, 0, :] - f[:, :, 1, :]) / den
    return (4.0 * D[0] - D[1]) / 3.0, np.isfinite(f).all(axis=(0, 1, 2))


def make_case(name: str) -> dict:
    Y, m, Th, tu = case_inputs(name)
    with np.errstate(all="ignore"):
        g1, ok1 = fd_gradient(Y, m, Th, tu, H1)
        g2, ok2 = fd_gradient(Y, m, Th, tu, H2)
        e_fd = np.abs(g1 - g2).max(axis=0)
        truth = TR.loglik_truth(KIND_DNS, Y, m, Th, space=0, T_use=tu)
        oracle = TR.loglik_oracle(KIND_DNS, Y, m, Th, space=0, T_use=tu)
        compared = ok1 & ok2 & np.isfinite(truth) & (e_fd <= REL * np.abs(g1).max(axis=0))
    B = Th.shape[1]
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Th,
                T_use=np.full(B, Y.shape[1], dtype=np.int32) if tu is None else tu,
                g_fd=g1, e_fd=e_fd, compared=compared, loglik_oracle=oracle, loglik_truth=truth)


def load_cases(path=HERE / "grad_cases.npz") -> dict:
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
        c = make_case(name)
        print(f"{name}: compared {int(c['compared'].sum())}/{c['compared'].size}")
        for k, v in c.items():
            flat[f"{name}/{k}"] = v
    np.savez_compressed(HERE / "grad_cases.npz", **flat)


if __name__ == "__main__":
    main()
