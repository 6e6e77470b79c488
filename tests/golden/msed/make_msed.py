"""Writes msed_cases.npz: one full filter per λ-model kind on N = 4, T = 8 — the panel, the maturities, a
constrained and an unconstrained θ per kind and get_loss of each from the Float64 restatement
(tests/msed_reference.py) — for the host build of csrc/yfm_msed.hpp (tests/test_msed_host_cpu.py).

    python tests/golden/msed/make_msed.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

FILE = HERE / "msed_cases.npz"


def build():
    import msed_reference as R
    from yfm_amd import synthetic as S
    from yfm_amd.params import transform_params

    mats = np.array([3.0, 12.0, 60.0, 120.0])
    Y = S.simulate_panel(R.KIND_SD_NS, 8, maturities=mats, seed=7)
    Y[0, 5] = np.nan  # one prediction-only step (the window of the first candidate stops before its comparison)
    out = dict(maturities=mats, Y=Y)
    for kind in R.KINDS:
        Th = S.theta_batch(kind, 3, scale=0.1, seed=11 + kind, bad_frac=0.0)
        Tc = np.stack([transform_params(kind, Th[:, b]) for b in range(3)], axis=1)
        tu = np.array([5, 8, 8])
        Yk = Y.copy()
        out[f"theta_{kind}"] = Th
        out[f"theta_c_{kind}"] = Tc
        out[f"T_use_{kind}"] = tu
        out[f"loss_{kind}"] = np.array([R.get_loss(kind, mats, Yk, Th[:, b], 0, R.FLOAT, int(tu[b])) for b in range(3)])
        out[f"loss_c_{kind}"] = np.array([R.get_loss(kind, mats, Yk, Tc[:, b], 1, R.FLOAT, int(tu[b])) for b in range(3)])
        # the same without the missing entry: three finite values per kind
        Yc = S.simulate_panel(R.KIND_SD_NS, 8, maturities=mats, seed=7)
        out[f"loss_full_{kind}"] = np.array([R.get_loss(kind, mats, Yc, Th[:, b], 0, R.FLOAT) for b in range(3)])
    return out


def load_cases():
    with np.load(FILE) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    np.savez(FILE, **build())
    c = load_cases()
    for k in sorted(c):
        if k.startswith("loss"):
            print(k, c[k])
