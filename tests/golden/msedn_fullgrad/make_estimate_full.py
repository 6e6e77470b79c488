"""Writes estimate_full.npz: the reference run for tests/test_gpu_neural_lbfgs.py — estimate! (L-BFGS over all P
parameters, optimization.jl:329-410) of 1SD-NNS and NNS on N = 4, T = 40, windows of 40 and 24 columns, from θ₀
(synthetic.theta0_constrained).  The recipe is tests/golden/msed_fullgrad/make_estimate_full.py's.

The reference run is yfm_amd.lbfgs.minimize_batch with its defaults (what models.estimate_neural_lbfgs_batch runs) on
the Float64 restatement's compute_loss (tests/msedn_reference.py, −get_loss at the unconstrained θ) with
central-difference gradients, once at h = 1e-6 and once at h = 3e-6.  Stored per (kind, window): the start
(constrained), ll_start, ll_ref — the better of the two runs — and G = max(1e-6, 10 × |difference of the two runs'
ll|): the floor is the optimiser's own f_abstol, the 10× allows for chains that part ways by rounding.  The GPU chain
must reach ll ≥ ll_ref − G.  The runs' status and iteration counts are stored beside them.

    python tests/golden/msedn_fullgrad/make_estimate_full.py        # 208 s on 8 cores
"""
from __future__ import annotations

import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

FILE = HERE / "estimate_full.npz"
KINDS = (32, 16)  # 1SD-NNS, NNS
WINDOWS = (40, 24)
STEPS = (1e-6, 3e-6)
MATS = np.array([3.0, 12.0, 60.0, 120.0])
SEED = 7


def panel():
    from yfm_amd import synthetic as S
    return S.simulate_panel(32, 40, maturities=MATS, seed=SEED)


def reference_run(args):
    """(ll, status, iterations, ll_start) of one L-BFGS run on central differences of the restatement."""
    kind, w, h = args
    import msedn_reference as R
    from yfm_amd import lbfgs, synthetic as S
    from yfm_amd.params import untransform_params
    Y = panel()
    x0 = untransform_params(kind, S.theta0_constrained(kind))

    def f(x):
        return -R.get_loss(kind, MATS, Y, x, 0, R.FLOAT, w)

    def fun(X):
        fs, gs = [], []
        for c in range(X.shape[1]):
            x = X[:, c]
            g = np.empty_like(x)
            for j in range(x.size):
                up, dn = x.copy(), x.copy()
                up[j] += h
                dn[j] -= h
                g[j] = (f(up) - f(dn)) / (2 * h)
            fs.append(f(x))
            gs.append(g)
        return np.array(fs), np.stack(gs, axis=1)

    r = lbfgs.minimize_batch(fun, x0[:, None])
    return -float(r["f"][0]), int(r["status"][0]), int(r["iterations"][0]), -f(x0)


def build(processes=8):
    from yfm_amd import synthetic as S
    jobs = [(kind, w, h) for kind in KINDS for w in WINDOWS for h in STEPS]
    with Pool(processes) as pool:
        res = dict(zip(jobs, pool.map(reference_run, jobs, chunksize=1)))
    out = dict(Y=panel(), maturities=MATS, windows=np.array(WINDOWS), seed=SEED)
    for kind in KINDS:
        out[f"k{kind}_start_c"] = S.theta0_constrained(kind)
        for w in WINDOWS:
            a, b = res[(kind, w, STEPS[0])], res[(kind, w, STEPS[1])]
            pre = f"k{kind}_w{w}"
            out[f"{pre}_ll_ref"] = max(a[0], b[0])
            out[f"{pre}_G"] = max(1e-6, 10.0 * abs(a[0] - b[0]))
            out[f"{pre}_ll_start"] = a[3]
            out[f"{pre}_ll_runs"] = np.array([a[0], b[0]])
            out[f"{pre}_iterations"] = np.array([a[2], b[2]])
            out[f"{pre}_status"] = np.array([a[1], b[1]])
    return out


def load():
    with np.load(FILE) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    import time
    t0 = time.time()
    np.savez_compressed(FILE, **build())
    c = load()
    for k in sorted(c):
        if k[0] == "k" and not k.endswith("start_c"):
            print(k, c[k])
    print("seconds", time.time() - t0)
