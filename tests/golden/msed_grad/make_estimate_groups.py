"""Writes estimate_groups.npz: the reference run for tests/test_gpu_estimate_groups.py — SD-NS and NS on N = 4,
T = 40, windows of 40 and 24 columns, parameter group "2" (δ and Φ) alone.

With the leading parameters fixed the γ path, the loadings Z_t a step predicts with and the β_t it predicts from are
fixed (src/models/filter.jl:52-91), and the prediction μ + Φβ_t is linear in μ = (I − Φ)δ and Φ: the best loss over
the group is a linear least-squares problem, whose optimum L* (the sign of get_loss: −SSR/N/nobs) `optimum` computes
from the Float64 restatement's trajectory (tests/msed_reference.py).

The reference run is yfm_amd.lbfgs.minimize_batch with the options of opt2 (optimization.jl:453-462) on the Float64
NumPy value and gradient of that loss (`loss_and_grad`: the formulas of csrc/yfm_msed.hpp, which
tests/golden/msed_grad/make_msed_grad.py checks against the 40-digit restatement), from the start the estimation
uses: θ₀ after try_initializations.  Stored per (kind, window): the start (constrained), L*, the run's final ll and
G = max(1e-6, 10 × (L* − ll)) — the two runs may stop an iteration apart under f_abstol = 1e-6.

    python tests/golden/msed_grad/make_estimate_groups.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

FILE = HERE / "estimate_groups.npz"
KINDS = (4, 3)  # SD-NS, NS
WINDOWS = (40, 24)
MATS = np.array([3.0, 12.0, 60.0, 120.0])
NG = 12


def panel():
    from yfm_amd import synthetic as S
    return S.simulate_panel(4, 40, maturities=MATS, seed=7)


def trajectory(kind, Y, theta_c, nobs):
    """[(Z_t, β_t)] for the steps t = 1 … nobs − 1 of the Float64 restatement: the loadings step t predicts with
    and the β it predicts from.  Neither depends on δ or Φ, so the recursion is run with μ = 0, Φ = I, which leaves
    β_t in the state."""
    import msed_reference as R
    m = R.set_params(kind, theta_c, MATS, R.FLOAT)
    m.mu = np.zeros(3)
    m.Phi = np.eye(3)
    out = []
    for t in range(nobs - 1):
        assert not np.isnan(Y[0, t])
        R.filter_step(m, Y[:, t])
        out.append((m.Z.copy(), m.beta.copy()))
    return out


def optimum(traj, Y, nobs):
    """L* = max over (μ, Φ) of −Σ_t ‖y_{t+1} − Z_t(μ + Φβ_t)‖²/N/nobs."""
    N = Y.shape[0]
    A = np.vstack([np.hstack([Z, np.kron(b[None, :], Z)]) for Z, b in traj])  # μ, then vec Φ column-major
    y = np.concatenate([Y[:, t + 1] for t in range(nobs - 1)])
    u, *_ = np.linalg.lstsq(A, y, rcond=None)
    r = y - A @ u
    return -float(r @ r) / N / nobs


def loss_and_grad(kind, Y, x, nobs, traj):
    """compute_loss (= −get_loss) at the unconstrained θ = x and its gradient with respect to the last 12 rows."""
    from yfm_amd.params import transform_params
    N = Y.shape[0]
    tc = transform_params(kind, x)
    delta, Phi = tc[-12:-9], tc[-9:].reshape(3, 3, order="F")
    ssr, gd, gF = 0.0, np.zeros(3), np.zeros((3, 3))
    for t, (Z, b) in enumerate(traj):
        v = Y[:, t + 1] - Z @ (delta + Phi @ (b - delta))
        s = Z.T @ v
        ssr += v @ v
        gd += (np.eye(3) - Phi).T @ s
        gF += np.outer(s, b - delta)
    sc = -2.0 / N / nobs
    g = np.concatenate([sc * gd, (sc * gF).reshape(-1, order="F")])
    for d in (0, 4, 8):
        y = np.exp(x[-9 + d])
        g[3 + d] *= 2 * y / (1 + y) ** 2
    return ssr / N / nobs, g


def build():
    import msed_reference as R
    from yfm_amd import lbfgs, synthetic as S
    from yfm_amd.groups import LBFGS_OPTIONS
    from yfm_amd.params import untransform_params
    Y = panel()
    out = dict(Y=Y, maturities=MATS, windows=np.array(WINDOWS))
    for kind in KINDS:
        start = S.theta0_constrained(kind)
        for w in WINDOWS:
            sc = start if kind == 3 else R.try_initializations(kind, MATS, Y, start, T_use=w)[0]
            traj = trajectory(kind, Y, sc, w)
            Lstar = optimum(traj, Y, w)
            x0 = untransform_params(kind, sc)

            def fun(Xb):
                f, G = [], []
                for c in range(Xb.shape[1]):
                    x = x0.copy()
                    x[-NG:] = Xb[:, c]
                    fv, gv = loss_and_grad(kind, Y, x, w, traj)
                    f.append(fv)
                    G.append(gv)
                return np.array(f), np.stack(G, axis=1)

            r = lbfgs.minimize_batch(fun, x0[-NG:, None], **LBFGS_OPTIONS)
            ll = -float(r["f"][0])
            pre = f"k{kind}_w{w}"
            out[f"{pre}_start_c"] = sc
            out[f"{pre}_Lstar"] = Lstar
            out[f"{pre}_ll_ref"] = ll
            out[f"{pre}_ll_start"] = -float(fun(x0[-NG:, None])[0][0])
            out[f"{pre}_G"] = max(1e-6, 10.0 * (Lstar - ll))
            out[f"{pre}_iterations"] = int(r["iterations"][0])
    return out


def load():
    with np.load(FILE) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    np.savez_compressed(FILE, **build())
    c = load()
    for k in sorted(c):
        if k[0] == "k" and not k.endswith("start_c"):
            print(k, c[k])
