"""Writes msedn_fullgrad_long.npz: the neural models' full loss gradient at estimation length, T = 600 and N = 30,
space 0 — where the risk is the 600-fold product of step Jacobians the adjoint sweep carries backwards.

Kinds NNS, 1SD-NNS, 3SSD-NNS and 1SRWSD-NNS, two candidates each from make_msedn's screened pool (their own A,
1e-5 … 1e-4: the recursion stays stable over 600 steps), kept where the torch checker (tests/msedn_fullgrad_torch.py)
gives a finite loss and gradient that passes make_msedn_fullgrad's conditioning screen.  For 1SD-NNS additionally the
windows 300 and 600 over a missing column 450: the long window is −Inf with P NaNs.  Stored per case: the panel,
θ, T_use, the Float64 restatement's loss and g_ad [P], the torch checker's gradient over all P rows — an algorithm
independent of the hand-written adjoint, itself held to the 40-digit truth at T = 8 and 40 by make_msedn_fullgrad.py and
at T = 600 by the anchor below.

One 40-digit anchor: 1SD-NNS at T = 600, N = 5, one candidate, the 22 leading rows by central differences of the
40-digit restatement at h = 1e-12 and 3e-12 (g_fd, e_fd).  N = 5 because the risk at length does not depend on N and
the 40-digit filter's cost does.  The script asserts max|g_ad − g_fd| ≤ 1e-10·‖g_fd‖∞ + e_fd on it.

    python tests/golden/msedn_fullgrad/make_msedn_fullgrad_long.py        # 225 s on 8 cores, the anchor included
"""
from __future__ import annotations

import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_msedn_fullgrad as MF  # noqa: E402  (paths, fd_leading, the conditioning screen's constants)

FILE = HERE / "msedn_fullgrad_long.npz"
T, N = 600, 30
KINDS = (16, 32, 42, 44)   # NNS, 1SD-NNS, 3SSD-NNS, 1SRWSD-NNS
NC = 2
ANCHOR_KIND, ANCHOR_N = 32, 5


def stable(kind, mats, Y, x, T_use):
    """(loss, g) of the torch checker where the candidate passes the screen, else None."""
    import msedn_fullgrad_torch as TQ
    loss, g = TQ.loss_and_grad(kind, mats, Y, x, 0, T_use)
    if not (np.isfinite(loss) and np.isfinite(g).all()):
        return None
    sign = np.where(np.arange(len(x)) % 2 == 0, 1.0, -1.0)
    g2 = TQ.loss_and_grad(kind, mats, Y, x * (1.0 + MF.PERTURB * sign), 0, T_use)[1]
    if not np.max(np.abs(g2 - g)) <= MF.AMP_MAX * MF.PERTURB * np.max(np.abs(g)):
        return None
    return loss, g


def pick(kind, mats, Y, n, T_use=T):
    import make_msedn as MN
    pool = MN.theta_for(kind, 0)
    out = []
    for c in range(pool.shape[1]):
        r = stable(kind, mats, Y, pool[:, c], T_use)
        if r is not None:
            out.append((c, pool[:, c].copy(), r[1]))
            if len(out) == n:
                return out
    raise AssertionError(("no stable candidate", kind))


def build(processes=None):
    import make_msedn as MN
    import msedn_fullgrad_torch as TQ
    import msedn_reference as R
    out = {}
    mats = MN.mats_for(N)
    Y = np.array(MN.panel_for(N, T), dtype=np.float64, order="F")
    for kind in KINDS:
        got = pick(kind, mats, Y, NC)
        pre = f"k{kind}_n{N}t{T}"
        Th = np.asfortranarray(np.stack([g[1] for g in got], axis=1))
        out[f"{pre}_maturities"], out[f"{pre}_Y"], out[f"{pre}_T_use"] = mats, Y, np.full(NC, T, dtype=np.int32)
        out[f"{pre}_theta"], out[f"{pre}_cand"] = Th, np.array([g[0] for g in got], dtype=np.int32)
        out[f"{pre}_g_ad"] = np.stack([g[2] for g in got], axis=1)
        out[f"{pre}_loss"] = np.array([R.get_loss(kind, mats, Y, Th[:, b], 0, R.FLOAT, T) for b in range(NC)])
        print(pre, out[f"{pre}_loss"], flush=True)
    # 1SD-NNS over a missing column 450: window 300 is finite, window 600 compares the column
    kind = 32
    Yn = Y.copy(order="F")
    Yn[:, 450] = np.nan
    pre = f"k{kind}_n{N}t{T}nan450"
    Th = out[f"k{kind}_n{N}t{T}_theta"]
    tu = np.array([300, 600], dtype=np.int32)
    res = [TQ.loss_and_grad(kind, mats, Yn, Th[:, b], 0, int(tu[b])) for b in range(2)]
    assert np.isfinite(res[0][0]) and np.isneginf(res[1][0]) and np.isnan(res[1][1]).all()
    out[f"{pre}_maturities"], out[f"{pre}_Y"], out[f"{pre}_T_use"], out[f"{pre}_theta"] = mats, Yn, tu, Th
    out[f"{pre}_g_ad"] = np.stack([r[1] for r in res], axis=1)
    out[f"{pre}_loss"] = np.array([r[0] for r in res])
    # the 40-digit anchor
    kind = ANCHOR_KIND
    m5 = MN.mats_for(ANCHOR_N)
    Y5 = np.array(MN.panel_for(ANCHOR_N, T), dtype=np.float64, order="F")
    (c, x, gad), = pick(kind, m5, Y5, 1)
    with Pool(processes) as pool:
        (g_fd, e_fd), = MF.fd_leading(pool, [(kind, m5, Y5, x.copy(), 0, T)])
    pre = f"k{kind}_n{ANCHOR_N}t{T}"
    out[f"{pre}_maturities"], out[f"{pre}_Y"], out[f"{pre}_T_use"] = m5, Y5, np.array([T], dtype=np.int32)
    out[f"{pre}_theta"], out[f"{pre}_cand"] = np.asfortranarray(x[:, None]), np.array([c], dtype=np.int32)
    out[f"{pre}_g_ad"], out[f"{pre}_g_fd"], out[f"{pre}_e_fd"] = gad[:, None], g_fd[:, None], np.array([e_fd])
    out[f"{pre}_loss"] = np.array([R.get_loss(kind, m5, Y5, x, 0, R.FLOAT, T)])
    return out


def load_cases():
    with np.load(FILE) as z:
        return {k: z[k] for k in z.files}


def long_names():
    return [f"k{kind}_n{N}t{T}" for kind in KINDS] + [f"k32_n{N}t{T}nan450"]


def anchor_name():
    return f"k{ANCHOR_KIND}_n{ANCHOR_N}t{T}"


if __name__ == "__main__":
    import time
    t0 = time.time()
    out = build()
    np.savez_compressed(FILE, **out)
    a = anchor_name()
    g, e, gad = out[f"{a}_g_fd"][:, 0], float(out[f"{a}_e_fd"][0]), out[f"{a}_g_ad"][:len(out[f"{a}_g_fd"]), 0]
    top, err = np.max(np.abs(g)), np.max(np.abs(gad - g))
    print(f"anchor: |g_fd|inf {top:.3e}, e_fd {e:.3e}, max|g_ad - g_fd| {err:.3e} ({err / top:.2e} of |g_fd|inf)")
    print("seconds", time.time() - t0, "bytes", FILE.stat().st_size)
    assert err <= MF.SELF_REL * top + e
