"""Writes msedn_fullgrad_cases.npz: the truth for the neural models' full loss gradient (csrc/yfm_msedn_adj.hpp
loss_and_fullgrad, nns_sweep_kernel / nns_adjoint_kernel of csrc/yfm_msedn_adj.hip) — central differences of the
40-digit restatement (tests/msedn_reference.py, TRUTH) of get_loss with respect to the LEADING rows of θ (A, B, ω; γ for
the static kinds).  The last 12 rows are held by bits against the δ/Φ gradient, whose truth is
tests/golden/msedn_grad/.  The recipe is tests/golden/msedn_grad/make_msedn_grad.py's.

Per kind (make_msedn.REP_KINDS: NNS, NNS-Anchored, 1SD-NNS, 2RWSD-NNS, 3SSD-NNS, 3SRWSD-NNS-Anchored) the cases are
    plain panels      N ∈ {4, 5, 33} at T = 8 and N = 4 at T = 40
    Y[:, 0] = NaN     (4, 8): step 1 is prediction-only
    Y[:, 5] = NaN     (4, 8) with windows 5, 8, 8: the long windows compare column 6 and return −Inf
on make_msedn's panels and maturities, two candidates each (the window case has its three), space 0 everywhere and
space 1 on the N = 4, T = 8 case.

Screen (DESIGN.md §3.9's): candidates come from make_msedn's screened pool, in pool order, with A and B moved along
START_GRID; one is kept where the torch checker (tests/msedn_fullgrad_torch.py) gives a finite loss and gradient whose
largest A row and largest B row are at least 2e-6·‖g‖∞ — from the pool's own A (1e-5 … 1e-4) those rows are 1e-8 of
the largest — and whose gradient moves by less than 1e3 times a relative 1e-10 of θ (a recursion that A = 1e-2 has
made chaotic has gradients of 1e9 that no difference quotient resolves).  The script asserts on the stored differences
that, for every kind, each leading row is at least 1e-6·‖g_fd‖∞ in at least one kept candidate, so that no row goes
unchecked.

Per candidate and space: g_fd [P − 12] at h = 1e-12, e_fd = max|g(h = 1e-12) − g(h = 3e-12)|, the Float64
restatement's loss, and g_ad [P], the torch checker's gradient.  The script asserts max|g_ad − g_fd| ≤
1e-10·‖g_fd‖∞ + e_fd over the leading rows of every stored candidate — ten times inside the 1e-9 the tests allow the
code under test — and e_fd ≤ 1e-9·‖g_fd‖∞, and replaces a candidate that fails either by the next screened one (printed;
the scaled kinds fail where a score component is of the size of eps(Float64), so that Float64 and 40 digits scale it
differently).  A candidate whose loss is −Inf has NaN in g_fd.

    python tests/golden/msedn_fullgrad/make_msedn_fullgrad.py        # 131 s on 8 cores (one replacement round included)
"""
from __future__ import annotations

import math
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))
sys.path.insert(0, str(HERE.parent / "msedn"))
sys.path.insert(0, str(HERE.parent / "msedn_grad"))

FILE = HERE / "msedn_fullgrad_cases.npz"
H1, H2 = "1e-12", "3e-12"
NG = 12
SELF_REL = 1e-10
SCREEN = 1e-6
START_GRID = [(1e-2, 0.9), (1e-3, 0.97), (1e-2, 0.95)]
PERTURB, AMP_MAX = 1e-10, 1e3   # the conditioning screen: a chaotic recursion has no gradient worth the name

# (tag, N, T, variant, candidates, spaces)
CASES = [("n4t8", 4, 8, "plain", 2, (0, 1)), ("n5t8", 5, 8, "plain", 2, (0,)), ("n33t8", 33, 8, "plain", 2, (0,)),
         ("n4t40", 4, 40, "plain", 2, (0,)), ("n4t8nan0", 4, 8, "nan0", 2, (0,)), ("n4t8nan6", 4, 8, "nan6", 3, (0,))]


def kinds():
    import make_msedn as MN
    return MN.REP_KINDS


def case_panel(N, T, variant, nc):
    import make_msedn_grad as MG
    mats, Y, tu = MG.case_panel(N, T, variant)
    return mats, Y, np.asarray(tu[:nc] if variant != "nan6" else tu, dtype=np.int64)


def moved(kind, th, a, b):
    """th with every A at a and every B at b (unconstrained)."""
    import msedn_reference as R
    x = np.array(th, dtype=np.float64)
    nu = R.n_unique(kind)
    if nu:
        x[:nu] = math.log(a)
        if R.has_b(kind):
            x[nu:2 * nu] = math.log(b / (1 - b))
    return x


def choose(kind, mats, Y, T_use, spaces, taken):
    """The next screened candidate for one slot: (pool index, grid index, θ unconstrained)."""
    import make_msedn as MN
    import msedn_fullgrad_torch as TQ
    import msedn_reference as R
    from yfm_amd.params import transform_params
    pool = MN.theta_for(kind, 0)
    nu, hb = R.n_unique(kind), R.has_b(kind)
    minus_inf = np.isnan(Y[:, 1:T_use]).any()
    sign = np.where(np.arange(pool.shape[0]) % 2 == 0, 1.0, -1.0)
    for c in range(pool.shape[1]):
        for gi, (a, bb) in enumerate(START_GRID if nu else START_GRID[:1]):
            if (c, gi) in taken:
                continue
            x = moved(kind, pool[:, c], a, bb)
            ok = True
            for space in spaces:
                xs = x if space == 0 else transform_params(kind, x)
                loss, g = TQ.loss_and_grad(kind, mats, Y, xs, space, T_use)
                if minus_inf:
                    continue
                if not (np.isfinite(loss) and np.isfinite(g).all()):
                    ok = False
                    break
                top = np.max(np.abs(g))
                if nu and np.max(np.abs(g[:nu])) < 2 * SCREEN * top:
                    ok = False
                if hb and np.max(np.abs(g[nu:2 * nu])) < 2 * SCREEN * top:
                    ok = False
                # conditioning: θ moved by a relative PERTURB must move the gradient by less than AMP_MAX times that
                g2 = TQ.loss_and_grad(kind, mats, Y, xs * (1.0 + PERTURB * sign), space, T_use)[1]
                if not np.max(np.abs(g2 - g)) <= AMP_MAX * PERTURB * top:
                    ok = False
            if ok:
                taken.add((c, gi))
                return c, gi, x
    raise AssertionError(("no candidate left", kind))


def fd_job(args):
    """One leading row of one candidate in one space: (g at H1, g at H2); j = −1: whether the loss is finite."""
    kind, mats, Y, theta, space, T_use, j = args
    import mpmath as mp
    import make_msedn_grad as MG
    import msedn_reference as R
    with mp.workdps(R.TRUTH.digits):
        base = [mp.mpf(float(x)) for x in theta]
        if j < 0:
            return bool(mp.isfinite(MG.truth_loss(kind, mats, Y, base, space, T_use)))
        out = []
        for hs in (H1, H2):
            h = mp.mpf(hs)
            up, dn = list(base), list(base)
            up[j] = base[j] + h
            dn[j] = base[j] - h
            out.append(float((MG.truth_loss(kind, mats, Y, up, space, T_use) -
                              MG.truth_loss(kind, mats, Y, dn, space, T_use)) / (2 * h)))
        return tuple(out)


def fd_leading(pool, wanted):
    """wanted: [(kind, mats, Y, θ, space, T_use)] → [(g_fd[P − 12], e_fd)] over the leading rows."""
    finite = pool.map(fd_job, [w + (-1,) for w in wanted], chunksize=1)
    jobs = [(i, j) for i, (w, f) in enumerate(zip(wanted, finite)) if f for j in range(len(w[3]) - NG)]
    jobs.sort(key=lambda a: -wanted[a[0]][2].shape[0] * wanted[a[0]][5])  # the long ones first
    res = dict(zip(jobs, pool.map(fd_job, [wanted[i] + (j,) for i, j in jobs], chunksize=1)))
    out = []
    for i, (w, f) in enumerate(zip(wanted, finite)):
        nl = len(w[3]) - NG
        if not f:
            out.append((np.full(nl, np.nan), math.nan))
            continue
        g = np.array([res[(i, j)] for j in range(nl)])
        out.append((g[:, 0], float(np.max(np.abs(g[:, 0] - g[:, 1])))))
    return out


def build(processes=None):
    """Slots are filled, differenced and checked in rounds: a candidate whose differences have not converged to the
    tests' bar (e_fd > 1e-9·‖g_fd‖∞) or on which the torch checker misses SELF_REL is replaced by the next screened one
    (printed), so that the GPU bar is a statement about the kernel."""
    import msedn_fullgrad_torch as TQ
    import msedn_reference as R
    from yfm_amd.params import transform_params
    slots = {}   # (kind, tag, b) → dict(pick, per space: X, loss, gad, g_fd, e_fd)
    taken = {kind: set() for kind in kinds()}
    todo = [(kind, tag, b) for kind in kinds() for tag, N, T, variant, nc, spaces in CASES for b in range(nc)]
    case = {c[0]: c for c in CASES}
    worst = 0.0
    with Pool(processes) as pool:
        while todo:
            wanted, keys = [], []
            for kind, tag, b in todo:
                _, N, T, variant, nc, spaces = case[tag]
                mats, Y, tu = case_panel(N, T, variant, nc)
                pick = choose(kind, mats, Y, int(tu[b]), spaces, taken[kind])
                sl = slots[(kind, tag, b)] = dict(pick=pick)
                for space in spaces:
                    x = pick[2] if space == 0 else transform_params(kind, pick[2])
                    sl[space] = dict(X=x, loss=R.get_loss(kind, mats, Y, x, space, R.FLOAT, int(tu[b])),
                                     gad=TQ.loss_and_grad(kind, mats, Y, x, space, int(tu[b]))[1])
                    wanted.append((kind, mats, Y, x.copy(), space, int(tu[b])))
                    keys.append((kind, tag, b, space))
            res = fd_leading(pool, wanted)
            bad = set()
            for (kind, tag, b, space), (g, e) in zip(keys, res):
                sl = slots[(kind, tag, b)][space]
                sl["g_fd"], sl["e_fd"] = g, e
                if np.isnan(g).any():
                    assert np.isneginf(sl["loss"]), (kind, tag, b)
                    continue
                top = float(np.max(np.abs(g)))
                err = float(np.max(np.abs(sl["gad"][:len(g)] - g)))
                if not (e <= 1e-9 * top and err <= SELF_REL * top + e):
                    print(f"k{kind}_{tag} b={b} space {space}: replaced (err/top {err / top:.2e}, e_fd/top {e / top:.2e})",
                          flush=True)
                    bad.add((kind, tag, b))
            todo = sorted(bad)
    out, covered = {}, {}
    for kind in kinds():
        for tag, N, T, variant, nc, spaces in CASES:
            mats, Y, tu = case_panel(N, T, variant, nc)
            pre = f"k{kind}_{tag}"
            sl = [slots[(kind, tag, b)] for b in range(nc)]
            out[f"{pre}_maturities"], out[f"{pre}_Y"], out[f"{pre}_T_use"] = mats, Y, tu.astype(np.int32)
            out[f"{pre}_cand"] = np.array([s_["pick"][:2] for s_ in sl], dtype=np.int32)
            for space in spaces:
                out[f"{pre}_theta" + ("" if space == 0 else "_c")] = np.asfortranarray(
                    np.stack([s_[space]["X"] for s_ in sl], axis=1))
                out[f"{pre}_loss_s{space}"] = np.array([s_[space]["loss"] for s_ in sl])
                out[f"{pre}_g_ad_s{space}"] = np.stack([s_[space]["gad"] for s_ in sl], axis=1)
                out[f"{pre}_g_fd_s{space}"] = np.stack([s_[space]["g_fd"] for s_ in sl], axis=1)
                out[f"{pre}_e_fd_s{space}"] = np.array([s_[space]["e_fd"] for s_ in sl])
                for s_ in sl:
                    g = s_[space]["g_fd"]
                    if np.isnan(g).any():
                        continue
                    top = np.max(np.abs(g))
                    worst = max(worst, float(np.max(np.abs(s_[space]["gad"][:len(g)] - g)) / top))
                    cov = covered.setdefault(kind, np.zeros(len(g), dtype=bool))
                    cov |= np.abs(g) >= SCREEN * top
    out["worst_checker_rel"] = np.array(worst)
    return out, covered


def load_cases():
    with np.load(FILE) as z:
        return {k: z[k] for k in z.files}


def case_names():
    return [f"k{kind}_{tag}" for kind in kinds() for tag, *_ in CASES]


def case_spaces(name):
    tag = name.split("_", 1)[1]
    return next(c[5] for c in CASES if c[0] == tag)


if __name__ == "__main__":
    import time
    t0 = time.time()
    out, covered = build()
    np.savez_compressed(FILE, **out)
    print("worst max|g_ad - g_fd| / |g_fd|inf over the leading rows:", float(out["worst_checker_rel"]))
    print("seconds", time.time() - t0, "bytes", FILE.stat().st_size)
    for kind, cov in covered.items():
        assert cov.all(), ("a leading row is below the screen in every kept candidate", kind, np.where(~cov)[0])
