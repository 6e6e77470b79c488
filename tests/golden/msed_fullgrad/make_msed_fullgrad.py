"""Writes msed_fullgrad_cases.npz: the truth for the λ models' full loss gradient (csrc/yfm_msed.hpp
get_loss_fullgrad, lambda_fullgrad_kernel of csrc/yfm_msed.hip) — central differences of the 40-digit restatement
(tests/msed_reference.py, TRUTH) of get_loss with respect to every row of θ, in both parameter spaces.  The recipe
is tests/golden/msed_grad/make_msed_grad.py's over all P rows.

Per kind (NS, SD-NS, RWSD-NS, SSD-NS, SRWSD-NS) the cases are
    plain panels      (N, T) ∈ {1, 4, 5, 30, 33} × {8}  and  {4, 33} × {40}      (N = 1 takes the ridge branch)
    Y[0, 0] = NaN     (4, 8), (30, 8): step 1 is prediction-only
    Y[0, 5] = NaN     (4, 8) with windows 5, 8, 8: the long windows compare column 6 and return −Inf
each with 3 candidates θ₀ + 0.1·N(0, I).  N = 3 is left out, as before.

Screen: a candidate is kept only if, in both spaces, every leading row (A, B, ω; γ for NS) of its gradient is at
least 1e-6·‖g‖∞, so that the tests' 1e-9·‖g_fd‖∞ resolves three digits of every row; a candidate that fails is
replaced by the same column of the next seed's batch, with A and B moved along START_GRID (below).  The screen picks
with the Float64 formulas below (fast) and is asserted on the stored differences.

`analytic` evaluates the formulas of DESIGN.md §3.9 in NumPy on the Float64 restatement's trajectory; the script
prints the worst max|g − g_fd| / ‖g_fd‖∞ over every stored candidate.

Per candidate and space: g_fd [P] at h = 1e-12, e_fd = max|g(h = 1e-12) − g(h = 3e-12)| and the Float64
restatement's loss.  A candidate whose loss is −Inf has NaN in g_fd.

    python tests/golden/msed_fullgrad/make_msed_fullgrad.py        # minutes, with its worker processes
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
sys.path.insert(0, str(HERE.parent / "msed_grad"))

import make_msed_grad as MG  # noqa: E402  (maturities, truth_loss)

FILE = HERE / "msed_fullgrad_cases.npz"
KINDS = (3, 4, 5, 6, 8)
H1, H2 = "1e-12", "3e-12"
SCREEN = 1e-6
# θ₀ + 0.1·N(0, I) keeps A near 1e-3 and B near 0.98, where SD-NS at T = 8 never passes the screen (row B is 1e-8 of
# the largest row): a replacement also moves A and B along the reference's own start grid (mselambda.jl:26-27)
START_GRID = [(a, b) for a in (1e-3, 1e-2, 1e-1) for b in (0.98, 0.95, 0.9)]

# (tag, N, T, variant)
CASES = [(f"n{N}t8", N, 8, "plain") for N in (1, 4, 5, 30, 33)] + [(f"n{N}t40", N, 40, "plain") for N in (4, 33)] + \
        [(f"n{N}t8nan0", N, 8, "nan0") for N in (4, 30)] + [("n4t8nan6", 4, 8, "nan6")]


def maturities(N):
    if N == 5:
        return np.array([3.0, 12.0, 36.0, 60.0, 120.0])
    return MG.maturities(N)


def n_lead(kind):
    return 1 if kind == 3 else (3 if kind in (4, 6) else 2)


def panel(kind, N, T, variant):
    from yfm_amd import synthetic as S
    mats = maturities(N)
    Y = S.simulate_panel(kind, T, maturities=mats, seed=7)
    tu = np.array([T, T, T])
    if variant == "nan0":
        Y[0, 0] = np.nan
    elif variant == "nan6":
        Y[0, 5] = np.nan
        tu = np.array([5, 8, 8])
    return mats, Y, tu


# ---- the formulas of DESIGN.md §3.9 in Float64 NumPy ----------------------------------------------------------
def _loadings(gamma, m):
    """Z, D = ∂Z/∂γ, E = ∂²Z/∂γ² (N×3 each)."""
    q = math.exp(gamma)
    lam = 0.01 + q
    z = np.exp(-lam * m)
    Z2 = (1 - z) / (lam * m)
    u = (z - Z2) / lam
    du = (-m * z - 2 * u) / lam
    one, nul = np.ones_like(m), np.zeros_like(m)
    Z = np.stack([one, Z2, Z2 - z], axis=1)
    D = np.stack([nul, u * q, (u + m * z) * q], axis=1)
    E = np.stack([nul, du * q * q + u * q, (du - m * m * z) * q * q + (u + m * z) * q], axis=1)
    return Z, D, E


def _ols(Z, y):
    """(G as solved with — ridged where the plain Cholesky fails —, β)."""
    G = Z.T @ Z
    try:
        np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        G = G + 1e-3 * np.eye(3)
        np.linalg.cholesky(G)
    return G, np.linalg.solve(G, Z.T @ y)


def analytic(kind, mats, Y, theta, space, nobs):
    """(get_loss, its gradient [P] in the caller's space) from the tangent recursion."""
    import msed_reference as R
    static, hasb, scaled = R.is_static(kind), R.has_b(kind), R.scaled(kind)
    tc = R.transform_params(kind, theta) if space == 0 else np.asarray(theta, dtype=np.float64)
    P, K, N = len(tc), n_lead(kind), Y.shape[0]
    A = 0.0 if static else tc[0]
    B = tc[1] if hasb else 0.0
    om = tc[K - 1]
    delta, Phi = tc[K:K + 3], tc[K + 3:].reshape(3, 3, order="F")
    mu = (np.eye(3) - Phi) @ delta
    nu = (1 - B) * om if hasb else 0.0
    # constrained directions: (A, B, ω) / (A, ω) / (γ)
    Ad = np.zeros(K)
    Bd = np.zeros(K)
    nud = np.zeros(K)
    gd = np.zeros(K)
    gd[K - 1] = 1.0
    if not static:
        Ad[0] = 1.0
    if hasb:
        Bd[1] = 1.0
        nud[1], nud[2] = -om, 1 - B
    gamma, beta = om, delta.copy()
    ewma, ed, count = 0.0, np.zeros(K), 0
    lead, gF, gdl = np.zeros(K), np.zeros((3, 3)), np.zeros(3)
    mse = 0.0
    for t in range(nobs - 1):
        y = Y[:, t]
        if np.isnan(y[0]):
            if hasb:
                gd = nud + Bd * gamma + B * gd
                gamma = nu + B * gamma
            gplus, pb, bpost = np.zeros(K), np.zeros(3), None
        else:
            Z, D, E = _loadings(gamma, mats)
            G, beta = _ols(Z, y)
            v = y - Z @ beta
            w = D @ beta
            bp = np.linalg.solve(G, D.T @ v - Z.T @ w)
            if not static:
                g = 2 * (v @ w)
                gp = 2 * (-(w + Z @ bp) @ w + v @ (E @ beta) + v @ (D @ bp))
                gk = gp * gd
                if scaled:
                    f = R.FORGET
                    ewma = f * ewma + (1 - f) * g * g
                    ed = f * ed + 2 * (1 - f) * g * gk
                    count += 1
                    c = 1 - f ** count
                    r = math.sqrt(ewma / c)
                    s = r + R.FLOAT.eps
                    sd = ed / (2 * c * r)
                    gk = gk / s - g * sd / (s * s)
                    g = g / s
                gd = gd + Ad * g + A * gk
                gamma = gamma + A * g
                Z, D, E = _loadings(gamma, mats)
                G, beta = _ols(Z, y)
                v = y - Z @ beta
                bp = np.linalg.solve(G, D.T @ v - Z.T @ (D @ beta))
            gplus, pb, bpost = gd.copy(), Phi @ bp, beta.copy()
            if hasb:
                gd = nud + Bd * gamma + B * gd
                gamma = nu + B * gamma
        beta = mu + Phi @ beta
        Z, D, E = _loadings(gamma, mats)
        vn = Y[:, t + 1] - Z @ beta
        mse -= vn @ vn
        if not np.isfinite(mse):
            return -math.inf, np.full(P, np.nan)
        s = Z.T @ vn
        lead += 2 * (vn @ (D @ beta)) * gd + 2 * (s @ pb) * gplus
        if bpost is None:
            gdl += 2 * s
        else:
            gdl += 2 * (np.eye(3) - Phi).T @ s
            gF += 2 * np.outer(s, bpost - delta)
    g = np.concatenate([lead, gdl, gF.reshape(-1, order="F")]) / N / nobs
    if space == 0:
        if not static:
            g[0] *= A
        if hasb:
            g[1] *= B * (1 - B)
        for d in (0, 4, 8):
            yy = math.exp(theta[K + 3 + d])
            g[K + 3 + d] *= 2 * yy / (1 + yy) ** 2
    return mse / N / nobs, g


def screened(kind, mats, Y, tu, th, tc, minus_inf):
    """True where the leading rows of the Float64 gradient pass the screen in both spaces.  minus_inf: the window
    compares the missing column, the loss is −Inf whatever θ is and there is nothing to screen."""
    K = n_lead(kind)
    for space, x in ((0, th), (1, tc)):
        loss, g = analytic(kind, mats, Y, x, space, tu)
        if minus_inf:
            continue
        if not np.isfinite(loss):
            return False
        if not np.all(np.abs(g[:K]) >= 2 * SCREEN * np.max(np.abs(g))):  # 2×: margin for the stored differences
            return False
    return True


def case_inputs(kind, tag, N, T, variant):
    """(maturities, Y, Θ unconstrained P×3, T_use[3]) with the screened candidates."""
    from yfm_amd import synthetic as S
    from yfm_amd.params import transform_params
    mats, Y, tu = panel(kind, N, T, variant)
    Th = S.theta_batch(kind, 3, scale=0.1, seed=11 + kind, bad_frac=0.0)
    for b in range(3):
        seed, r = 11 + kind, 0
        minus_inf = variant == "nan6" and tu[b] > 6
        while not screened(kind, mats, Y, int(tu[b]), Th[:, b], transform_params(kind, Th[:, b]), minus_inf):
            seed, r = seed + 100, r + 1
            assert r < 200, (kind, tag, b)
            Th[:, b] = S.theta_batch(kind, 3, scale=0.1, seed=seed, bad_frac=0.0)[:, b]
            if kind != 3:  # the start grid for A and B, mildest first, under the same 0.1·N(0, 1)
                a, bb = START_GRID[(r - 1) % len(START_GRID)]
                Th[0, b] += math.log(a / 1e-3)
                if kind in (4, 6):
                    Th[1, b] += math.log(bb / (1 - bb)) - math.log(0.98 / 0.02)
    return mats, Y, Th, tu


def fd_gradient(args):
    """One candidate in one space: (g at H1 [P], e_fd)."""
    kind, mats, Y, theta, space, T_use = args
    import mpmath as mp
    import msed_reference as R
    P = len(theta)
    with mp.workdps(R.MP_DIGITS):
        base = [mp.mpf(float(x)) for x in theta]
        if not mp.isfinite(MG.truth_loss(kind, mats, Y, base, space, T_use)):
            return np.full(P, np.nan), math.nan
        g = np.empty((2, P))
        for k, hs in enumerate((H1, H2)):
            h = mp.mpf(hs)
            for j in range(P):
                up, dn = list(base), list(base)
                up[j] = base[j] + h
                dn[j] = base[j] - h
                g[k, j] = float((MG.truth_loss(kind, mats, Y, up, space, T_use) -
                                 MG.truth_loss(kind, mats, Y, dn, space, T_use)) / (2 * h))
        return g[0], float(np.max(np.abs(g[0] - g[1])))


def build(processes=8):
    import msed_reference as R
    from yfm_amd.params import transform_params
    out, jobs, keys = {}, [], []
    for kind in KINDS:
        for tag, N, T, variant in CASES:
            mats, Y, Th, tu = case_inputs(kind, tag, N, T, variant)
            Tc = np.stack([transform_params(kind, Th[:, b]) for b in range(3)], axis=1)
            pre = f"k{kind}_{tag}"
            out[f"{pre}_maturities"], out[f"{pre}_Y"], out[f"{pre}_T_use"] = mats, Y, tu
            out[f"{pre}_theta"], out[f"{pre}_theta_c"] = Th, Tc
            for space, X in ((0, Th), (1, Tc)):
                out[f"{pre}_loss_s{space}"] = np.array(
                    [R.get_loss(kind, mats, Y, X[:, b], space, R.FLOAT, int(tu[b])) for b in range(3)])
                for b in range(3):
                    jobs.append((kind, mats, Y, X[:, b].copy(), space, int(tu[b])))
                    keys.append((pre, space, b))
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][1].size * jobs[i][5])  # the long cases first
    with Pool(processes) as pool:
        res = pool.map(fd_gradient, [jobs[i] for i in order], chunksize=1)
    worst = 0.0
    for i, (g, e) in zip(order, res):
        pre, space, b = keys[i]
        kind, mats, Y, x, _, tu = jobs[i]
        out.setdefault(f"{pre}_g_fd_s{space}", np.empty((len(g), 3)))[:, b] = g
        out.setdefault(f"{pre}_e_fd_s{space}", np.empty(3))[b] = e
        if np.isfinite(g).all():
            K, top = n_lead(kind), np.max(np.abs(g))
            assert np.all(np.abs(g[:K]) >= SCREEN * top), (pre, space, b, g[:K], top)  # the screen, on the truth
            ga = analytic(kind, mats, Y, x, space, tu)[1]
            ratio = float(np.max(np.abs(ga - g)) / top)
            worst = max(worst, ratio)
            if ratio > 1e-9:
                print(f"{pre} space {space} b={b}: formulas / truth ratio {ratio:.3e}")
    print(f"worst max|g_formulas - g_fd| / |g_fd|inf over the fixture: {worst:.3e}")
    return out


def load_cases():
    with np.load(FILE) as z:
        return {k: z[k] for k in z.files}


def case_names():
    return [f"k{kind}_{tag}" for kind in KINDS for tag, *_ in CASES]


if __name__ == "__main__":
    np.savez_compressed(FILE, **build())
    c = load_cases()
    for k in sorted(c):
        if "_e_fd_" in k:
            print(k, c[k], np.max(np.abs(c[k.replace("_e_fd_", "_g_fd_")]), axis=0))
