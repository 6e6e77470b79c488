"""Generator of tests/golden/tvl_info/tvl_info_cases.npz: reference score series and Hessians of the TVλ
log-likelihood that use no derivative code.  It follows tests/golden/info/make_info.py, which does the same for DNS.

Truth scores (cases S-n4, S-nan, S-n67; unconstrained space) — nested windows of make_tvl_grad.fd_gradient on the
binary128 truth, with that generator's step ladder per window: s_k = g_fd(T_use = k+2) − g_fd(T_use = k+1),
e_fd[b] = max_k of the two windows' e_fd summed; g_fd is the whole window's gradient.
    S-n4:  N = 4, T = 8 — fewer maturities than lanes per candidate.
    S-nan: make_tvl_grad's case C panel (N = 7, T = 12) with column 5 all NaN and one entry of column 9 missing.
    S-n67: N = 67, T = 10 — three maturities on some lanes.

Truth Hessians (cases H-n4: N = 4, T = 8; H-nan: N = 6, T = 12 with a missing column and a missing entry) — central
second differences of the 40-digit oracle (oracle.kalman_mp.loglik_mp(KIND_TVL, …)), the perturbed points formed in
40-digit arithmetic, at the step h of H_LADDER whose difference to the 3h value is smallest: e_fd[b] = max |H_h − H_3h|.
loglik_mp rounds its result to float64 on return, so main() runs it with that module's name `float` bound to the
identity (make_info.full_precision: only while the worker pool lives; nothing of oracle/ is changed or copied).
    ref_err[b]: the error, against the truth Hessian, of a plain FP64 reference of the same operation — the same second
differences of the dense FP64 oracle (oracle.truth.loglik_oracle) at its best step of 1e-1 … 1e-5.

Selection: every stored candidate is compared.  Per case and seed a pool of 16 candidates is drawn and the first that
pass — by the reference alone — are kept: all truth evaluations finite, e_fd ≤ 1e-9 of the largest entry (of g_fd, of
H_truth) and, for scores, the dense oracle's loglik within 1e-9·max(1, |truth|) of the truth on every window.  The first
of ten seeds that fills the quota is used; the script prints how many candidates were replaced and how long it ran.

A point where H is usable (case E2E): one (panel, θ) at N = 6, T = 40 from a few hundred scipy L-BFGS iterations on the
dense oracle from θ₀; the 40-digit truth Hessian there and whether it is negative definite (negdef).

Run from the repository root:  python tests/golden/tvl_info/make_tvl_info.py      # minutes; it prints its own time
"""
from __future__ import annotations

import multiprocessing as mproc
import sys
import time
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "tvl_grad"))
sys.path.insert(0, str(HERE.parent / "info"))

import make_tvl_grad as MG  # noqa: E402  (fd_gradient and its ladder; it puts the repository on sys.path)
import make_info as MI  # noqa: E402  (the stencils and full_precision)
from oracle import kalman_mp as KM  # noqa: E402
from oracle import truth as TR  # noqa: E402
from yfm_amd import KIND_TVL  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "tvl_info_cases.npz"
H_LADDER = ("1e-8", "1e-9")
REL = 1e-9
ORACLE_REL = 1e-9
REF_STEPS = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-5)
HESS_CASES = ("H-n4", "H-nan")
SCORE_CASES = ("S-n4", "S-nan", "S-n67")
POOL = 16   # candidates drawn per seed; the first that pass are kept
SEEDS = 10  # seeds tried per case


def case_inputs(name: str, seed_no: int = 0):
    """(Y, maturities, candidate pool of seed number seed_no, number kept) of a case."""
    m30 = S.maturities_30()

    def pool(seed):
        return S.theta_batch(KIND_TVL, POOL, 0.02, seed + 100 * seed_no, bad_frac=0)

    if name in ("S-n4", "H-n4"):
        m = m30[[1, 7, 13, 22]]
        return S.simulate_panel(KIND_TVL, 8, m, 5), m, pool(41), 3 if name == "S-n4" else 2
    if name == "S-nan":
        Y, m, _, _ = MG.case_inputs("C")
        Y = Y.copy()
        Y[:, 5] = np.nan
        Y[3, 9] = np.nan
        return Y, m, pool(42), 3
    if name == "S-n67":
        m = np.linspace(3, 360, 67)
        return S.simulate_panel(KIND_TVL, 10, m, 5), m, pool(43), 2
    if name == "H-nan":
        m = m30[::5]
        Y = S.simulate_panel(KIND_TVL, 12, m, 21).copy()
        Y[:, 5] = np.nan
        Y[2, 9] = np.nan
        return Y, m, pool(44), 2
    raise KeyError(name)


# ---- truth scores -------------------------------------------------------------------------------------------------
def ladder_gradient(Y, m, X, tu):
    """make_tvl_grad.make_case's choice per column of X: (g_fd, e_fd, finite) at the ladder step with the smallest
    e(h)/‖g_h‖∞."""
    B = X.shape[1]
    steps = sorted({h for h0 in MG.LADDER for h in (h0, 3.0 * h0)})
    gs = {h: MG.fd_gradient(Y, m, X, tu, h) for h in steps}
    g_fd, e_fd, ratio, used = np.zeros_like(X), np.full(B, np.inf), np.full(B, np.inf), np.zeros(B, dtype=bool)
    ok = np.ones(B, dtype=bool)
    for h in steps:
        ok &= gs[h][1]
    for h in MG.LADDER:
        g1, g3 = gs[h][0], gs[3.0 * h][0]
        e = np.abs(g1 - g3).max(axis=0)
        gn = np.abs(g1).max(axis=0)
        r = np.where(gn > 0, e / np.where(gn > 0, gn, 1.0), np.where(e == 0, 0.0, np.inf))
        r = np.where(np.isfinite(r), r, np.inf)
        better = (r < ratio) | (~used & (r <= ratio))  # a window with no term: zero at every step
        g_fd[:, better] = g1[:, better]
        e_fd[better] = e[better]
        ratio[better] = r[better]
        used |= better
    return g_fd, e_fd, ok


def window_gradients(Y, m, Th):
    """(g[P, T, B]: the difference gradient on the window of w + 1 columns, w = 0 … T − 1; e[T, B]; usable[B])."""
    P, B = Th.shape
    T = Y.shape[1]
    X = np.asfortranarray(np.repeat(Th, T, axis=1))  # candidate b's windows 1 … T side by side
    tu = np.tile(np.arange(1, T + 1, dtype=np.int32), B)
    with np.errstate(all="ignore"):
        g, e, ok = ladder_gradient(Y, m, X, tu)
        truth = TR.loglik_truth(KIND_TVL, Y, m, X, space=0, T_use=tu)
        oracle = TR.loglik_oracle(KIND_TVL, Y, m, X, space=0, T_use=tu)
        near = np.isfinite(truth) & (np.abs(oracle - truth) <= ORACLE_REL * np.maximum(1.0, np.abs(truth)))
    ok = (ok & near).reshape(B, T).all(axis=1)
    return g.reshape(P, B, T).transpose(0, 2, 1), e.reshape(B, T).T, ok


def make_score_case(name: str) -> dict:
    for seed_no in range(SEEDS):
        Y, m, Th, keep = case_inputs(name, seed_no)
        T = Y.shape[1]
        g, e, ok = window_gradients(Y, m, Th)
        # column k of the scores (k = 1 … T − 2): the windows of k + 2 and k + 1 columns; column 0 holds no term
        s = np.zeros((Th.shape[0], T - 1, Th.shape[1]))
        s[:, 1:, :] = g[:, 2:, :] - g[:, 1:-1, :]
        e_fd = (e[2:] + e[1:-1]).max(axis=0)
        g_fd = g[:, T - 1, :]
        good = ok & (e_fd <= REL * np.abs(g_fd).max(axis=0))
        kept = np.flatnonzero(good)[:keep]
        if kept.size == keep:
            break
        print(f"{name}: seed number {seed_no} fills {kept.size} of {keep}")
    assert kept.size == keep, (name, "no seed fills the quota: shrink T")
    replaced = int(kept[-1] + 1 - keep)
    print(f"{name}: seed number {seed_no}, kept pool columns {kept.tolist()}, replaced {replaced}; e_fd/|g| "
          f"{(e_fd[kept] / np.abs(g_fd[:, kept]).max(axis=0)).tolist()}")
    Thk = np.asfortranarray(Th[:, kept])
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Thk, s_truth=np.asfortranarray(s[:, :, kept]),
                g_fd=np.asfortranarray(g_fd[:, kept]), e_fd=e_fd[kept], replaced=np.array(replaced),
                seed_no=np.array(seed_no), loglik_truth=TR.loglik_truth(KIND_TVL, Y, m, Thk, space=0))


# ---- truth Hessians ----------------------------------------------------------------------------------------------
def _ll_mp(job):
    Y, m, theta = job
    return KM.loglik_mp(KIND_TVL, m, Y, theta, space=0)[0]


def truth_hessian(pool, Y, m, th):
    """(H at the kept step as float64, e_fd, finite, the kept step)."""
    P = len(th)
    best = (None, np.inf, False, "")
    for hs in H_LADDER:
        Hs = []
        for mult in (1, 3):
            h = mult * mp.mpf(hs)
            f = pool.map(_ll_mp, [(Y, m, p) for p in MI.hessian_points(th, h)], chunksize=8)
            if not all(mp.isfinite(v) for v in f):
                return None, np.inf, False, hs
            Hs.append(MI.hessian_from_values(f, P, h))
        e_fd = max(abs(float(Hs[0][i][j] - Hs[1][i][j])) for i in range(P) for j in range(P))
        if e_fd < best[1]:
            best = (np.array([[float(v) for v in row] for row in Hs[0]]), e_fd, True, hs)
    return best


def oracle_hessian(Y, m, th, h):
    """The same two stencils on the dense FP64 oracle, in plain float64."""
    P = th.size
    cols = [th.copy()]
    for i in range(P):
        for s in (h, -h):
            x = th.copy()
            x[i] += s
            cols.append(x)
    for i in range(P):
        for j in range(i + 1, P):
            for si, sj in ((h, h), (h, -h), (-h, h), (-h, -h)):
                x = th.copy()
                x[i] += si
                x[j] += sj
                cols.append(x)
    f = TR.loglik_oracle(KIND_TVL, Y, m, np.asfortranarray(np.stack(cols, axis=1)), space=0)
    return np.array(MI.hessian_from_values(list(f), P, h), dtype=np.float64)


def reference_error(Y, m, th, H):
    with np.errstate(all="ignore"):
        errs = [np.abs(oracle_hessian(Y, m, th, h) - H).max() for h in REF_STEPS]
    errs = [e if np.isfinite(e) else np.inf for e in errs]
    return min(errs), REF_STEPS[int(np.argmin(errs))]


def make_hessian_case(pool, name: str) -> dict:
    for seed_no in range(SEEDS):
        Y, m, Th, keep = case_inputs(name, seed_no)
        kept, Hs, es, hs_used, refs, ref_steps, replaced = [], [], [], [], [], [], 0
        for b in range(Th.shape[1]):
            if len(kept) == keep:
                break
            H, e_fd, ok, hs = truth_hessian(pool, Y, m, Th[:, b])
            if not (ok and e_fd <= REL * np.abs(H).max()):
                replaced += 1
                continue
            r, rs = reference_error(Y, m, Th[:, b], H)
            kept.append(b)
            Hs.append(H)
            es.append(e_fd)
            hs_used.append(float(hs))
            refs.append(r)
            ref_steps.append(rs)
        if len(kept) == keep:
            break
        print(f"{name}: seed number {seed_no} fills {len(kept)} of {keep}")
    assert len(kept) == keep, (name, "no seed fills the quota: shrink T")
    Thk = np.asfortranarray(Th[:, kept])
    print(f"{name}: seed number {seed_no}, kept pool columns {kept}, replaced {replaced}; steps {hs_used}; e_fd/|H| "
          f"{[e / np.abs(H).max() for e, H in zip(es, Hs)]}, ref_err/|H| {[r / np.abs(H).max() for r, H in zip(refs, Hs)]}"
          f" at steps {ref_steps}")
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Thk, H_truth=np.stack(Hs, axis=2),
                e_fd=np.array(es), h_used=np.array(hs_used), ref_err=np.array(refs), ref_step=np.array(ref_steps),
                replaced=np.array(replaced), seed_no=np.array(seed_no),
                loglik_truth=TR.loglik_truth(KIND_TVL, Y, m, Thk, space=0))


# ---- a point where H is usable ------------------------------------------------------------------------------------
def make_e2e_case(pool) -> dict:
    from scipy.optimize import minimize
    m = S.maturities_30()[::5]
    Y = S.simulate_panel(KIND_TVL, 40, m, 7)
    x0 = S.theta0(KIND_TVL)

    def nll(x):
        v = TR.loglik_oracle(KIND_TVL, Y, m, np.asfortranarray(x.reshape(-1, 1)), space=0)[0]
        return -v if np.isfinite(v) else 1e300

    r = minimize(nll, x0, method="L-BFGS-B", options=dict(maxiter=400, maxfun=100000, ftol=1e-15, gtol=1e-9))
    th = np.asarray(r.x, dtype=np.float64)
    H, e_fd, ok, hs = truth_hessian(pool, Y, m, th)
    negdef = bool(ok and np.linalg.eigvalsh(H).max() < 0.0)
    ref, ref_step = reference_error(Y, m, th, H) if ok else (np.inf, 0.0)
    eig = np.linalg.eigvalsh(H) if ok else np.full(th.size, np.nan)
    print(f"E2E: {r.nit} iterations, loglik {-r.fun:.6f} (θ₀: {-nll(x0):.6f}), truth H finite {ok}, e_fd/|H| "
          f"{e_fd / np.abs(H).max() if ok else np.inf:.2e}, eigenvalues {eig.min():.3e} … {eig.max():.3e}: negative "
          f"definite {negdef}; ref_err/|H| {ref / np.abs(H).max() if ok else np.inf:.2e} at step {ref_step}")
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=np.asfortranarray(th.reshape(-1, 1)),
                Theta0=np.asfortranarray(x0.reshape(-1, 1)),
                H_truth=(H if ok else np.full((th.size, th.size), np.nan))[:, :, None], e_fd=np.array([e_fd]),
                ref_err=np.array([ref]), ref_step=np.array([ref_step]), negdef=np.array(negdef),
                loglik_truth=TR.loglik_truth(KIND_TVL, Y, m, th.reshape(-1, 1), space=0))


def load_cases(path=FILE) -> dict:
    """{case name: {field: array}} of the committed file."""
    return MG.load_cases(path)


def main():
    t0 = time.time()
    flat = {}
    for name in SCORE_CASES:
        for k, v in make_score_case(name).items():
            flat[f"{name}/{k}"] = v
        print(f"  … {time.time() - t0:.0f} s")
    with MI.full_precision(), mproc.Pool() as pool:
        for name in HESS_CASES:
            for k, v in make_hessian_case(pool, name).items():
                flat[f"{name}/{k}"] = v
            print(f"  … {time.time() - t0:.0f} s")
        for k, v in make_e2e_case(pool).items():
            flat[f"E2E/{k}"] = v
        print(f"  … {time.time() - t0:.0f} s")
    np.savez_compressed(FILE, **flat)
    print(f"wrote {FILE.name}: {FILE.stat().st_size} bytes in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
