"""Generator of tests/golden/info/info_cases.npz: reference Hessians and score series of the DNS log-likelihood that
use no derivative code.

Truth Hessians (cases H-E, H-nan; unconstrained space) — central second differences of the 40-digit oracle
(oracle.kalman_mp.loglik_mp): the 3-point stencil on the diagonal, the 4-point mixed stencil off it, the perturbed
points formed in 40-digit arithmetic so the steps are exact, at h = 1e-8 (kept) and 3e-8; e_fd[b] = max |H_1e-8 −
H_3e-8| bounds the kept value's error (the truncation term falls 9× between the two).  The binary128 truth cannot
serve here: its float64-rounded output limits second differences to about 1e-7 of an entry.  loglik_mp rounds its
result to float64 on return too, so main() runs it with that module's name `float` bound to the identity (full_precision:
only while the generator's worker pool lives; importing this module leaves the oracle alone, and nothing of oracle/ is
changed or copied).
    ref_err[b]: the error, against the truth Hessian, of a plain FP64 reference of the same operation — the same
second differences of the dense FP64 oracle (oracle.truth.loglik_oracle) at its best step of 1e-1 … 1e-5.

Truth scores (cases S-E, S-nan, S-n64) — nested windows of make_grad.fd_gradient on the binary128 truth:
s_k = g_fd(T_use = k+2) − g_fd(T_use = k+1), e_fd[b] = max_k of the two windows' e_fd summed; g_fd is the whole
window's gradient.

Every stored candidate is compared: all its truth evaluations are finite and e_fd ≤ 1e-9 of the largest entry (of
H_truth, of g_fd); a candidate that fails is replaced by the next of the same seed, and the script prints how many were.

Run from the repository root:  python tests/golden/info/make_info.py      # minutes; it prints its own time
"""
from __future__ import annotations

import contextlib
import multiprocessing as mproc
import sys
import time
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "grad"))

import make_grad as MG  # noqa: E402  (fd_gradient; it puts the repository on sys.path)
from oracle import kalman_mp as KM  # noqa: E402
from oracle import truth as TR  # noqa: E402
from yfm_amd import KIND_DNS  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "info_cases.npz"
H_STEPS = ("1e-8", "3e-8")
REL = 1e-9
REF_STEPS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5)
HESS_CASES = ("H-E", "H-nan")
SCORE_CASES = ("S-E", "S-nan", "S-n64")
POOL = 16  # candidates drawn per seed; the first that pass are kept


def case_inputs(name: str):
    """(Y, maturities, candidate pool, number kept) of a case."""
    m30 = S.maturities_30()
    if name in ("H-E", "S-E"):  # make_grad's case E: N = 4 (fewer maturities than lanes per candidate), T = 8
        Y, m, Th, _ = MG.case_inputs("E")
        return Y, m, Th[:, :POOL], 2
    if name == "H-nan":
        m = m30[::5]
        Y = S.simulate_panel(KIND_DNS, 12, m, 21).copy()
        Y[:, 5] = np.nan
        Y[2, 9] = np.nan
        return Y, m, S.theta_batch(KIND_DNS, POOL, 0.1, 22, bad_frac=0), 2
    if name == "S-nan":  # make_grad's case A-nan: NaN entries in columns 5, 20 and 39, column 6 all NaN
        Y, m, Th, _ = MG.case_inputs("A-nan")
        return Y, m, Th[:, :POOL], 3
    if name == "S-n64":
        Y, m, Th, _ = MG.case_inputs("D")
        return Y, m, Th[:, :POOL], 2
    raise KeyError(name)


# ---- truth Hessians ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def full_precision():
    """loglik_mp's float(ll) keeps its 40 digits inside this block (and in the worker processes forked inside it)."""
    KM.float = lambda x: x
    try:
        yield
    finally:
        del KM.float


def _ll_mp(job):
    Y, m, theta = job
    return KM.loglik_mp(KIND_DNS, m, Y, theta, space=0)[0]


def hessian_points(th, h):
    """The 40-digit points of both stencils around th (float64): the centre, ±h e_i, (±h, ±h) on every pair i < j."""
    P = len(th)
    x = [mp.mpf(float(v)) for v in th]

    def moved(*steps):
        y = list(x)
        for i, s in steps:
            y[i] = y[i] + s
        return y

    pts = [moved()]
    for i in range(P):
        pts += [moved((i, h)), moved((i, -h))]
    for i in range(P):
        for j in range(i + 1, P):
            pts += [moved((i, h), (j, h)), moved((i, h), (j, -h)), moved((i, -h), (j, h)), moved((i, -h), (j, -h))]
    return pts


def hessian_from_values(f, P, h):
    H = [[None] * P for _ in range(P)]
    k = 1
    for i in range(P):
        H[i][i] = (f[k] - 2 * f[0] + f[k + 1]) / (h * h)
        k += 2
    for i in range(P):
        for j in range(i + 1, P):
            H[i][j] = H[j][i] = (f[k] - f[k + 1] - f[k + 2] + f[k + 3]) / (4 * h * h)
            k += 4
    return H


def truth_hessian(pool, Y, m, th):
    """(H at h = 1e-8 as float64, e_fd, finite)."""
    P = len(th)
    Hs = []
    for hs in H_STEPS:
        h = mp.mpf(hs)
        f = pool.map(_ll_mp, [(Y, m, p) for p in hessian_points(th, h)], chunksize=8)
        if not all(mp.isfinite(v) for v in f):
            return None, np.inf, False
        Hs.append(hessian_from_values(f, P, h))
    H1 = np.array([[float(v) for v in row] for row in Hs[0]])
    e_fd = max(abs(float(Hs[0][i][j] - Hs[1][i][j])) for i in range(P) for j in range(P))
    return H1, e_fd, True


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
    f = TR.loglik_oracle(KIND_DNS, Y, m, np.asfortranarray(np.stack(cols, axis=1)), space=0)
    return np.array(hessian_from_values(list(f), P, h), dtype=np.float64)


def make_hessian_case(pool, name: str) -> dict:
    Y, m, Th, keep = case_inputs(name)
    kept, Hs, es, refs, ref_steps, replaced = [], [], [], [], [], 0
    for b in range(Th.shape[1]):
        if len(kept) == keep:
            break
        H, e_fd, ok = truth_hessian(pool, Y, m, Th[:, b])
        if not (ok and e_fd <= REL * np.abs(H).max()):
            replaced += 1
            continue
        with np.errstate(all="ignore"):
            errs = [np.abs(oracle_hessian(Y, m, Th[:, b], h) - H).max() for h in REF_STEPS]
        errs = [e if np.isfinite(e) else np.inf for e in errs]
        kept.append(b)
        Hs.append(H)
        es.append(e_fd)
        refs.append(min(errs))
        ref_steps.append(REF_STEPS[int(np.argmin(errs))])
    assert len(kept) == keep, (name, kept)
    Thk = np.asfortranarray(Th[:, kept])
    print(f"{name}: kept pool columns {kept}, replaced {replaced}; e_fd/|H| "
          f"{[e / np.abs(H).max() for e, H in zip(es, Hs)]}, ref_err/|H| {[r / np.abs(H).max() for r, H in zip(refs, Hs)]}"
          f" at steps {ref_steps}")
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Thk, H_truth=np.stack(Hs, axis=2),
                e_fd=np.array(es), ref_err=np.array(refs), ref_step=np.array(ref_steps), replaced=np.array(replaced),
                loglik_truth=TR.loglik_truth(KIND_DNS, Y, m, Thk, space=0))


# ---- truth scores -------------------------------------------------------------------------------------------------
def window_gradients(Y, m, Th):
    """(g[P, T, B]: the difference gradient on the window of w + 1 columns, w = 0 … T − 1; e[T, B]; finite[B])."""
    P, B = Th.shape
    T = Y.shape[1]
    X = np.asfortranarray(np.repeat(Th, T, axis=1))  # candidate b's windows 1 … T side by side
    tu = np.tile(np.arange(1, T + 1, dtype=np.int32), B)
    with np.errstate(all="ignore"):
        g1, ok1 = MG.fd_gradient(Y, m, X, tu, MG.H1)
        g2, ok2 = MG.fd_gradient(Y, m, X, tu, MG.H2)
    e = np.abs(g1 - g2).max(axis=0).reshape(B, T).T
    ok = (ok1 & ok2).reshape(B, T).all(axis=1)
    return g1.reshape(P, B, T).transpose(0, 2, 1), e, ok


def make_score_case(name: str) -> dict:
    Y, m, Th, keep = case_inputs(name)
    T = Y.shape[1]
    g, e, ok = window_gradients(Y, m, Th)
    # column k of the scores (k = 1 … T − 2): the windows of k + 2 and k + 1 columns; columns 0 (and T − 1) hold no term
    s = np.zeros((Th.shape[0], T - 1, Th.shape[1]))
    s[:, 1:, :] = g[:, 2:, :] - g[:, 1:-1, :]
    e_fd = (e[2:] + e[1:-1]).max(axis=0)
    g_fd = g[:, T - 1, :]
    good = ok & (e_fd <= REL * np.abs(g_fd).max(axis=0))
    kept = np.flatnonzero(good)[:keep]
    replaced = int(kept[-1] + 1 - keep) if kept.size == keep else -1
    assert kept.size == keep, (name, good)
    print(f"{name}: kept pool columns {kept.tolist()}, replaced {replaced}; e_fd/|g| "
          f"{(e_fd[kept] / np.abs(g_fd[:, kept]).max(axis=0)).tolist()}")
    Thk = np.asfortranarray(Th[:, kept])
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Thk, s_truth=np.asfortranarray(s[:, :, kept]),
                g_fd=np.asfortranarray(g_fd[:, kept]), e_fd=e_fd[kept], replaced=np.array(replaced),
                loglik_truth=TR.loglik_truth(KIND_DNS, Y, m, Thk, space=0))


def load_cases(path=FILE) -> dict:
    """{case name: {field: array}} of the committed file."""
    return MG.load_cases(path)


def main():
    t0 = time.time()
    flat = {}
    for name in SCORE_CASES:
        for k, v in make_score_case(name).items():
            flat[f"{name}/{k}"] = v
    with full_precision(), mproc.Pool() as pool:
        for name in HESS_CASES:
            for k, v in make_hessian_case(pool, name).items():
                flat[f"{name}/{k}"] = v
            print(f"  … {time.time() - t0:.0f} s")
    np.savez_compressed(FILE, **flat)
    print(f"wrote {FILE.name}: {FILE.stat().st_size} bytes in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
