"""Generator of tests/golden/smooth_long/smooth_long_cases.npz: the fixed-interval smoother's references at estimation
length (include/yfm.h yfm_smooth_batch), from tests/smoother_reference.py as tests/golden/smooth/make_smooth.py makes
the short ones — the dense FP64 checker (N × N F_t, RTS gain) against the same recursion in 40-digit mpmath, the truth.

Cases, each the smallest shape that reaches the stated branch of smooth_kernel (a chunk is 64 columns):

  SL-chunk  DNS  N = 6,  T = 200, B = 3  an interior chunk and windows that end on, one past and two past a chunk
                                         boundary: T_use ∈ {128, 129, 130, 192, 193, 200}.  Missing (1-based): column 64
                                         whole, one entry of 65, columns 128 and 129 whole, one entry of column 200 —
                                         the L = Φ branch on both sides of the hand-over of r and N.  The last
                                         candidate has a Φ eigenvalue of 0.999 (make_smooth.unit_root_theta)
  SL-n64    DNS  N = 64, T = 130, B = 2  all 64 rows of the forward launch's z̃ tile with three chunks; one NaN entry
                                         in column 65
  SL-hard   DNS  N = 30, T = 600, B = 4  the bench panel with bench columns 10283, 1679 (the hard candidates of
                                         tests/golden/dns_hard_T600.npz), 0 and 1
  GL-chunk  GNS5 N = 7,  T = 200, B = 3  M = 5 across chunks: G-E's maturities; SL-chunk's missing layout, windows and
                                         near-unit-root last candidate
  GL-n30    GNS5 N = 30, T = 130, B = 2  M = 5 at the workload's N

Candidates are θ₀ + 0.02·N(0, I) but for SL-hard's.  Seeds: 4300 + the case's index for the panel, that + 50 + 100·k for
the candidates; for GL-n30 k is the first with κ₁(Z'Z) ≤ 5e5 at every candidate (NumPy's 1-norm condition number; the
forward launch defers a candidate at 1e6, and a deferred candidate has no states to compare).  k = 0 serves.

What is stored differs from make_smooth.py, to keep the file under 512 KiB at these lengths:

  * the checker is not stored: it costs milliseconds and the tests run it;
  * per candidate b, window w and array (β̂, V, C), `e_ct[b, w, :]` is the checker's distance from the truth under the
    rule's measure (smoother_reference.traj_err: per-step normwise error against the truth's magnitude);
  * `hard[b]`: some e_ct[b] is above GEN_REL = 1e-10.  Only a hard candidate's truth is stored — float64, V as its packed
    upper triangle, per window (`w<n>_b<b>_beta`, `_Vu`, `_C`), unconstrained space only;
  * so every candidate is either within 1e-10 of the truth in every array (asserted; the margin of make_smooth.py, a
    decade below the 1e-9 bar from the reference alone) or carries its truth — the constructed near-unit-root
    candidates included, which are hard whenever they exceed it.  SL-hard's `hard` is asserted to be
    [True, True, False, False];
  * SL-hard's panel is the one tests/golden/grad/grad_long_cases.npz stores under L, and is read from there;
  * `kappa1` for the GNS5 cases.

Run from the repository root:  python tests/golden/smooth_long/make_smooth_long.py    # minutes; it prints its own time
"""
from __future__ import annotations

import multiprocessing as mproc
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
for p in (str(ROOT / "yieldfactormodels.jl_amd"), str(ROOT), str(ROOT / "tests"), str(HERE.parent / "smooth")):
    if p not in sys.path:
        sys.path.insert(0, p)

import smoother_reference as SR  # noqa: E402
from make_smooth import maturities, pack_upper, unit_root_theta, unpack_upper  # noqa: E402
from yfm_amd import KIND_DNS, KIND_GNS  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "smooth_long_cases.npz"
SHARED_PANEL = HERE.parent / "grad" / "grad_long_cases.npz"  # L/Y, L/maturities: the bench panel
CASES = ("SL-chunk", "SL-n64", "SL-hard", "GL-chunk", "GL-n30")
WINDOWS_CHUNK = (128, 129, 130, 192, 193, 200)
HARD_COLUMNS = (10283, 1679, 0, 1)
GEN_REL = 1e-10
SCALE = 0.02
KAPPA_MAX = 5e5
MAX_BYTES = 512 * 1024
SHAPES = {"SL-chunk": (6, 200, 3), "SL-n64": (64, 130, 2), "SL-hard": (30, 600, 4), "GL-chunk": (7, 200, 3),
          "GL-n30": (30, 130, 2)}
ARRAYS = ("beta", "V", "C")


def chunk_missing(Y):
    """The missing layout of the chunk cases (1-based columns): 64 whole, one entry of 65, 128 and 129 whole, one entry
    of 200."""
    Y[:, 63] = np.nan
    Y[2, 64] = np.nan
    Y[:, 127] = np.nan
    Y[:, 128] = np.nan
    Y[2, 199] = np.nan


def kappa1(kind, m, theta):
    """NumPy's 1-norm condition number of Z'Z at θ."""
    Z = SR.model_fp64(kind, m, theta)[0]
    return float(np.linalg.cond(Z.T @ Z, 1))


def case_inputs(name):
    """(kind, Y, maturities, Theta, windows, index of the near-unit-root candidate or −1)."""
    seed = 4300 + CASES.index(name)
    kind = KIND_GNS if name.startswith("GL") else KIND_DNS
    N, T, B = SHAPES[name]
    unit = -1
    if name == "SL-hard":
        Y = S.simulate_panel(KIND_DNS, T)
        Th = S.theta_batch(KIND_DNS, 65536)[:, list(HARD_COLUMNS)]
        return kind, Y, S.maturities_30(), np.asfortranarray(Th), (T,), unit
    m = np.array([3.0, 6.0, 18.0, 24.0, 60.0, 72.0, 360.0]) if name == "GL-chunk" else maturities(N)
    Y = S.simulate_panel(kind, T, m, seed).copy()
    k = 0
    while True:
        Th = S.theta_batch(kind, B, SCALE, seed + 50 + 100 * k, bad_frac=0)
        if name != "GL-n30" or all(kappa1(kind, m, Th[:, b]) <= KAPPA_MAX for b in range(B)):
            break
        k += 1
    windows = (T,)
    if name in ("SL-chunk", "GL-chunk"):
        chunk_missing(Y)
        unit = B - 1
        Th[:, unit] = unit_root_theta(kind, Th[:, unit])
        windows = WINDOWS_CHUNK
    if name == "SL-n64":
        Y[2, 64] = np.nan
    return kind, Y, m, np.asfortranarray(Th), windows, unit


def _truth_job(job):
    kind, m, Y, theta, n = job
    return SR.smooth_mp(kind, m, Y, theta, 0, n)


def make_case(pool, name):
    kind, Y, m, Th, windows, unit = case_inputs(name)
    B = Th.shape[1]
    truth = pool.map(_truth_job, [(kind, m, Y, Th[:, b], n) for b in range(B) for n in windows], chunksize=1)
    out = dict(kind=np.int64(kind), Y=Y, maturities=m, Theta=Th, windows=np.asarray(windows, dtype=np.int64),
               unit_root=np.int64(unit))
    e_ct = np.empty((B, len(windows), 3))
    for b in range(B):
        for wi, n in enumerate(windows):
            chk = SR.smooth_dense(kind, m, Y, Th[:, b], 0, n)
            tru = truth[b * len(windows) + wi]
            for k, what in enumerate(ARRAYS):
                e_ct[b, wi, k] = SR.traj_err(chk[k], tru[k], tru[k])
                print(f"{name} n={n} b={b} {what}: checker vs truth {e_ct[b, wi, k]:.2e}", flush=True)
    hard = (e_ct > GEN_REL).any(axis=(1, 2))
    assert (e_ct[~hard] <= GEN_REL).all()
    if name == "SL-hard":
        assert hard.tolist() == [True, True, False, False], hard
    for b in np.flatnonzero(hard):
        for wi, n in enumerate(windows):
            tru = truth[b * len(windows) + wi]
            out[f"w{n}_b{b}_beta"], out[f"w{n}_b{b}_Vu"], out[f"w{n}_b{b}_C"] = tru[0], pack_upper(tru[1]), tru[2]
    out["hard"], out["e_ct"] = hard, e_ct
    if kind == KIND_GNS:
        out["kappa1"] = np.array([kappa1(kind, m, Th[:, b]) for b in range(B)])
        assert name != "GL-n30" or (out["kappa1"] <= KAPPA_MAX).all()
    return out


def load_cases(path=FILE) -> dict:
    """{case: {kind, Y, maturities, Theta, windows (tuple), unit_root, hard, e_ct[B, W, 3], truth}}; truth[(n, b)] is
    the (β̂, V, C) of a hard candidate on the window of n columns, V unpacked.  SL-hard gets the shared bench panel."""
    with np.load(path, allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    raw = {}
    for key, v in flat.items():
        name, field = key.split("/", 1)
        raw.setdefault(name, {})[field] = v
    with np.load(SHARED_PANEL, allow_pickle=False) as z:
        raw["SL-hard"]["Y"], raw["SL-hard"]["maturities"] = z["L/Y"], z["L/maturities"]
    cases = {}
    for name in CASES:
        c = raw[name]
        kind = int(c["kind"])
        M = SR.STATE_DIM[kind]
        truth = {}
        for b in np.flatnonzero(c["hard"]):
            for n in c["windows"]:
                pre = f"w{int(n)}_b{int(b)}_"
                truth[(int(n), int(b))] = (c[pre + "beta"], unpack_upper(c[pre + "Vu"], M), c[pre + "C"])
        cases[name] = dict(kind=kind, Y=c["Y"], maturities=c["maturities"], Theta=c["Theta"],
                           windows=tuple(int(n) for n in c["windows"]), unit_root=int(c["unit_root"]),
                           hard=c["hard"], e_ct=c["e_ct"], truth=truth)
        if "kappa1" in c:
            cases[name]["kappa1"] = c["kappa1"]
    return cases


def main():
    t0 = time.time()
    flat = {}
    with mproc.Pool(16) as pool:
        for name in CASES:
            c = make_case(pool, name)
            if name == "SL-hard":  # the panel of grad_long_cases.npz's L
                with np.load(SHARED_PANEL, allow_pickle=False) as z:
                    assert np.array_equal(z["L/Y"], c["Y"]) and np.array_equal(z["L/maturities"], c["maturities"])
                del c["Y"], c["maturities"]
            for k, v in c.items():
                flat[f"{name}/{k}"] = v
            print(f"{name} done at {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(FILE, **flat)
    assert FILE.stat().st_size < MAX_BYTES, FILE.stat().st_size
    print(f"wrote {FILE} ({FILE.stat().st_size} bytes) in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
