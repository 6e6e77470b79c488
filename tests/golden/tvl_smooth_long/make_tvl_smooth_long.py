"""Generator of tests/golden/tvl_smooth_long/tvl_smooth_long_cases.npz: the TVλ extended smoother's references at
estimation length (include/yfm.h yfm_tvl_smooth_batch), from tests/tvl_smoother_reference.py as
tests/golden/tvl_smooth/make_tvl_smooth.py makes the short ones — the dense FP64 checker (EKF with the N × N F_t, RTS
gain) against the same recursion in 40-digit mpmath, the truth.

Cases, each the smallest shape that reaches the stated branch of tvl_smooth_kernel (a chunk is 64 columns):

  TL-chunk  N = 6,  T = 200, B = 3  make_smooth_long.py's SL-chunk: an interior chunk, windows T_use ∈ {128, 129, 130,
                                    192, 193, 200}, missing columns on both sides of a chunk boundary
                                    (make_smooth_long.chunk_missing), a near-unit-root last candidate
  TL-n90    N = 90, T = 130, B = 2  larger N across three chunks
  TL-600    N = 30, T = 600, B = 2  the panel of tests/golden/tvl_grad/tvl_grad_long_cases.npz's L600 with the first two
                                    of its candidates whose oracle loglik is finite

Seeds: 4400 + the case's index for the panel, that + 50 + 100·k for the candidates θ₀ + 0.02·N(0, I), with the first k
at which every candidate's oracle loglik is finite on every window (make_tvl_smooth.py documents why about half of the
TVλ candidates at this scale have none: a non-stationary Φ and an indefinite P_1); `seed_step` stores the k taken.
TL-600's candidates come from make_tvl_grad_long.case_inputs("L600") instead.

Stored as make_smooth_long.py stores its cases: no checker; `e_ct[b, w, :]`, the checker's distance from the truth per
candidate, window and array (β̂, V, C); `hard[b]`, some e_ct[b] above GEN_REL = 1e-10; the float64 truth of the hard
candidates only, V as its packed upper triangle, unconstrained space only.  Every candidate is therefore either within
1e-10 of the truth in every array (asserted) or carries its truth.  TL-600's panel is read from
tvl_grad_long_cases.npz (L600/Y).

Run from the repository root:  python tests/golden/tvl_smooth_long/make_tvl_smooth_long.py   # minutes; it prints its time
"""
from __future__ import annotations

import multiprocessing as mproc
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
for p in (str(ROOT / "yieldfactormodels.jl_amd"), str(ROOT), str(ROOT / "tests"), str(HERE.parent / "smooth"),
          str(HERE.parent / "smooth_long"), str(HERE.parent / "tvl_grad")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tvl_smoother_reference as TR  # noqa: E402
from oracle import kalman_oracle as O  # noqa: E402
from make_smooth import maturities, pack_upper, unit_root_theta, unpack_upper  # noqa: E402
from make_smooth_long import WINDOWS_CHUNK, chunk_missing  # noqa: E402
from yfm_amd import KIND_TVL  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "tvl_smooth_long_cases.npz"
SHARED_PANEL = HERE.parent / "tvl_grad" / "tvl_grad_long_cases.npz"  # L600/Y, L600/maturities
CASES = ("TL-chunk", "TL-n90", "TL-600")
GEN_REL = 1e-10
SCALE = 0.02
MAX_BYTES = 512 * 1024
SHAPES = {"TL-chunk": (6, 200, 3), "TL-n90": (90, 130, 2), "TL-600": (30, 600, 2)}
ARRAYS = ("beta", "V", "C")


def finite_loglik(m, Y, theta, windows):
    return all(np.isfinite(O.loglik(O.KIND_TVL, m, 4, Y[:, :n], theta, 0)) for n in windows)


def case_inputs(name):
    """(Y, maturities, Theta, windows, index of the near-unit-root candidate or −1, the k of the seed search)."""
    N, T, B = SHAPES[name]
    if name == "TL-600":
        import make_tvl_grad_long as ML
        Y, m, Th, _ = ML.case_inputs("L600")
        with np.errstate(all="ignore"):
            keep = [b for b in range(Th.shape[1]) if finite_loglik(m, Y, Th[:, b], (T,))][:B]
        return Y, np.asarray(m, dtype=np.float64), np.asfortranarray(Th[:, keep]), (T,), -1, 0
    seed = 4400 + CASES.index(name)
    m = maturities(N)
    Y = S.simulate_panel(KIND_TVL, T, m, seed).copy()
    windows, unit = (T,), -1
    if name == "TL-chunk":
        chunk_missing(Y)
        windows, unit = WINDOWS_CHUNK, B - 1
    k = 0
    while True:
        Th = S.theta_batch(KIND_TVL, B, SCALE, seed + 50 + 100 * k, bad_frac=0)
        if unit >= 0:
            Th[:, unit] = unit_root_theta(KIND_TVL, Th[:, unit])
        with np.errstate(all="ignore"):
            if all(finite_loglik(m, Y, Th[:, b], windows) for b in range(B)):
                break
        k += 1
    return Y, m, np.asfortranarray(Th), windows, unit, k


def _truth_job(job):
    m, Y, theta, windows = job
    return TR.smooth_mp_windows(m, Y, theta, 0, windows)


def make_case(inputs, truth, name):
    """The stored fields of a case from its inputs and its candidates' truths (one list over the windows each)."""
    Y, m, Th, windows, unit, k = inputs
    print(f"{name}: seed step k = {k}", flush=True)
    B = Th.shape[1]
    out = dict(Y=Y, maturities=m, Theta=Th, windows=np.asarray(windows, dtype=np.int64), unit_root=np.int64(unit),
               seed_step=np.int64(k))
    e_ct = np.empty((B, len(windows), 3))
    for b in range(B):
        f = TR.forward_dense(m, Y, Th[:, b], 0, max(windows))
        for wi, n in enumerate(windows):
            chk = TR.backward_dense(f, n)
            for j, what in enumerate(ARRAYS):
                e_ct[b, wi, j] = TR.traj_err(chk[j], truth[b][wi][j], truth[b][wi][j])
                print(f"{name} n={n} b={b} {what}: checker vs truth {e_ct[b, wi, j]:.2e}", flush=True)
    hard = (e_ct > GEN_REL).any(axis=(1, 2))
    assert (e_ct[~hard] <= GEN_REL).all()
    for b in np.flatnonzero(hard):
        for wi, n in enumerate(windows):
            tru = truth[b][wi]
            out[f"w{n}_b{b}_beta"], out[f"w{n}_b{b}_Vu"], out[f"w{n}_b{b}_C"] = tru[0], pack_upper(tru[1]), tru[2]
    out["hard"], out["e_ct"] = hard, e_ct
    return out


def load_cases(path=FILE) -> dict:
    """{case: {Y, maturities, Theta, windows (tuple), unit_root, seed_step, hard, e_ct[B, W, 3], truth}}; truth[(n, b)]
    is the (β̂, V, C) of a hard candidate on the window of n columns, V unpacked.  TL-600 gets the shared panel."""
    with np.load(path, allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    raw = {}
    for key, v in flat.items():
        name, field = key.split("/", 1)
        raw.setdefault(name, {})[field] = v
    with np.load(SHARED_PANEL, allow_pickle=False) as z:
        raw["TL-600"]["Y"], raw["TL-600"]["maturities"] = z["L600/Y"], z["L600/maturities"]
    cases = {}
    for name in CASES:
        c = raw[name]
        truth = {}
        for b in np.flatnonzero(c["hard"]):
            for n in c["windows"]:
                pre = f"w{int(n)}_b{int(b)}_"
                truth[(int(n), int(b))] = (c[pre + "beta"], unpack_upper(c[pre + "Vu"], 4), c[pre + "C"])
        cases[name] = dict(Y=c["Y"], maturities=c["maturities"], Theta=c["Theta"],
                           windows=tuple(int(n) for n in c["windows"]), unit_root=int(c["unit_root"]),
                           seed_step=int(c["seed_step"]), hard=c["hard"], e_ct=c["e_ct"], truth=truth)
    return cases


def main():
    t0 = time.time()
    flat = {}
    with mproc.Pool(16) as pool:
        inputs = {name: case_inputs(name) for name in CASES}
        # every case's truths at once, the longest first: a case has only two or three candidates
        pending = {}
        for name in ("TL-n90", "TL-600", "TL-chunk"):
            Y, m, Th, windows = inputs[name][:4]
            jobs = [(m, Y, Th[:, b], windows) for b in range(Th.shape[1])]
            pending[name] = pool.map_async(_truth_job, jobs, chunksize=1)
        for name in CASES:
            c = make_case(inputs[name], pending[name].get(), name)
            if name == "TL-600":  # the panel of tvl_grad_long_cases.npz's L600
                with np.load(SHARED_PANEL, allow_pickle=False) as z:
                    assert np.array_equal(z["L600/Y"], c["Y"]) and np.array_equal(z["L600/maturities"], c["maturities"])
                del c["Y"], c["maturities"]
            for k, v in c.items():
                flat[f"{name}/{k}"] = v
            print(f"{name} done at {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(FILE, **flat)
    assert FILE.stat().st_size < MAX_BYTES, FILE.stat().st_size
    print(f"wrote {FILE} ({FILE.stat().st_size} bytes) in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
