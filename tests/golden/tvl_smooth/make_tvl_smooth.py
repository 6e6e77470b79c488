"""Generator of tests/golden/tvl_smooth/tvl_smooth_cases.npz: the TVλ extended smoother's reference arrays
(include/yfm.h yfm_tvl_smooth_batch), from tests/tvl_smoother_reference.py — the dense FP64 checker (EKF with the N × N
F_t, RTS gain) and the same recursion in 40-digit mpmath as the truth.

Cases (the smallest shapes at which the kernel can still go wrong), candidates θ₀ + 0.02·N(0, I):

  T-E    N = 4,  T = 8    smallest shape
  T-nan  N = 6,  T = 12   columns 1 and 5 missing, one NaN entry in column 9, last column missing
  T-n30  N = 30, T = 70   crosses the sweep's 64-column chunk; windows T_use ∈ {1, 2, 3, 64, 65, 69, 70}; the last
                          candidate has a Φ eigenvalue of 0.999 (make_smooth.unit_root_theta)
  T-n90  N = 90, T = 12   larger N

The kernel does not tile the maturities (a lane walks all N of its column), so there is no T-nK case.

Stored per case, as make_smooth.py stores its arrays: Y, maturities, Theta (unconstrained), Theta_c (its transform) and,
per window n, the checker's β̂ (4 × n × B), packed upper triangles of V (10 × n × B) and C (4 × 4 × (n − 1) × B) in
float64 at the unconstrained θ; the truth as its float32 difference from the checker; and the constrained-space truth
as its float32 difference from the unconstrained one.  The constrained-space checker is cheap and is run by the tests.

The generator asserts, for every ordinary candidate, array and space, that the checker is within 1e-10 of the truth
under the rule's measure (per-step normwise error against the truth's magnitude), which leaves the 1e-9 bar a decade
from the reference alone.  The near-unit-root candidate alone is exempt.  It also asserts that the oracle's log-likelihood
of every candidate is finite on every window: a candidate with a −Inf loglik has no smoothed states to compare.

Seeds: 4200 + the case's index for the panel, that + 50 + 100·k for the candidates, with the first k whose candidates
all have a finite loglik.  k = 0 serves T-E, T-n30 and T-n90.  T-nan took k = 2: at θ₀ + 0.02·N(0, I) about half of the
TVλ candidates have a non-stationary Φ and an indefinite P_1; with column 1 missing, column 2 is then the first update
and the first term of the loss, and its determinant was negative (loglik −Inf) for candidates 1 and 2 at k = 0 and for
candidate 2 at k = 1.  (With data in column 1 the negative determinant falls on column 1, which the loss skips.)

Run from the repository root:  python tests/golden/tvl_smooth/make_tvl_smooth.py     # it prints its own time
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

import tvl_smoother_reference as TR  # noqa: E402
from oracle import kalman_oracle as O  # noqa: E402
from make_smooth import maturities, pack_upper, unit_root_theta, unpack_upper  # noqa: E402
from yfm_amd import KIND_TVL  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402
from yfm_amd.params import transform_params  # noqa: E402

FILE = HERE / "tvl_smooth_cases.npz"
CASES = ("T-E", "T-nan", "T-n30", "T-n90")
WINDOWS_N30 = (1, 2, 3, 64, 65, 69, 70)
GEN_REL = 1e-10
SCALE = 0.02
CAND_SEED_STEP = {"T-nan": 2}  # the k of the docstring's seed search (0 elsewhere)
SHAPES = {"T-E": (4, 8, 3), "T-nan": (6, 12, 3), "T-n30": (30, 70, 2), "T-n90": (90, 12, 2)}


def case_inputs(name):
    """(Y, maturities, Theta, windows, index of the near-unit-root candidate or −1)."""
    seed = 4200 + CASES.index(name)
    N, T, B = SHAPES[name]
    m = maturities(N)
    Y = S.simulate_panel(KIND_TVL, T, m, seed).copy()
    Th = S.theta_batch(KIND_TVL, B, SCALE, seed + 50 + 100 * CAND_SEED_STEP.get(name, 0), bad_frac=0)
    unit = -1
    if name == "T-nan":  # 1-based columns 1, 5 and the last missing; one NaN entry in column 9
        Y[:, 0] = np.nan
        Y[:, 4] = np.nan
        Y[2, 8] = np.nan
        Y[:, T - 1] = np.nan
    if name == "T-n30":
        unit = B - 1
        Th[:, unit] = unit_root_theta(KIND_TVL, Th[:, unit])
    windows = WINDOWS_N30 if name == "T-n30" else (T,)
    return Y, m, np.asfortranarray(Th), windows, unit


def _truth_job(job):
    m, Y, theta, space, windows = job
    return TR.smooth_mp_windows(m, Y, theta, space, windows)


def make_case(pool, name):
    Y, m, Th, windows, unit = case_inputs(name)
    B = Th.shape[1]
    Thc = np.asfortranarray(np.stack([transform_params(KIND_TVL, Th[:, b]) for b in range(B)], axis=1))
    for b in range(B):
        for n in windows:
            ll = O.loglik(O.KIND_TVL, m, 4, Y[:, :n], Th[:, b], 0)
            assert np.isfinite(ll), (name, b, n, ll)
    jobs = [(m, Y, (Th if sp == 0 else Thc)[:, b], sp, windows) for sp in (0, 1) for b in range(B)]
    truth = pool.map(_truth_job, jobs)
    out = dict(Y=Y, maturities=m, Theta=Th, Theta_c=Thc, windows=np.asarray(windows, dtype=np.int64),
               unit_root=np.int64(unit))
    for wi, n in enumerate(windows):
        chk = [TR.smooth_dense(m, Y, Th[:, b], 0, n) for b in range(B)]
        chk1 = [TR.smooth_dense(m, Y, Thc[:, b], 1, n) for b in range(B)]
        tr0 = [truth[b][wi] for b in range(B)]
        tr1 = [truth[B + b][wi] for b in range(B)]
        for b in range(B):
            for k, what in enumerate(("beta", "V", "C")):
                for sp, c, t in ((0, chk[b][k], tr0[b][k]), (1, chk1[b][k], tr1[b][k])):
                    e = TR.traj_err(c, t, t)
                    print(f"{name} n={n} b={b} space={sp} {what}: checker vs truth {e:.2e}", flush=True)
                    assert b == unit or e <= GEN_REL, (name, n, b, sp, what, e)
        st = lambda xs, k: np.stack([x[k] for x in xs], axis=-1)  # noqa: E731
        pre = f"w{n}_"
        out[pre + "beta_chk"] = st(chk, 0)
        out[pre + "Vu_chk"] = pack_upper(st(chk, 1))
        out[pre + "C_chk"] = st(chk, 2)
        out[pre + "beta_d0"] = (st(tr0, 0) - st(chk, 0)).astype(np.float32)
        out[pre + "Vu_d0"] = pack_upper(st(tr0, 1) - st(chk, 1)).astype(np.float32)
        out[pre + "C_d0"] = (st(tr0, 2) - st(chk, 2)).astype(np.float32)
        out[pre + "beta_d1"] = (st(tr1, 0) - st(tr0, 0)).astype(np.float32)
        out[pre + "Vu_d1"] = pack_upper(st(tr1, 1) - st(tr0, 1)).astype(np.float32)
        out[pre + "C_d1"] = (st(tr1, 2) - st(tr0, 2)).astype(np.float32)
    return out


def load_cases(path=FILE) -> dict:
    """{case: {Y, maturities, Theta, Theta_c, unit_root, windows: {n: arrays}}}; per window beta / V / C of the checker
    (`*_chk`, unconstrained θ), the truth there (`*_tru`) and the truth at Theta_c (`*_tru1`), V unpacked."""
    with np.load(path, allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    cases = {}
    for key, v in flat.items():
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = v
    for name, c in cases.items():
        wins = {}
        for n in c["windows"]:
            pre = f"w{int(n)}_"
            w = dict(beta_chk=c[pre + "beta_chk"], V_chk=unpack_upper(c[pre + "Vu_chk"], 4), C_chk=c[pre + "C_chk"])
            w["beta_tru"] = w["beta_chk"] + c[pre + "beta_d0"].astype(np.float64)
            w["V_tru"] = w["V_chk"] + unpack_upper(c[pre + "Vu_d0"].astype(np.float64), 4)
            w["C_tru"] = w["C_chk"] + c[pre + "C_d0"].astype(np.float64)
            w["beta_tru1"] = w["beta_tru"] + c[pre + "beta_d1"].astype(np.float64)
            w["V_tru1"] = w["V_tru"] + unpack_upper(c[pre + "Vu_d1"].astype(np.float64), 4)
            w["C_tru1"] = w["C_tru"] + c[pre + "C_d1"].astype(np.float64)
            wins[int(n)] = w
        cases[name] = dict(Y=c["Y"], maturities=c["maturities"], Theta=c["Theta"], Theta_c=c["Theta_c"],
                           unit_root=int(c["unit_root"]), windows=wins)
    return cases


def main():
    t0 = time.time()
    flat = {}
    with mproc.Pool(16) as pool:
        for name in CASES:
            for k, v in make_case(pool, name).items():
                flat[f"{name}/{k}"] = v
            print(f"{name} done at {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(FILE, **flat)
    print(f"wrote {FILE} ({FILE.stat().st_size} bytes) in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
