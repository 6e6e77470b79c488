"""Generator of tests/golden/smooth/smooth_cases.npz: the fixed-interval smoother's reference arrays
(include/yfm.h yfm_smooth_batch), from tests/smoother_reference.py — the dense FP64 checker (N × N F_t, RTS gain) and the
same recursion in 40-digit mpmath as the truth.

Cases (the smallest shapes at which the kernel can still go wrong), candidates θ₀ + 0.02·N(0, I):

  S-E    DNS  N = 4,  T = 8
  S-nan  DNS  N = 6,  T = 12   column 1 missing, column 5 missing, one NaN entry in column 9, last column missing
  S-n30  DNS  N = 30, T = 70   crosses the forward kernel's 64-column chunk and the sweep's; the last candidate has a Φ
                               eigenvalue of 0.999, where V = P − PNP cancels; windows T_use ∈ {1, 2, 3, 64, 65, 69, 70}
  S-n33  DNS  N = 33, T = 20
  S-n64  DNS  N = 64, T = 20
  G-E    GNS5 N = 7,  T = 12   one missing column

Stored per case: Y, maturities, kind, Theta (unconstrained), Theta_c (its transform, for the constrained space) and, per
window n, the checker's β̂ (M × n × B), packed upper triangles of V (U × n × B) and C (M × M × (n − 1) × B) in float64
at the unconstrained θ; the truth as its float32 difference from the checker (the difference is ~1e-13 of an entry, so
the sum restores the truth rounded to FP64); and the constrained-space truth as its float32 difference from the
unconstrained one.  The constrained-space checker is cheap and is run by the tests themselves.

The generator asserts, for every ordinary candidate, array and space, that the checker is within 1e-10 of the truth
under the rule's measure (per-step normwise error against the truth's magnitude), which leaves the 1e-9 bar a decade of
margin from the reference alone.  The near-unit-root candidate is exempt from this assertion only.

Run from the repository root:  python tests/golden/smooth/make_smooth.py     # under a minute on 16 cores (it prints its own time)
"""
from __future__ import annotations

import multiprocessing as mproc
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
for p in (str(ROOT / "yieldfactormodels.jl_amd"), str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import smoother_reference as SR  # noqa: E402
from yfm_amd import KIND_DNS, KIND_GNS  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402
from yfm_amd.params import param_layout, transform_params, untransform_params  # noqa: E402

FILE = HERE / "smooth_cases.npz"
CASES = ("S-E", "S-nan", "S-n30", "S-n33", "S-n64", "G-E")
WINDOWS_N30 = (1, 2, 3, 64, 65, 69, 70)
GEN_REL = 1e-10
SCALE = 0.02


def maturities(N):
    """N maturities in months: the 30-maturity grid thinned, or extended by further 24-month steps."""
    m30 = S.maturities_30()
    if N <= 30:
        return m30[np.linspace(0, 29, N).round().astype(int)]
    return np.concatenate([m30, 360.0 + 24.0 * np.arange(1, N - 30 + 1)])


def unit_root_theta(kind, th):
    """θ with Φ's first row and column cleared but for Φ₁₁ = 0.999: an eigenvalue of exactly 0.999."""
    lay = param_layout(kind)
    tc = transform_params(kind, th)
    Phi = tc[lay.phi_offset:lay.phi_offset + lay.M * lay.M].reshape(lay.M, lay.M).copy()
    Phi[0, :] = 0.0
    Phi[:, 0] = 0.0
    Phi[0, 0] = 0.999
    tc[lay.phi_offset:lay.phi_offset + lay.M * lay.M] = Phi.reshape(-1)
    return untransform_params(kind, tc)


def case_inputs(name):
    """(kind, Y, maturities, Theta, windows, index of the near-unit-root candidate or −1)."""
    seed = 4100 + CASES.index(name)
    kind = KIND_GNS if name == "G-E" else KIND_DNS
    N, T, B = {"S-E": (4, 8, 3), "S-nan": (6, 12, 3), "S-n30": (30, 70, 2), "S-n33": (33, 20, 2),
               "S-n64": (64, 20, 2), "G-E": (7, 12, 3)}[name]
    m = maturities(N)
    if name == "G-E":
        # seven maturities that identify both decay rates: κ₁(Z'Z) ≈ 3e4 at these candidates.  The thinned grid gives
        # 6e7, past the 1e6 at which the forward launch defers a candidate — and a deferred candidate has no states
        m = np.array([3.0, 6.0, 18.0, 24.0, 60.0, 72.0, 360.0])
    Y = S.simulate_panel(kind, T, m, seed).copy()
    Th = S.theta_batch(kind, B, SCALE, seed + 50, bad_frac=0)
    unit = -1
    if name == "S-nan":  # 1-based columns 1, 5 and the last missing; one NaN entry in column 9
        Y[:, 0] = np.nan
        Y[:, 4] = np.nan
        Y[2, 8] = np.nan
        Y[:, T - 1] = np.nan
    if name == "G-E":
        Y[:, 6] = np.nan
    if name == "S-n30":
        unit = B - 1
        Th[:, unit] = unit_root_theta(kind, Th[:, unit])
    windows = WINDOWS_N30 if name == "S-n30" else (T,)
    return kind, Y, m, np.asfortranarray(Th), windows, unit


def _truth_job(job):
    kind, m, Y, theta, space, windows = job
    return [SR.smooth_mp(kind, m, Y, theta, space, n) for n in windows]


def pack_upper(V):
    iu = np.triu_indices(V.shape[0])
    return V[iu[0], iu[1]]


def unpack_upper(Vu, M):
    iu = np.triu_indices(M)
    V = np.empty((M, M) + Vu.shape[1:])
    V[iu[0], iu[1]] = Vu
    V[iu[1], iu[0]] = Vu
    return V


def make_case(pool, name):
    kind, Y, m, Th, windows, unit = case_inputs(name)
    B = Th.shape[1]
    Thc = np.asfortranarray(np.stack([transform_params(kind, Th[:, b]) for b in range(B)], axis=1))
    jobs = [(kind, m, Y, (Th if sp == 0 else Thc)[:, b], sp, windows) for sp in (0, 1) for b in range(B)]
    truth = pool.map(_truth_job, jobs)
    out = dict(kind=np.int64(kind), Y=Y, maturities=m, Theta=Th, Theta_c=Thc, windows=np.asarray(windows, dtype=np.int64),
               unit_root=np.int64(unit))
    for wi, n in enumerate(windows):
        chk = [SR.smooth_dense(kind, m, Y, Th[:, b], 0, n) for b in range(B)]
        chk1 = [SR.smooth_dense(kind, m, Y, Thc[:, b], 1, n) for b in range(B)]
        tr0 = [truth[b][wi] for b in range(B)]
        tr1 = [truth[B + b][wi] for b in range(B)]
        for b in range(B):
            for k, what in enumerate(("beta", "V", "C")):
                for sp, c, t in ((0, chk[b][k], tr0[b][k]), (1, chk1[b][k], tr1[b][k])):
                    e = SR.traj_err(c, t, t)
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
    """{case: {kind, Y, maturities, Theta, Theta_c, unit_root, windows: {n: arrays}}}; per window beta / V / C of the
    checker (`*_chk`, unconstrained θ), the truth there (`*_tru`) and the truth at Theta_c (`*_tru1`), V unpacked."""
    with np.load(path, allow_pickle=False) as z:
        flat = {k: z[k] for k in z.files}
    cases = {}
    for key, v in flat.items():
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = v
    for name, c in cases.items():
        M = SR.STATE_DIM[int(c["kind"])]
        wins = {}
        for n in c["windows"]:
            pre = f"w{int(n)}_"
            w = dict(beta_chk=c[pre + "beta_chk"], V_chk=unpack_upper(c[pre + "Vu_chk"], M), C_chk=c[pre + "C_chk"])
            w["beta_tru"] = w["beta_chk"] + c[pre + "beta_d0"].astype(np.float64)
            w["V_tru"] = w["V_chk"] + unpack_upper(c[pre + "Vu_d0"].astype(np.float64), M)
            w["C_tru"] = w["C_chk"] + c[pre + "C_d0"].astype(np.float64)
            w["beta_tru1"] = w["beta_tru"] + c[pre + "beta_d1"].astype(np.float64)
            w["V_tru1"] = w["V_tru"] + unpack_upper(c[pre + "Vu_d1"].astype(np.float64), M)
            w["C_tru1"] = w["C_tru"] + c[pre + "C_d1"].astype(np.float64)
            wins[int(n)] = w
        cases[name] = dict(kind=int(c["kind"]), Y=c["Y"], maturities=c["maturities"], Theta=c["Theta"],
                           Theta_c=c["Theta_c"], unit_root=int(c["unit_root"]), windows=wins)
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
