"""Writes msedn_cases.npz — the recorded values of the neural models' checker (tests/msedn_reference.py) that the
tests would otherwise pay for at run time — and defines the cases themselves (maturities, panels, θ batches), which
are regenerated from the seeded generators of yfm_amd.synthetic and pinned by a checksum in the file.

    python tests/golden/msedn/make_msedn.py        (about three minutes on 8 cores)

Contents:
* ``float_<kind>_<N>_<T>_<space>``  get_loss of the Float64 restatement for every parity candidate: all 26 kinds at
  N ∈ {4, 30}, T = 40, 70 candidates; the six representative kinds at N ∈ {4, 5, 30, 33, 90}, T ∈ {8, 40}, 300
  candidates; both parameter spaces.  Every value is finite (checked here).
* ``truth_<kind>_<N>_<T>_<space>``  the 40-digit value of the first N_TRUTH candidates of the T = 40, space-0 cases.
  (All of them would take ten hours; the GPU tests compute a truth only where the parity rule's second clause asks.)
* ``host_*``  the host check's cases: 10 switch combinations over the three duplicator forms × N ∈ {4, 5, 30, 33} on a
  panel with a NaN column and one with a NaN first column, with the restatement's losses.
* ``score_*``  γ, β, y and the 40-digit score for N ∈ {4, 5, 30}, both transforms.
* ``tryinit_*``  the restatement's sequential try_initializations walk for 1SD-NNS and 1RWSD-NNS on two windows.

θ comes from theta_batch(kind, POOL, seed = 700 + kind, bad_frac = 0, a_range = (1e-5, 1e-4)).  Two things keep the
1e-9 parity rule a statement about the kernel and not about the restatement's own rounding, both decided by the
restatement alone:
* the step sizes: over 1e-5 … 1e-4 the Float64 restatement's own error against the 40-digit truth stays below
  1e-12 at every N used here (measured when these cases were chosen: N = 90, kinds 32 / 37 / 42 / 46, worst 3.1e-13;
  over 1e-4 … 1e-3 it reaches 2.2e-7 there);
* a screen for candidates whose loadings amplify rounding (``sel_<kind>``).  The Z₂ transform divides by
  u = raw₁ − raw_{n−1} + 1e-7, and about 0.7 % of random networks put the two anchors so close that t = (raw − raw_{n−1})/u
  reaches 1e4 … 1e9: the loss then is 1e3 … 1e15 and the Float64 restatement itself is up to 1e-6 from the truth
  (3SD-NNS, N = 4, pool candidate 32: restatement −1893264248817752.8, truth −1893265879158424.8), so neither clause
  of the rule can tell a right kernel from a wrong one there.  Every pool candidate is therefore evaluated twice by
  the Float64 restatement, on the panel and on the panel with every entry moved by a relative 1e-12, in every
  (N, T) case of its kind; the batch is the first 300 (70) candidates whose loss moves by no more than
  AMP_MAX × 1e-12 relative in all of them.  The screen never sees the code under test.
"""
from __future__ import annotations

import hashlib
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

import msedn_reference as R  # noqa: E402
from yfm_amd import params as P  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "msedn_cases.npz"
A_RANGE = (1e-5, 1e-4)
POOL_EXTRA = 1.25    # pool = 1.25 × the batch
PERTURB = 1e-12      # relative panel perturbation of the conditioning screen
AMP_MAX = 1e3        # largest amplification kept: Float64 rounding (1e-16) then stays below 1e-12 of the loss
N_TRUTH = 2
ALL_KINDS = tuple(R.all_kinds())
REP_KINDS = (R.KIND_NNS, R.KIND_NNS_ANCHORED, R.sd_kind(0), R.sd_kind(1, True), R.sd_kind(2, False, True),
             R.sd_kind(2, True, True, True))  # NNS, NNS-Anchored, 1SD-NNS, 2RWSD-NNS, 3SSD-NNS, 3SRWSD-NNS-Anchored
REP_N = (4, 5, 30, 33, 90)
REP_T = (8, 40)
# host check: 2 static and 8 score-driven switch combinations, the duplicator form cycling through all three
HOST_KINDS = (R.KIND_NNS, R.KIND_NNS_ANCHORED) + tuple(
    R.sd_kind(i % 3, bool(i & 1), bool(i & 2), bool(i & 4)) for i in range(8))
HOST_N = (4, 5, 30, 33)
HOST_T = 10
SCORE_N = (4, 5, 30)
TRYINIT_KINDS = (R.sd_kind(0), R.sd_kind(0, True))
TRYINIT_N, TRYINIT_T, TRYINIT_WINDOWS = 5, 24, (24, 16)
# The winner of the walk must be the restatement's, so it has to lead by more than rounding.  From θ₀ it does not:
# the smallest A wins, γ then stays at ω, B does not matter and the trials tie to 1e-15.  Panel seed and start (pool
# candidate 1 of the kind) were searched with the restatement alone for a lead ≥ TRYINIT_LEAD in both windows of both
# kinds (seeds 11 … 30: 23 is the only one for 1RWSD-NNS; 1SD-NNS: trial 252 by 1.6e-6 and 2.7e-6)
TRYINIT_SEED, TRYINIT_START, TRYINIT_LEAD = 23, 1, 1e-8


def mats_for(N):
    if N == 4:
        return np.array([3.0, 12.0, 60.0, 120.0])
    if N == 30:
        return S.maturities_30()
    return np.arange(1, N + 1) * float(360 // N)


_panels, _thetas = {}, {}


def panel_for(N, T):
    if (N, T) not in _panels:
        _panels[(N, T)] = S.simulate_panel(P.KIND_NNS, T, maturities=mats_for(N))
    return _panels[(N, T)]


def batch_size(kind):
    return 300 if kind in REP_KINDS else 70


def kind_grid(kind):
    """The (N, T) cases of a kind."""
    return [(N, T) for N in REP_N for T in REP_T] if kind in REP_KINDS else [(4, 40), (30, 40)]


def pool_for(kind):
    """The candidates the screen chooses from (unconstrained)."""
    if ("pool", kind) not in _thetas:
        _thetas[("pool", kind)] = S.theta_batch(kind, int(batch_size(kind) * POOL_EXTRA), scale=0.1, seed=700 + kind,
                                                bad_frac=0.0, a_range=A_RANGE)
    return _thetas[("pool", kind)]


def perturbed(Y):
    """Every entry moved by a relative PERTURB, signs alternating."""
    sign = np.where((np.arange(Y.size) % 2 == 0), 1.0, -1.0).reshape(Y.shape, order="F")
    return np.asfortranarray(Y * (1.0 + PERTURB * sign))


_selection = {}


def theta_for(kind, space):
    """The kind's batch (300 candidates, 70 outside the representative kinds): the screened pool candidates, in pool
    order; space 1: their constrained images."""
    if (kind, space) not in _thetas:
        sel = _selection[kind] if kind in _selection else load_cases(check=False)[f"sel_{kind}"]
        Th = np.asfortranarray(pool_for(kind)[:, sel])
        _thetas[(kind, 0)] = Th
        _thetas[(kind, 1)] = np.asfortranarray(P.transform_params(kind, Th))
    return _thetas[(kind, space)]


def parity_cases():
    """(kind, N, T, space) → number of candidates."""
    cases = {}
    for kind in ALL_KINDS:
        for N, T in kind_grid(kind):
            for space in (0, 1):
                cases[(kind, N, T, space)] = batch_size(kind)
    return cases


def host_panels(N):
    """The host check's two panels: a NaN column mid-panel, and a NaN first column."""
    Y = S.simulate_panel(P.KIND_NNS, HOST_T, maturities=mats_for(N), seed=7)
    mid, first = Y.copy(order="F"), Y.copy(order="F")
    mid[:, 4] = np.nan
    first[:, 0] = np.nan
    return mid, first


def host_theta(kind):
    return S.theta_batch(kind, 3, scale=0.1, seed=900 + kind, bad_frac=0.0, a_range=A_RANGE)


def tryinit_panel():
    return S.simulate_panel(P.KIND_NNS, TRYINIT_T, maturities=mats_for(TRYINIT_N), seed=TRYINIT_SEED)


def tryinit_start(kind):
    return P.transform_params(kind, pool_for(kind)[:, TRYINIT_START])


def checksum():
    """The inputs the recorded values belong to: θ batches, panels and maturities, hashed."""
    h = hashlib.sha256()
    for kind in ALL_KINDS:
        h.update(np.ascontiguousarray(theta_for(kind, 0)).tobytes())
    for N in REP_N:
        for T in REP_T:
            h.update(np.ascontiguousarray(panel_for(N, T)).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _screen_job(a):
    kind, N, T, b = a
    th = pool_for(kind)[:, b]
    Y = panel_for(N, T)
    f = R.get_loss(kind, mats_for(N), Y, th, 0, R.FLOAT)
    fp = R.get_loss(kind, mats_for(N), perturbed(Y), th, 0, R.FLOAT)
    return f, fp


def _float_job(a):
    kind, N, T, space, b = a
    return R.get_loss(kind, mats_for(N), panel_for(N, T), theta_for(kind, space)[:, b], space, R.FLOAT)


def _truth_job(a):
    kind, N, T, space, b = a
    return R.get_loss(kind, mats_for(N), panel_for(N, T), theta_for(kind, space)[:, b], space, R.TRUTH)


def _host_job(a):
    kind, N, which, space, b = a
    Th = host_theta(kind)
    th = Th[:, b] if space == 0 else P.transform_params(kind, Th[:, b])
    return R.get_loss(kind, mats_for(N), host_panels(N)[which], th, space, R.FLOAT)


def _tryinit_job(a):
    kind, w = a
    start = tryinit_start(kind)
    mats, Y = mats_for(TRYINIT_N), tryinit_panel()
    losses = [-R.get_loss(kind, mats, Y, start, 1, R.FLOAT, w)]
    trial, k = start.copy(), 1
    while True:
        p = R.trial_params(kind, trial, k)
        if p is None:
            break
        trial = p
        losses.append(-R.get_loss(kind, mats, Y, p, 1, R.FLOAT, w))
        k += 1
    return np.array(losses)


def score_case(N, anchored):
    """γ, β (the OLS fit at γ), y and the 40-digit score of 3SD-NNS[-Anchored] at candidate 0."""
    import mpmath as mp
    kind = R.sd_kind(2, anchored=anchored)
    mats = mats_for(N)
    th = P.transform_params(kind, theta_for(kind, 0)[:, 0])
    y = panel_for(N, 8)[:, 0]
    with mp.workdps(R.TRUTH.digits):
        m = R.set_params(kind, th, mats, R.TRUTH)
        yy = R._data(y[:, None], R.TRUTH)[:, 0]
        beta = R.get_beta_ols(m, yy)
        g = R.score(m, m.gamma, beta, yy)
        return R.TRUTH.to_float(m.gamma), R.TRUTH.to_float(beta), y, R.TRUTH.to_float(g)


def build():
    out = {}
    cases = parity_cases()
    with Pool() as pool:
        # the screen: space 0, every pool candidate, on the panel and on the perturbed panel
        sjobs = [(k, N, T, b) for k in ALL_KINDS for (N, T) in kind_grid(k) for b in range(pool_for(k).shape[1])]
        svals = dict(zip(sjobs, pool.map(_screen_job, sjobs, chunksize=16)))
        kept_out = 0
        for k in ALL_KINDS:
            nb = pool_for(k).shape[1]
            amp = np.zeros(nb)
            for (N, T) in kind_grid(k):
                f = np.array([svals[(k, N, T, b)][0] for b in range(nb)])
                fp = np.array([svals[(k, N, T, b)][1] for b in range(nb)])
                with np.errstate(all="ignore"):
                    a = np.abs(fp - f) / np.abs(f) / PERTURB
                amp = np.maximum(amp, np.where(np.isfinite(a), a, np.inf))
            good = np.flatnonzero(amp <= AMP_MAX)
            assert good.size >= batch_size(k), ("pool too small for kind", k, good.size)
            sel = good[:batch_size(k)]
            kept_out += int(sel[-1] + 1 - sel.size)
            _selection[k] = out[f"sel_{k}"] = sel.astype(np.int32)
            for (N, T) in kind_grid(k):  # the screen's unperturbed run is the space-0 reference
                v = np.array([svals[(k, N, T, int(b))][0] for b in sel])
                assert np.all(np.isfinite(v)), ("the restatement must be finite on every parity candidate", k, N, T)
                out[f"float_{k}_{N}_{T}_0"] = v
    print("screened out", kept_out, "pool candidates ahead of the kept ones")
    out["checksum"] = checksum()
    with Pool() as pool:  # forked now: the workers see the selection
        jobs =[(k, N, T, sp, b) for (k, N, T, sp), n in cases.items() if sp == 1 for b in range(n)]
        vals = pool.map(_float_job, jobs, chunksize=16)
        pos = 0
        for (k, N, T, sp), n in cases.items():
            if sp != 1:
                continue
            v = np.array(vals[pos:pos + n])
            pos += n
            assert np.all(np.isfinite(v)), ("the restatement must be finite on every parity candidate", k, N, T, sp)
            out[f"float_{k}_{N}_{T}_{sp}"] = v
        tcases = [c for c in cases if c[2] == 40 and c[3] == 0]
        tvals = pool.map(_truth_job, [c + (b,) for c in tcases for b in range(N_TRUTH)], chunksize=1)
        for i, (k, N, T, sp) in enumerate(tcases):
            out[f"truth_{k}_{N}_{T}_{sp}"] = np.array(tvals[i * N_TRUTH:(i + 1) * N_TRUTH])
        hjobs = [(k, N, w, sp, b) for k in HOST_KINDS for N in HOST_N for w in (0, 1) for sp in (0, 1) for b in range(3)]
        hvals = pool.map(_host_job, hjobs, chunksize=4)
        for i in range(0, len(hjobs), 3):
            k, N, w, sp, _ = hjobs[i]
            out[f"host_{k}_{N}_{w}_{sp}"] = np.array(hvals[i:i + 3])
        tjobs = [(k, w) for k in TRYINIT_KINDS for w in TRYINIT_WINDOWS]
        for (k, w), v in zip(tjobs, pool.map(_tryinit_job, tjobs, chunksize=1)):
            order = np.argsort(v)
            assert np.all(np.isfinite(v)) and (v[order[1]] - v[order[0]]) >= TRYINIT_LEAD * abs(v[order[0]]), (k, w)
            out[f"tryinit_{k}_{w}"] = v
    for N in SCORE_N:
        for anchored in (False, True):
            gam, beta, y, g = score_case(N, anchored)
            tag = f"{N}_{int(anchored)}"
            out[f"score_gamma_{tag}"], out[f"score_beta_{tag}"], out[f"score_y_{tag}"], out[f"score_g_{tag}"] = gam, beta, y, g
    return out


_loaded = None


_checked = False


def load_cases(check=True):
    """The recorded values; raises if the seeded inputs no longer are the ones they were computed for."""
    global _loaded, _checked
    if _loaded is None:
        with np.load(FILE) as z:
            _loaded = {k: z[k] for k in z.files}
    if check and not _checked:
        if not np.array_equal(_loaded["checksum"], checksum()):
            raise RuntimeError("tests/golden/msedn/msedn_cases.npz was made for other θ batches or panels: rerun "
                               "tests/golden/msedn/make_msedn.py")
        _checked = True
    return _loaded


if __name__ == "__main__":
    np.savez_compressed(FILE, **build())
    _loaded = None
    c = load_cases()
    worst = 0.0
    for k in sorted(c):
        if k.startswith("truth_"):
            f = c["float_" + k[6:]][:N_TRUTH]
            worst = max(worst, float(np.max(np.abs(f - c[k]) / np.abs(c[k]))))
    print("entries", len(c), "bytes", FILE.stat().st_size, "worst FLOAT-to-TRUTH gap on the recorded truths", worst)
