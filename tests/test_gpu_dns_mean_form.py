"""The DNS mean update that reads G⁻¹ directly (csrc/yfm_fixedz.hpp: collapsed_innov — ĉ₁, ĉ₂ from G⁻¹ and z̃,
c₀ = ȳ − β₀ + G⁻¹₀·z̃ as one fma chain: 45 FP64 operations per steady step instead of 48), in every
kernel that shares it.

B = 200 (three waves and a partial one of 8 lanes), T = 100 (the steady instantiation: T ≥ 80).  N = 8, 24 (their own
widths), 25 and 30 (both ends of NP = 30), 32 (NP = 32), 33 (NP = 48: Z'ỹ on the VALU), 65 (the lane-group kernel).
Both parameter spaces; a clean panel and one with NaN columns and ragged windows.  Yields in units of 4 % (UNIT below:
an exact rescaling that keeps every loglik away from zero, where the relative steady-vs-full gate has no meaning).

Gates per case: the dense oracle's NaN / −Inf pattern and factor-1 parity adjudicated by the binary128 truth
(`assert_parity`); the steady state against the full recursion (YFM_DNS_STEADY=0) ≤ 1e-12 with a non-empty
bitwise-equal share (the two are one expression: a frozen lane's steady step is bitwise its full step); where the
two-wave kernel exists (N ≤ 32) it agrees with the per-lane kernel bit for bit.  Trajectory mode (the RECORD
instantiations) against the NumPy oracle with tests/test_gpu_predict.py's tolerance.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle.truth import loglik_oracle, loglik_truth
from test_gpu_parity import assert_parity
from test_gpu_predict import KEYS, O, assert_close, oracle_state
from test_gpu_split import both
from test_gpu_steady_sweep import full
from yfm_amd import KIND_DNS
from yfm_amd import synthetic as S
from yfm_amd.params import param_layout, transform_params, untransform_params

pytestmark = pytest.mark.gpu

B, T = 200, 100
NS = (8, 24, 25, 30, 32, 33, 65)
PATTERNS = ("clean", "nan+ragged")
CASES = [(N, sp, pat) for N in NS for sp in (0, 1) for pat in PATTERNS]
SPLIT_MAX_N = 32  # dns_split_supported: NP ∈ {8, 16, 24, 30, 32}
# The steady-vs-full gate is relative to |loglik| with no floor, and a steady and a full launch may differ by one
# ulp of Σq (≈ 1e-13 at Σq ≈ 10³): on the synthetic panel in percent an N = 8 loglik is a sum of terms of either
# sign that lands anywhere in −30 … 40, and a candidate that cancels to |ll| < 0.1 reads 1e-12 and more on the
# parent build and this one alike (measured: |ll| = 0.074 → 1.5e-12 on both; |ll| = 0.0093 → 6.1e-12).  The cases
# therefore measure yields in units of 4 %: Y, δ and U times 1/4, σ² times 1/16 — a power of two, so every product
# and sum of the filter is the same bits scaled, and only the log-determinant terms move: each loglik by
# (T_b − 2)·N·log 4 ≥ 343, away from zero.
UNIT = 0.25


def maturities(N):
    """N points of the 30-maturity grid spread over its whole range (the short end alone makes Z'Z
    ill-conditioned: the grid's first 8 points put the dense oracle itself 1e-9 from the kernels' trajectories);
    past 30, N points evenly over 3 … 360 months."""
    if N <= 30:
        return S.maturities_30()[np.round(np.linspace(0, 29, N)).astype(int)].copy()
    return np.linspace(3.0, 360.0, N)


def make_case(N, space, pattern):
    seed = 1000 * N + space
    mats = maturities(N)
    Y = S.simulate_panel(KIND_DNS, T, maturities=mats, seed=seed).copy(order="F")
    lay = param_layout(KIND_DNS)
    thc = transform_params(KIND_DNS, S.theta_batch(KIND_DNS, B, seed=seed + 1, bad_frac=0.02))
    Y *= UNIT
    thc[lay.base_offset] *= UNIT * UNIT
    thc[lay.u_offset:lay.delta_offset + lay.M] *= UNIT  # U (Q = U'U) and δ
    Th = np.asfortranarray(thc if space == 1 else untransform_params(KIND_DNS, thc))
    T_use = None
    if pattern != "clean":
        Y[:, [37, 48]] = np.nan  # mid-block after the waves froze, and a block's first step: the lanes thaw
        T_use = np.full(B, T, dtype=np.int32)
        T_use[B - 1] = T // 2  # the partial wave's mirror candidate
        T_use[70] = T // 3     # one lane of the second wave
        T_use[150:160] = np.random.default_rng(seed).integers(T // 2, T + 1, 10)
    return mats, Y, Th, T_use


_REF = {}


def reference(case):
    """(dense oracle, binary128 truth) of a case, computed once."""
    if case not in _REF:
        N, space, pattern = case
        mats, Y, Th, T_use = make_case(*case)
        _REF[case] = (loglik_oracle(KIND_DNS, Y, mats, Th, space=space, T_use=T_use),
                      loglik_truth(KIND_DNS, Y, mats, Th, space=space, T_use=T_use))
    return _REF[case]


def same_pattern(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c[0]}-space{c[1]}-{c[2]}")
def test_mean_form_parity_steady_split(engine, case):
    N, space, pattern = case
    mats, Y, Th, T_use = make_case(*case)
    orc, tru = reference(case)
    assert np.isfinite(orc).mean() >= 0.9, np.isfinite(orc).mean()  # the gates below must have something to check
    engine.set_panel(Y, mats)
    run = lambda: engine.loglik(KIND_DNS, Th, space=space, T_use=T_use)  # noqa: E731
    got = run()
    steady_ws = engine.last_steady()
    # the instantiation the case is meant to run: NP > 32 and the lane-group kernel have no steady state; on the
    # config-2 class of grids (24 maturities and up) the waves freeze well inside T = 100 (N = 8 freezes later:
    # its R = σ²(Z'Z)⁻¹ is larger and the Riccati recursion slower; its share is printed)
    if N > 32:
        assert steady_ws == 0, (N, steady_ws)
    elif N >= 24:
        assert steady_ws > 0, (N, steady_ws)
    tab = assert_parity(got, orc, tru)
    # steady vs the full recursion
    ref_full = full(run)
    assert same_pattern(got, ref_full)
    fin = np.isfinite(ref_full)
    d_full = np.abs(got[fin] - ref_full[fin]) / np.maximum(np.abs(ref_full[fin]), 1e-300)
    share = float(np.mean(got[fin] == ref_full[fin]))
    print(f"mean form N {N} space {space} {pattern:10s}: finite {int(fin.sum())}/{B}, steady wave-steps {steady_ws}, "
          f"vs full max rel {d_full.max():.2e}, bitwise share {share:.3f}, gpu vs truth "
          f"{tab['gpu_vs_truth_max_rel']:.2e} (oracle {tab['oracle_vs_truth_max_rel']:.2e}), within 1e-9 "
          f"{tab['within_1e-9']}, adjudicated {tab['adjudicated']}")
    assert d_full.max() <= 1e-12, d_full.max()
    assert share > 0.0
    # the two-wave kernel: the same bits as the per-lane kernel's full recursion
    if N <= SPLIT_MAX_N:
        a, b = both(run)
        np.testing.assert_array_equal(a, ref_full)
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("N", NS)
def test_mean_form_trajectory_vs_oracle(engine, N):
    """predict (RECORD instantiations: per-lane MFMA, per-lane VALU, lane group) at T = 100, 4 candidates, horizon 3,
    normwise 1e-9 per array against the NumPy oracle."""
    mats = maturities(N)
    h, nb = 3, 4
    Y = S.simulate_panel(KIND_DNS, T, maturities=mats, seed=500 + N).copy(order="F")
    Th = transform_params(KIND_DNS, S.theta_batch(KIND_DNS, nb, seed=600 + N, bad_frac=0.0, scale=0.05))
    engine.set_panel(Y, mats)
    r = engine.predict(KIND_DNS, Th, space=1, horizon=h)
    n = T + h - 1
    for b in range(nb):
        ref = O.predict(oracle_state(KIND_DNS, mats, Th[:, b]), O.pad_nan(Y, h))
        for k in KEYS:
            assert_close(r[k][:, :n, b], ref[k], what=(k, b))
