"""DNS at NP = 30 with the last maturity eliminated: Z'ỹ on 7 MFMA k-steps (`ktrim_*` in
csrc/yfm_fixedz.hpp).

The kernel forms z̃ = Σ_{i<N−1} (Zᵢ − Z_{N−1}) ỹᵢ — slots 0..27 on the matrix cores, slot 28 as one fma per loading
column on the VALU — and neglects Z_{N−1}·Σᵢỹᵢ (the centring's rounding residual).  N = 25, 28, 29, 30 reach the
runtime index of the eliminated maturity in its sub-cases: no elimination needed (N ≤ 28), slot 28 empty (N = 29),
slot 28 on the VALU (N = 30).  T = 100 runs the steady instantiation, T = 40 the full-recursion one (T < 80).

Gates per case (the project's own rules): the NaN / −Inf pattern of the dense oracle; within 1e-9 of the oracle, or
no further from the binary128 truth than the oracle is (`parity_adjudicated`); steady vs `YFM_DNS_STEADY=0` ≤ 1e-12.
`YFM_DNS_KTRIM=0` (the 8-k-step instantiations) passes the same gates with the same non-finite pattern; the largest
relative difference between the two is printed, not gated — what bounds it is the truth adjudication.  Every case
requires ≥ 90% of its candidates to have a finite oracle loglik.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from oracle.truth import loglik_oracle, loglik_truth
from test_gpu_predict import KEYS, O, assert_close, oracle_state
from test_gpu_steady_sweep import full, parity_adjudicated
from yfm_amd import KIND_DNS
from yfm_amd import synthetic as S
from yfm_amd.params import transform_params

pytestmark = pytest.mark.gpu

B = 200  # three full waves and a partial one of 8 lanes
NS = (30, 25, 28, 29)
TS = (100, 40)
PATTERNS = ("clean", "nan+ragged")
CASES = [(N, T, sp, pat) for N in NS for T in TS for sp in (0, 1) for pat in PATTERNS]


def untrimmed(fn):
    os.environ["YFM_DNS_KTRIM"] = "0"
    try:
        return fn()
    finally:
        os.environ.pop("YFM_DNS_KTRIM", None)


def nan_columns(T):
    """One NaN column mid-block after every wave has frozen (the config-2 class freezes by step 14) and one at a
    block's first step (a multiple of 16)."""
    return (37, 48) if T == 100 else (21, 32)


def make_case(N, T, space, pattern):
    seed = 100 * N + T + space
    mats = S.maturities_30()[:N].copy()
    Y = S.simulate_panel(KIND_DNS, T, maturities=mats, seed=seed).copy(order="F")
    Th = S.theta_batch(KIND_DNS, B, seed=seed + 1, bad_frac=0.02)
    if space == 1:
        Th = np.asfortranarray(transform_params(KIND_DNS, Th))
    T_use = None
    if pattern != "clean":
        Y[:, list(nan_columns(T))] = np.nan
        T_use = np.full(B, T, dtype=np.int32)
        T_use[B - 1] = T // 2  # the partial wave's mirror candidate
        T_use[70] = T // 3     # one lane of the second wave
        T_use[150:160] = np.random.default_rng(seed).integers(T // 2, T + 1, 10)
    return mats, Y, Th, T_use


_REF = {}


def reference(case):
    """(dense oracle, binary128 truth) of a case, computed once."""
    if case not in _REF:
        N, T, space, pattern = case
        mats, Y, Th, T_use = make_case(*case)
        _REF[case] = (loglik_oracle(KIND_DNS, Y, mats, Th, space=space, T_use=T_use),
                      loglik_truth(KIND_DNS, Y, mats, Th, space=space, T_use=T_use))
    return _REF[case]


def same_pattern(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))


def max_rel(a, b):
    fin = np.isfinite(a) & np.isfinite(b)
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300))) if fin.any() else 0.0


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"N{c[0]}-T{c[1]}-space{c[2]}-{c[3]}")
def test_ktrim_parity(engine, case):
    N, T, space, pattern = case
    mats, Y, Th, T_use = make_case(*case)
    orc, tru = reference(case)
    assert np.isfinite(orc).mean() >= 0.9, np.isfinite(orc).mean()  # the gates below must have something to check
    engine.set_panel(Y, mats)
    run = lambda: engine.loglik(KIND_DNS, Th, space=space, T_use=T_use)  # noqa: E731
    got = run()
    steady_ws = engine.last_steady()
    assert (steady_ws > 0) == (T >= 80), (T, steady_ws)  # the instantiation the case is meant to run
    # the oracle's NaN / −Inf pattern and factor-1 parity
    assert same_pattern(got, orc)
    tab = parity_adjudicated(got, orc, tru)
    # steady vs the full recursion
    ref_full = full(run)
    assert same_pattern(got, ref_full)
    d_full = max_rel(got, ref_full)
    # the 8-k-step instantiation: same non-finite pattern, same gates
    got8 = untrimmed(run)
    assert same_pattern(got, got8) and same_pattern(got8, orc)
    tab8 = parity_adjudicated(got8, orc, tru)
    d8_full = max_rel(got8, untrimmed(lambda: full(run)))
    d_trim = max_rel(got, got8)
    print(f"ktrim N {N} T {T} space {space} {pattern:10s}: finite {int(np.isfinite(orc).sum())}/{B}, steady wave-steps "
          f"{steady_ws}, vs full {d_full:.2e} (untrimmed {d8_full:.2e}), trimmed vs untrimmed max rel {d_trim:.3e}, "
          f"gpu vs truth {tab['gpu_vs_truth_max_rel']:.2e} (untrimmed {tab8['gpu_vs_truth_max_rel']:.2e}, oracle "
          f"{tab['oracle_vs_truth_max_rel']:.2e})")
    assert d_full <= 1e-12, d_full
    assert d8_full <= 1e-12, d8_full


@pytest.mark.parametrize("N", [25, 28, 29])
def test_ktrim_split_kernel_bitwise(engine, N):
    """The two-wave kernel (YFM_DNS_SPLIT=1) shares the trimmed fragments and the VALU term: bitwise the per-lane
    kernel at the widths of NP = 30 that tests/test_gpu_split.py does not visit (it has N = 30), trimmed and
    untrimmed, on the NaN + ragged panel."""
    from test_gpu_split import both
    mats, Y, Th, T_use = make_case(N, 40, 0, "nan+ragged")
    engine.set_panel(Y, mats)
    run = lambda: engine.loglik(KIND_DNS, Th, T_use=T_use)  # noqa: E731
    a, b = both(run)
    np.testing.assert_array_equal(a, b)
    a8, b8 = untrimmed(lambda: both(run))
    np.testing.assert_array_equal(a8, b8)


def test_ktrim_predict_vs_oracle(engine):
    """Trajectory mode (the RECORD instantiation) at N = 30, B = 8, T = 40 against the NumPy oracle, with
    tests/test_gpu_predict.py's tolerance (1e-9 normwise per array); the untrimmed instantiation likewise."""
    mats = S.maturities_30()
    T, h, nb = 40, 3, 8
    Y = S.simulate_panel(KIND_DNS, T, maturities=mats, seed=77).copy(order="F")
    Th = transform_params(KIND_DNS, S.theta_batch(KIND_DNS, nb, seed=78, bad_frac=0.0, scale=0.05))
    engine.set_panel(Y, mats)
    run = lambda: engine.predict(KIND_DNS, Th, space=1, horizon=h)  # noqa: E731
    r, r8 = run(), untrimmed(run)
    n = T + h - 1
    for b in range(nb):
        ref = O.predict(oracle_state(KIND_DNS, mats, Th[:, b]), O.pad_nan(Y, h))
        for k in KEYS:
            assert_close(r[k][:, :n, b], ref[k], what=(k, b))
            assert_close(r8[k][:, :n, b], ref[k], what=(k, b, "untrimmed"))
