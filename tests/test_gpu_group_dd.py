"""Every instantiation of the two kernels that serve the fixed-loading models at N > 64 — the lane-group kernel
fixedz_group_kernel<L, M, LEAD, RECORD> (yfm_group.hip) and the double-double kernel of the candidates it defers,
fixedz_dd_loglik_kernel<L, M, LEAD, RECORD> (yfm_fixedz_dd.hip) — on a fixed list of shapes (DESIGN.md §3.1b holds
the table of instantiations and the test that runs each):

* the loglik at both ends of every L's range of N (DNS: 16 maturities per lane, GNS5: 8; at N = MPL·L every lane owns
  all its slots, at N = MPL·L/2 + 1 half the slots of most lanes are empty), N = 1016 and 1024 (two- and one-column
  chunks of the group kernel), each batch half collapsed (FP64) and half deferred (double-double);
* missing columns on either side of a chunk hand-over of either kernel, and windows that end on or next to one;
* the trajectories (RECORD) of filter_states and predict at one N per lane count (N = 64 … 513), deferred candidates
  included;
* a deferral list longer than one pass of the double-double kernel's 256-block grid (its grid-stride loop's second
  trip);
* the refusal above the largest N (DNS 1024, GNS5 512), after which the context still serves.

Inputs of every case: mats = (1 … N)·360/N, the panel simulated on them, θ = theta_batch(seed = 71 + N, scale 0.05).
The first half of a batch is left as drawn (κ₁(Z'Z) < 5e5: the FP64 collapsed form); the second half is made
ill-conditioned — DNS by a large λ (γ = 2.5, 3, 4: the slope and curvature loadings coincide), GNS5 by γ₂ = γ₁ + ε.

Asserted in every case: no candidate's κ₁ lies in the factor-2 band [5e5, 2e6] around the kernels' threshold of 1e6;
last_deferred() equals the number of candidates with κ₁ ≥ 2e6 exactly (a deferred case that ran the FP64 form would
otherwise still pass); the parity rule of test_gpu_parity.assert_parity on the whole batch; and every deferred
candidate within 1e-9 of the binary128 truth relative to |ll| — the project's parity bar applied against the truth,
because the dense FP64 oracle is itself up to 4.4e-9 from the truth on these candidates.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import kalman_oracle as O
from oracle.truth import loglik_oracle, loglik_truth, predict_states_truth, states_truth
from test_gpu_deferred import kappa1
from test_gpu_parity import assert_parity
from test_gpu_predict import assert_close_truth, oracle_state
from yfm_amd import KIND_DNS, KIND_GNS, _lib
from yfm_amd import synthetic as S
from yfm_amd.params import n_params, state_dim, transform_params

pytestmark = pytest.mark.gpu

REL = 1e-9
NAME = {KIND_DNS: "DNS", KIND_GNS: "GNS5"}
DEFER_DNS = (2.5, 3.0, 4.0)     # γ: λ = 0.01 + e^γ so large that e^{−λm} ≈ 0 and C ≈ S
DEFER_GNS = (1e-3, -1e-5, 1e-7)  # γ₂ − γ₁


def maturities(N):
    return np.arange(1, N + 1, dtype=np.float64) * (360.0 / N)


def candidates(kind, N, B):
    """B candidates, the first B/2 as drawn, the others with the deferral recipe (two of them: its two extremes)."""
    Th = S.theta_batch(kind, B, seed=71 + N, bad_frac=0.0, scale=0.05)
    h = B // 2
    nd = B - h
    assert nd in (2, 3)
    pick = slice(None, None, 2) if nd == 2 else slice(None)
    if kind == KIND_DNS:
        Th[0, h:] = DEFER_DNS[pick]
    else:
        Th[1, h:] = Th[0, h:] + np.array(DEFER_GNS[pick])
    return np.asfortranarray(Th)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def deferred_mask(kind, Th, mats):
    """The candidates the kernels must defer; none may sit in the factor-2 band around their threshold."""
    k = kappa1(kind, Th, mats)
    band = (k >= 5e5) & (k <= 2e6)
    assert not band.any(), (np.flatnonzero(band), k[band])
    return k >= 2e6, k


def check_values(got, kind, Y, mats, Th, T_use, deferred, what):
    """The parity rule on the whole batch, and the deferred candidates within 1e-9 of the binary128 truth."""
    ora = loglik_oracle(kind, Y, mats, Th, T_use=T_use)
    tru = loglik_truth(kind, Y, mats, Th, T_use=T_use)
    assert np.isfinite(ora).all() and np.isfinite(tru).all(), (what, ora, tru)
    table = assert_parity(got, ora, tru)
    e_gt = np.abs(got - tru)
    print(what, f"B={Th.shape[1]} deferred={int(deferred.sum())}", table,
          "deferred vs truth max rel %.3e" % np.max(e_gt[deferred] / np.maximum(np.abs(tru[deferred]), 1e-300),
                                                    initial=0.0))
    bad = deferred & ~(e_gt <= REL * np.abs(tru))  # a truth of exactly 0.0 (T_use ≤ 2) must be met exactly
    assert not bad.any(), (what, np.flatnonzero(bad), got[bad], tru[bad])


def check_loglik(engine, kind, Y, mats, Th, what, T_use=None):
    deferred, k = deferred_mask(kind, Th, mats)
    engine.set_panel(Y, mats)
    got = engine.loglik(kind, Th, T_use=T_use)
    nd = engine.last_deferred()
    assert nd == int(deferred.sum()), (what, nd, k)
    check_values(got, kind, Y, mats, Th, T_use, deferred, what)
    return got


# ---- 1. loglik at both ends of every L --------------------------------------------------------------------------
# (kind, N, T, B): what the shape reaches — group kernel L / double-double kernel L
ENDS = [
    (KIND_DNS, 65, 8, 6), (KIND_DNS, 128, 8, 6),     # L = 8
    (KIND_DNS, 129, 8, 6), (KIND_DNS, 256, 8, 6),    # L = 16
    (KIND_DNS, 257, 8, 6), (KIND_DNS, 512, 6, 6),    # L = 32
    (KIND_DNS, 513, 6, 6),                           # L = 64
    (KIND_DNS, 1016, 5, 4),                          # L = 64, the last N with two columns per chunk (TC = 2)
    (KIND_DNS, 1024, 5, 4),                          # L = 64, the maximum: every slot owned, one column per chunk
    (KIND_GNS, 65, 8, 6), (KIND_GNS, 128, 8, 6),     # L = 16
    (KIND_GNS, 129, 8, 6), (KIND_GNS, 256, 8, 6),    # L = 32
    (KIND_GNS, 257, 8, 6), (KIND_GNS, 512, 6, 6),    # L = 64; 512 is the maximum
]


@functools.lru_cache(maxsize=None)
def ends_case(kind, N, T, B):
    mats = maturities(N)
    return frozen(S.simulate_panel(kind, T, maturities=mats), mats, candidates(kind, N, B))


@pytest.mark.parametrize("kind,N,T,B", ENDS, ids=[f"{NAME[k]}-N{N}" for k, N, _, _ in ENDS])
def test_loglik_at_both_ends_of_every_lane_count(engine, kind, N, T, B):
    """fixedz_group_kernel<L, M, LEAD, false> and fixedz_dd_loglik_kernel<L, M, LEAD, false> for every L that N > 64
    reaches, at the smallest and the largest N of each."""
    Y, mats, Th = ends_case(kind, N, T, B)
    check_loglik(engine, kind, Y, mats, Th, f"{NAME[kind]} N={N} T={T}")


# ---- 2. chunk hand-over, missing columns and windows ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def handover_case(kind, N):
    """N = 129, T = 32: the group kernel stages 14 columns per chunk and the double-double kernel 15; columns 14, 15,
    16, 29, 30 (1-based) are missing and column 31 has one missing entry, so each kernel has a missing column last in
    a chunk and first in the next one, and the windows end on and next to a hand-over of either.
    N = 1024, T = 5: one column per chunk in the group kernel, two in the double-double kernel; column 3 missing."""
    mats = maturities(N)
    if N == 129:
        T, tu = 32, (32, 29, 16, 15)
    else:
        T, tu = 5, (5, 4, 5, 3)
    Y = S.simulate_panel(kind, T, maturities=mats).copy(order="F")
    if N == 129:
        Y[:, [13, 14, 15, 28, 29]] = np.nan
        Y[7, 30] = np.nan
    else:
        Y[:, 2] = np.nan
    return frozen(Y, mats, candidates(kind, N, 4), np.array(tu, dtype=np.int32))


HANDOVER = [(KIND_DNS, 129), (KIND_GNS, 129), (KIND_DNS, 1024)]


@pytest.mark.parametrize("kind,N", HANDOVER, ids=[f"{NAME[k]}-N{N}" for k, N in HANDOVER])
def test_missing_columns_and_windows_at_chunk_handover(engine, kind, N):
    Y, mats, Th, tu = handover_case(kind, N)
    check_loglik(engine, kind, Y, mats, Th, f"{NAME[kind]} N={N} hand-over", T_use=tu)


# ---- 3. trajectories (RECORD) at large N, deferred candidates included ------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectory_case(kind, N):
    if N == 129:
        return handover_case(kind, N)
    mats = maturities(N)
    T = 6
    return frozen(S.simulate_panel(kind, T, maturities=mats), mats, candidates(kind, N, 4),
                  np.full(4, T, dtype=np.int32))


# N = 129: the hand-over panels (DNS L = 16, GNS5 L = 32); the others T = 6 and whole windows, one N per remaining L of
# either kernel's RECORD instantiations — DNS 65 (L = 8), 257 (32), 513 (64); GNS5 65 (16), 257 (64), and 64, where
# the per-lane kernel defers to the double-double kernel at L = 8
TRAJ = [(KIND_DNS, 65), (KIND_DNS, 129), (KIND_DNS, 257), (KIND_DNS, 513),
        (KIND_GNS, 64), (KIND_GNS, 65), (KIND_GNS, 129), (KIND_GNS, 257)]
TRAJ_IDS = [f"{NAME[k]}-N{N}" for k, N in TRAJ]


def normwise(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("kind,N", TRAJ, ids=TRAJ_IDS)
def test_filter_states_at_large_n(engine, kind, N):
    """fixedz_group_kernel<…, true> and fixedz_dd_loglik_kernel<…, true> through filter_states: ll, β and P of every
    candidate against the binary128 trajectory under the rule of assert_close_truth (within 1e-9 of the FP64 oracle or
    at least as close to the truth), the deferred candidates within 1e-9 of the truth normwise as well, NaN past a
    window's end.

    The deferred candidates' measured distance from the truth is printed, not gated beyond 1e-9
    (test_gpu_deferred.test_deferred_trajectories gates 1e-13 on ll and 1e-12 on β, P at N = 30; whether that holds
    here is recorded in profiles/group_dd/pytest_gpu.txt and DESIGN.md §3.1b)."""
    Y, mats, Th, tu = trajectory_case(kind, N)
    M = state_dim(kind)
    deferred, k = deferred_mask(kind, Th, mats)
    engine.set_panel(Y, mats)
    ll, beta, P = engine.filter_states(kind, Th, T_use=tu)
    assert engine.last_deferred() == int(deferred.sum()), k
    assert beta.shape == (M, Y.shape[1] - 1, 4) and P.shape == (M, M, Y.shape[1] - 1, 4)
    worst = {"ll": 0.0, "beta": 0.0, "P": 0.0}
    for b in range(4):
        n = int(tu[b])
        llt, bt, Pt = states_truth(kind, Y[:, :n], mats, Th[:, b])
        rec = []
        llo = O.loglik(kind, mats, M, Y[:, :n], Th[:, b], record=rec)
        bo = np.stack([r[0] for r in rec], axis=1)
        Po = np.stack([r[1] for r in rec], axis=2)
        assert np.isfinite(llt) and np.isfinite(bt).all() and np.isfinite(Pt).all(), (N, b)
        for name, got, ora, tru in (("ll", np.array([ll[b]]), np.array([llo]), np.array([llt])),
                                    ("beta", beta[:, :n - 1, b], bo, bt), ("P", P[:, :, :n - 1, b], Po, Pt)):
            assert_close_truth(got, ora, tru, what=(NAME[kind], N, name, b))
            if deferred[b]:
                d = normwise(got, tru)
                worst[name] = max(worst[name], d)
                assert d <= REL, (NAME[kind], N, name, b, d)
        assert np.isnan(beta[:, n - 1:, b]).all() and np.isnan(P[:, :, n - 1:, b]).all(), b
    print(f"{NAME[kind]} N={N} filter_states, deferred candidates vs binary128 truth (normwise): "
          + " ".join(f"{k_}={v:.3e}" for k_, v in worst.items())
          + f"; within the N = 30 gate (1e-13, 1e-12, 1e-12): "
          f"{worst['ll'] <= 1e-13 and worst['beta'] <= 1e-12 and worst['P'] <= 1e-12}")


@pytest.mark.parametrize("kind,N", TRAJ, ids=TRAJ_IDS)
def test_predict_at_large_n(engine, kind, N):
    """predict(horizon = 3) on the constrained θ of the same candidates and windows: factors and preds against the
    binary128 trajectory under assert_close_truth, NaN past each window's end."""
    Y, mats, Th, tu = trajectory_case(kind, N)
    h = 3
    deferred, k = deferred_mask(kind, Th, mats)
    Thc = transform_params(kind, Th)
    engine.set_panel(Y, mats)
    r = engine.predict(kind, Thc, space=1, T_use=tu, horizon=h)
    assert engine.last_deferred() == int(deferred.sum()), k
    for b in range(4):
        n = int(tu[b]) + h - 1
        Yb = Y[:, :tu[b]]
        ref = O.predict(oracle_state(kind, mats, Thc[:, b]), O.pad_nan(Yb, h))
        A = predict_states_truth(kind, Yb, mats, Thc[:, b], horizon=h)[:n + 1]
        Z = oracle_state(kind, mats, Thc[:, b]).Z
        tru = {"factors": A[1:].T, "preds": Z @ A[:n].T}
        for key in ("factors", "preds"):
            assert np.isfinite(tru[key]).all(), (N, key, b)
            assert_close_truth(r[key][:, :n, b], ref[key], tru[key], what=(NAME[kind], N, key, b))
        for key, v in r.items():
            assert np.isnan(v[:, n:, b]).all(), (key, b)


# ---- 4. the deferral list's second trip --------------------------------------------------------------------------
SECOND_TRIP = [(KIND_GNS, 257), (KIND_DNS, 513)]


@pytest.mark.parametrize("kind,N", SECOND_TRIP, ids=[f"{NAME[k]}-N{N}" for k, N in SECOND_TRIP])
def test_deferral_list_longer_than_one_grid_pass(engine, kind, N):
    """L = 64: four candidates per block, and the double-double kernel's grid is capped at 256 blocks, so 1,097
    deferred candidates need a second trip of its loop over the list (LDS reused, s_nobs_max reset, an idle group
    reading its block's first record).  Five distinct deferred θ with windows of their own are tiled over B = 1,100
    with three undeferred candidates at 0, 550 and 1,099; the group reductions have a fixed order, so every copy must
    equal its θ's value from a B = 1 call bit for bit, whatever its slot in the list and the trip that served it."""
    T, B = 5, 1100
    mats = maturities(N)
    Y = S.simulate_panel(kind, T, maturities=mats)
    D = S.theta_batch(kind, 5, seed=5, bad_frac=0.0, scale=0.05)
    if kind == KIND_GNS:
        D[1] = D[0] + np.array([1e-3, -1e-4, 1e-5, -1e-6, 1e-7])
    else:
        D[0] = (3.0, 3.25, 3.5, 3.75, 4.0)
    U = S.theta_batch(kind, 3, seed=71 + N, bad_frac=0.0, scale=0.05)
    Th8 = np.asfortranarray(np.hstack([D, U]))
    tu8 = np.array([5, 4, 3, 5, 2, 5, 5, 5], dtype=np.int32)
    deferred8, k8 = deferred_mask(kind, Th8, mats)
    assert deferred8.tolist() == [True] * 5 + [False] * 3, k8

    src = np.empty(B, dtype=np.int64)  # which of the eight distinct θ sits in each slot
    free = np.array([0, 550, 1099])
    src[free] = (5, 6, 7)
    rest = np.setdiff1d(np.arange(B), free)
    src[rest] = np.arange(rest.size) % 5
    engine.set_panel(Y, mats)
    got = engine.loglik(kind, np.asfortranarray(Th8[:, src]), T_use=tu8[src])
    assert engine.last_deferred() == 1097
    solo = np.array([engine.loglik(kind, Th8[:, i], T_use=tu8[i:i + 1])[0] for i in range(8)])
    np.testing.assert_array_equal(got, solo[src])
    first = np.array([int(np.flatnonzero(src == i)[0]) for i in range(8)])
    check_values(got[first], kind, Y, mats, Th8, tu8, deferred8, f"{NAME[kind]} N={N} second trip")


# ---- 5. the limit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N", [(KIND_DNS, 1025), (KIND_GNS, 513)], ids=["DNS-N1025", "GNS5-N513"])
def test_refusal_above_the_largest_n(engine, kind, N):
    """One maturity more than the lane-group kernels hold: YFM_EUNSUPPORTED from the C ABI with a message naming the
    limit, YFMError with that code from Engine (as the other size refusals), and the context still serves N = 65."""
    mats = maturities(N)
    P = n_params(kind)
    Th = np.asfortranarray(S.theta_batch(kind, 1, seed=71 + N, bad_frac=0.0, scale=0.05))
    engine.set_panel(np.asfortranarray(np.ones((N, 4)) + np.arange(N)[:, None] * 1e-3), mats)
    out = np.full(1, 7.0)
    rc = engine.lib.yfm_loglik_batch(engine.ctx, kind, 0, _lib.dptr(Th), P, 1, None, _lib.dptr(out))
    assert rc == -4  # YFM_EUNSUPPORTED
    msg = engine.lib.yfm_last_error().decode()
    assert msg == f"N = {N} maturities exceeds the fixed-loading kernels' {N - 1}", msg
    assert out[0] == 7.0  # nothing was written
    with pytest.raises(_lib.YFMError) as e:
        engine.loglik(kind, Th)
    assert e.value.code == -4 and str(N - 1) in str(e.value), str(e.value)
    Y, m65, Th65 = ends_case(kind, 65, 8, 6)
    check_loglik(engine, kind, Y, m65, Th65, f"{NAME[kind]} N=65 after the refusal at N={N}")
