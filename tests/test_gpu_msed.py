"""GPU tests of the static and score-driven λ models (csrc/yfm_msed.hip) against the restatement of
src/models/filter.jl in tests/msed_reference.py.

Parity rule (README): a finite GPU value passes when it is within 1e-9 relative of the Float64 restatement or at
least as close to the 40-digit truth as that restatement is; −Inf must agree exactly; no candidate is left out.
The restatement of a (kind, N, T, space) case is computed once for 300 candidates and shared by the three batch
sizes, which evaluate prefixes of the same batch.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import msed_reference as R
from gpu_scenarios import assert_device_entry_matches
from yfm_amd import _lib
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

pytestmark = pytest.mark.gpu

KINDS = R.KINDS
CODE = {3: "NS", 4: "SD-NS", 5: "RWSD-NS", 6: "SSD-NS", 8: "SRWSD-NS"}
REL = 1e-9


def mats_for(N):
    if N <= 4:
        return np.array([3.0, 12.0, 60.0, 120.0])[:N]
    if N == 30:
        return S.maturities_30()
    if N == 10:
        return S.maturities_30()[::3]
    return np.arange(1, N + 1) * float(360 // N)


_panels, _thetas, _refs = {}, {}, {}


def panel_for(N, T):
    if (N, T) not in _panels:
        _panels[(N, T)] = S.simulate_panel(P.KIND_SD_NS, T, maturities=mats_for(N))
    return _panels[(N, T)]


def theta_for(kind, space):
    """300 candidates from theta_batch(kind, …, scale 0.1); space 1: their constrained images."""
    if (kind, space) not in _thetas:
        Th = S.theta_batch(kind, 300, scale=0.1, seed=500 + kind, bad_frac=0.0)
        _thetas[(kind, 0)] = Th
        _thetas[(kind, 1)] = np.asfortranarray(P.transform_params(kind, Th))
    return _thetas[(kind, space)]


def ref_for(kind, N, T, space, B):
    """Float64 restatement of the first B candidates (computed once per case, extended on demand)."""
    key = (kind, N, T, space)
    have = _refs.setdefault(key, np.empty(0))
    if have.size < B:
        Th = theta_for(kind, space)
        more = [R.get_loss(kind, mats_for(N), panel_for(N, T), Th[:, b], space, R.FLOAT) for b in range(have.size, B)]
        _refs[key] = have = np.concatenate([have, more])
    return have[:B]


_truths = {}


def truth_for(kind, N, T, space, b):
    """The 40-digit value of candidate b (25 ms each: computed where the rule needs it, once per case)."""
    key = (kind, N, T, space, b)
    if key not in _truths:
        _truths[key] = R.get_loss(kind, mats_for(N), panel_for(N, T), theta_for(kind, space)[:, b], space, R.TRUTH)
    return _truths[key]


def assert_parity(got, ref, truth_of, what=""):
    """Every candidate: −Inf agrees exactly, finite values meet the parity rule (truth_of(b) only where needed)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    assert not np.isnan(got).any(), what
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (what, got, ref)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), what
    rel = np.zeros(got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):  # a reference of 0.0 (one-column window) must be met exactly
        rel[fin] = np.where(got[fin] == ref[fin], 0.0, np.abs(got[fin] - ref[fin]) / np.abs(ref[fin]))
    print(what, "finite", int(fin.sum()), "of", got.size, "max rel", rel.max() if rel.size else 0.0)
    missed = []
    for b in np.flatnonzero(rel > REL):
        truth = truth_of(int(b))
        if not R.parity_ok(got[b], ref[b], truth, REL):
            missed.append((int(b), float(got[b]), float(ref[b]), truth))
        if len(missed) == 5:  # enough to fail and to show: the truth costs 25 ms a candidate
            break
    for m in missed:
        print("  missed: candidate %d gpu %.17g float64 %.17g truth %.17g" % m)
    assert not missed, (what, "missed", len(missed), "(counting stops at 5) of", got.size, missed[:3])


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("B", [1, 70, 300])
@pytest.mark.parametrize("T", [8, 40])
@pytest.mark.parametrize("N", [1, 3, 4, 30, 33, 90])
@pytest.mark.parametrize("kind", KINDS)
def test_loss_parity(engine, kind, N, T, B, space):
    """The issue's shapes, all of them held to the parity rule.

    The scaled kinds at N = 3 pass on the second clause of the rule: the loadings are square, OLS interpolates, the
    exact score is 0 and γ never moves (the 40-digit truth), but the scaled update (filter.jl:29-44) divides
    whatever rounding noise the score carries by its own magnitude, so the Float64 restatement takes steps of ±A
    and ends 1e-3 from the truth (e.g. T = 40, kind 6, candidate 298: restatement −0.42027081, truth −0.41984639).
    The kernel evaluates the scaled kinds' score at the refined β (csrc/yfm_msed.hpp) and stays within 1e-12 of
    the truth there; a first build without the refinement missed 18 of these cases."""
    mats, Y = mats_for(N), panel_for(N, T)
    Th = theta_for(kind, space)[:, :B]
    engine.set_panel(Y, mats)
    got = engine.loglik(kind, Th, space=space)
    ref = ref_for(kind, N, T, space, B)
    assert_parity(got, ref, lambda b: truth_for(kind, N, T, space, b), f"kind {kind} N {N} T {T} B {B} space {space}")
    thrown, neg_inf = engine.last_flags()
    assert thrown == 0 and neg_inf == int(np.isneginf(ref).sum())


def test_ridge_branch_is_deterministic(engine):
    """NS with γ = 800: λ = Inf, Z₂ = Z₃ = 0 exactly, so the second pivot is exactly zero in any arithmetic: the
    ridge retry runs and the loss is finite and the restatement's."""
    for N in (4, 30):
        mats, Y = mats_for(N), panel_for(N, 8)
        th = S.theta0_constrained(P.KIND_NS)
        th[0] = 800.0
        engine.set_panel(Y, mats)
        got = engine.loglik(P.KIND_NS, th, space=1)
        ref = R.get_loss(P.KIND_NS, mats, Y, th, 1, R.FLOAT)
        assert np.isfinite(ref)
        assert_parity(got, [ref], lambda b: R.get_loss(P.KIND_NS, mats, Y, th, 1, R.TRUTH), f"ridge N {N}")


@pytest.mark.parametrize("kind", KINDS)
def test_windows_and_missing_data(engine, kind):
    """T_use cycled over 70 candidates on a panel whose column 20 misses maturity 1: −Inf for the windows that
    reach it, finite (and the restatement's) for those that stop before."""
    N, T, B = 10, 40, 70
    mats = mats_for(N)
    Y = panel_for(N, T).copy(order="F")
    Y[0, 19] = np.nan
    tu = np.array([1, 2, 3, 17, 40])[np.arange(B) % 5]
    Th = theta_for(kind, 1)[:, :B]
    engine.set_panel(Y, mats)
    got = engine.loglik(kind, Th, space=1, T_use=tu)
    ref = np.array([R.get_loss(kind, mats, Y, Th[:, b], 1, R.FLOAT, int(tu[b])) for b in range(B)])
    assert np.all(np.isneginf(ref[tu == 40])) and np.all(np.isfinite(ref[tu < 20]))
    assert np.all(ref[tu == 1] == 0.0) and np.all(got[tu == 1] == 0.0)
    assert_parity(got, ref, lambda b: R.get_loss(kind, mats, Y, Th[:, b], 1, R.TRUTH, int(tu[b])), f"windows {kind}")
    assert engine.last_flags() == (0, int((tu == 40).sum()))


def _close(got, want, what):
    """Trajectory arrays: NaN / ±Inf in the same places, finite entries within 1e-9 of the array's scale."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    fin = np.isfinite(want)
    if fin.any():
        scale = np.abs(want[fin]).max()
        err = np.abs(got[fin] - want[fin]).max()
        print(what, "max err / scale", err / scale)
        assert err <= REL * scale, (what, err, scale)


@pytest.mark.parametrize("kind", KINDS)
def test_predict_on_nan_padding(engine, kind):
    """predict with horizon 12 on the NaN padding, windows of 17 and 24 columns: finite predictions equal to the
    restatement's, NaN beyond each window."""
    N, T, h = 10, 24, 12
    mats, Y = mats_for(N), panel_for(N, T)
    Th = theta_for(kind, 1)[:, :4]
    tu = np.array([24, 17, 1, 24])
    engine.set_panel(Y, mats)
    out = engine.predict(kind, Th, space=1, T_use=tu, horizon=h)
    ncol = T + h - 1
    assert out["preds"].shape == (N, ncol, 4) and out["factors"].shape == (3, ncol, 4)
    assert out["states"].shape == (1, ncol, 4) and out["factor_loadings_1"].shape == (N, ncol, 4)
    for b in range(4):
        want = R.predict(kind, mats, Y, Th[:, b], 1, R.FLOAT, int(tu[b]), h)
        n = int(tu[b]) + h - 1
        for k in ("preds", "factors", "states", "factor_loadings_1", "factor_loadings_2"):
            assert np.all(np.isfinite(out[k][:, :n, b])), k
            _close(out[k][:, :n, b], want[k], f"predict {kind} {k} b {b}")
            assert np.all(np.isnan(out[k][:, n:, b])), k
    # the model-level call: one candidate, the reference's named tuple
    model, _ = M.create_model(CODE[kind], mats, N, 3)
    M.set_params_(model, Th[:, 0])
    single = M.predict(model, Y)
    _close(single["preds"], R.predict(kind, mats, Y, Th[:, 0], 1, R.FLOAT)["preds"], "model predict")


@pytest.mark.parametrize("kind", KINDS)
def test_forecast_blocks(engine, kind):
    N, T, h = 10, 24, 6
    mats, Y = mats_for(N), panel_for(N, T)
    Th = theta_for(kind, 0)[:, :5]
    tu = np.array([24, 20, 2, 1, 13])
    model, _ = M.create_model(CODE[kind], mats, N, 3)
    out = M.forecast_batch(model, Y, Th, tu, h, space=0)
    assert out.shape == (3 + 1 + N, h, 5)
    for b in range(5):
        _close(out[:, :, b], R.forecast(kind, mats, Y, Th[:, b], int(tu[b]), h, 0, R.FLOAT), f"forecast {kind} b {b}")


@pytest.mark.parametrize("kind", KINDS)
def test_loss_array(engine, kind):
    """Per-step losses: entry 1 is a real value, NaN beyond each window, −Inf rows where the reference returns the
    scalar −Inf (a NaN in maturity 2 of column 15)."""
    N, T = 10, 24
    mats = mats_for(N)
    Y = panel_for(N, T).copy(order="F")
    Y[1, 14] = np.nan
    Th = theta_for(kind, 1)[:, :4]
    tu = np.array([24, 10, 1, 15])
    engine.set_panel(Y, mats)
    out = engine.loss_array(kind, Th, space=1, T_use=tu)
    assert out.shape == (T - 1, 4)
    for b in range(4):
        want = R.get_loss_array(kind, mats, Y, Th[:, b], 1, R.FLOAT, int(tu[b]))
        n = int(tu[b]) - 1
        assert np.all(np.isnan(out[n:, b]))
        if np.isscalar(want) or np.ndim(want) == 0:
            assert tu[b] >= 15 and np.all(np.isneginf(out[:n, b]))
        else:
            _close(out[:n, b], want, f"loss array {kind} b {b}")
            if n:
                assert out[0, b] < 0.0
    assert engine.last_flags() == (0, 2)
    # the model-level forms: the array, and the scalar −Inf
    model, _ = M.create_model(CODE[kind], mats, N, 3)
    M.set_params_(model, Th[:, 0])
    assert M.get_loss_array(model, Y) == -np.inf
    assert M.get_loss(model, Y) == -np.inf
    clean = panel_for(N, T)
    arr = M.get_loss_array(model, clean)
    assert arr.shape == (T - 1,) and M.get_loss(model, clean) == pytest.approx(arr.sum() / T, rel=1e-12)
    assert M.compute_loss(model, clean, P.untransform_params(kind, Th[:, 0])) == pytest.approx(-arr.sum() / T, rel=1e-9)
    with pytest.raises(_lib.YFMError) as e:
        engine.loss_array(kind, Th, space=1, K=2)
    assert e.value.code == -4


@pytest.fixture
def lanes_env():
    old = os.environ.pop("YFM_MSED_LANES", None)
    yield
    os.environ.pop("YFM_MSED_LANES", None)
    if old is not None:
        os.environ["YFM_MSED_LANES"] = old


@pytest.mark.parametrize("N", [30, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence(engine, lanes_env, kind, N):
    """A candidate's loss is bitwise the same alone, inside a batch of 70, with the batch reversed, with either
    lane count forced, and in a batch large enough for the launch to change its lane count by itself."""
    T = 40
    mats, Y = mats_for(N), panel_for(N, T)
    Th = theta_for(kind, 0)[:, :70]
    engine.set_panel(Y, mats)
    base = engine.loglik(kind, Th, space=0).copy()
    assert np.all(np.isfinite(base))
    for b in (0, 33, 69):
        assert engine.loglik(kind, Th[:, b], space=0)[0] == base[b]
    np.testing.assert_array_equal(engine.loglik(kind, np.asfortranarray(Th[:, ::-1]), space=0)[::-1], base)
    for lanes in ("4", "16"):
        os.environ["YFM_MSED_LANES"] = lanes
        np.testing.assert_array_equal(engine.loglik(kind, Th, space=0), base)
    os.environ.pop("YFM_MSED_LANES")
    big = np.asfortranarray(np.tile(Th, (1, 118)))  # 8,260 candidates: past the 8,192 at which L goes from 16 to 4
    np.testing.assert_array_equal(engine.loglik(kind, big, space=0), np.tile(base, 118))


def test_device_entry_point(engine):
    N, T = 30, 40
    mats, Y = mats_for(N), panel_for(N, T)
    engine.set_panel(Y, mats)
    for kind in KINDS:
        Th = theta_for(kind, 0)[:, :70]
        tu = (np.arange(70) % 40 + 1).astype(np.int32)
        assert_device_entry_matches(engine.loglik, engine.loglik_device, kind, Th, tu, space=0)


@pytest.mark.parametrize("kind", [4, 5, 6, 8])
def test_try_initializations(engine, kind):
    """The winner and its loss equal the restatement's sequential walk, on a panel where the best trial is neither
    the first nor the last; the batched-windows form matches the per-window calls bitwise."""
    N, T = 10, 24
    mats = mats_for(N)
    # (generating model, seed) of a panel on which an interior trial wins by ≥ 2e-6 relative (searched on the CPU
    # with the restatement; on most panels the smallest or the largest A wins)
    gen, seed = {4: (P.KIND_TVL, 8), 5: (P.KIND_DNS, 26), 6: (P.KIND_DNS, 0), 8: (P.KIND_DNS, 0)}[kind]
    Y = S.simulate_panel(gen, T, maturities=mats, seed=seed)
    model, _ = M.create_model(CODE[kind], mats, N, 3)
    start = S.theta0_constrained(kind)
    want, want_loss = R.try_initializations(kind, mats, Y, start)
    n_trials = 30 if P.lambda_has_b(kind) else 6
    trials = [R.trial_params(kind, start, k) for k in range(1, n_trials + 1)]
    idx = [k for k, p in enumerate(trials) if np.array_equal(p, want)]
    assert idx and 0 < idx[0] < n_trials - 1, idx  # neither the first nor the last trial
    got = M.try_initializations(start, model, Y)
    assert got.shape == (len(start), 1)
    np.testing.assert_array_equal(got[:, 0], want)
    assert -M.get_loss(model, Y) == pytest.approx(want_loss, rel=REL)
    # many windows, one launch
    tu = np.array([24, 12, 18, 6])
    starts = np.repeat(start[:, None], 4, axis=1)
    W, L = M.try_initializations_batch(starts, model, Y, T_use=tu)
    for w in range(4):
        Yw = np.asfortranarray(Y[:, :tu[w]])
        one, one_loss = M.try_initializations_batch(start[:, None], model, Yw)
        np.testing.assert_array_equal(W[:, w], one[:, 0])
        assert L[w] == one_loss[0]
        rw, rl = R.try_initializations(kind, mats, Y, start, T_use=int(tu[w]))
        assert L[w] == pytest.approx(rl, rel=REL)  # (the winner itself may be a near-tie on a short window)


def test_unsupported_requests(engine):
    N, T = 10, 24
    mats, Y = mats_for(N), panel_for(N, T)
    engine.set_panel(Y, mats)
    for kind in KINDS:
        th = S.theta0_constrained(kind)
        for call in (lambda: engine.filter_states(kind, th, space=1),
                     lambda: engine.estimate(kind, th, space=1, iterations=1),
                     lambda: engine.loglik_grad(kind, th, space=1),
                     lambda: engine.loss_array(kind, th, space=1, K=2)):
            with pytest.raises(_lib.YFMError) as e:
                call()
            assert e.value.code == -4, str(e.value)
        with pytest.raises(_lib.YFMError) as e:
            engine.loglik_grad(kind, th, space=1)
        assert "DNS" in str(e.value)
    # 7 is not a kind
    assert engine.lib.yfm_param_count(7) == -1 and engine.lib.yfm_gamma_dim(7) == -1
    assert [engine.lib.yfm_param_count(k) for k in KINDS] == [13, 15, 14, 15, 14]
    assert all(engine.lib.yfm_state_dim(k) == 3 and engine.lib.yfm_gamma_dim(k) == 1 for k in KINDS)
