"""GPU tests of the neural Nelson–Siegel models (csrc/yfm_msedn.hip) against the restatement of the reference in
tests/msedn_reference.py.

Parity rule (README): a finite GPU value passes when it is within 1e-9 relative of the Float64 restatement or at
least as close to the 40-digit truth as that restatement is; −Inf must agree exactly; no candidate is left out.
The restatement's values for the parity batches are recorded in tests/golden/msedn/ (make_msedn.py defines the
cases: maturities, panels from simulate_panel, θ from theta_batch with bad_frac = 0; every recorded value is finite);
a truth is computed only where the rule's second clause asks for one.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_device_entry_matches

import msedn_reference as R
from oracle import optim_nm as NM
from yfm_amd import _lib
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

sys.path.insert(0, str(GOLDEN / "msedn"))
import make_msedn as MM  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-9
mats_for, panel_for, theta_for = MM.mats_for, MM.panel_for, MM.theta_for
# one static, one with B, one random-walk scaled, one anchored
TRAJ_KINDS = (R.KIND_NNS, R.sd_kind(0), R.sd_kind(1, True, True), R.sd_kind(2, False, False, True))


@pytest.fixture(scope="module")
def cases():
    return MM.load_cases()


@pytest.fixture
def lanes_env():
    old = os.environ.pop("YFM_MSED_LANES", None)
    yield
    os.environ.pop("YFM_MSED_LANES", None)
    if old is not None:
        os.environ["YFM_MSED_LANES"] = old


def assert_parity(got, ref, truth_of, what=""):
    """Every candidate: −Inf agrees exactly, finite values meet the parity rule (truth_of(b) only where needed)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
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
        if len(missed) == 3:  # enough to fail and to show: a truth costs seconds
            break
    for m in missed:
        print("  missed: candidate %d gpu %.17g float64 %.17g truth %.17g" % m)
    assert not missed, (what, "missed", len(missed), "(counting stops at 3) of", got.size, missed)


def truth_of_case(kind, N, T, space):
    return lambda b: R.get_loss(kind, mats_for(N), panel_for(N, T), theta_for(kind, space)[:, b], space, R.TRUTH)


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("N", [4, 30])
@pytest.mark.parametrize("kind", MM.ALL_KINDS)
def test_loss_parity_all_kinds(engine, cases, kind, N, space):
    T, B = 40, 70
    engine.set_panel(panel_for(N, T), mats_for(N))
    got = engine.loglik(kind, theta_for(kind, space)[:, :B], space=space)
    ref = cases[f"float_{kind}_{N}_{T}_{space}"][:B]
    assert np.all(np.isfinite(ref))
    assert_parity(got, ref, truth_of_case(kind, N, T, space), f"{P.KIND_NAMES[kind]} N {N} space {space}")
    assert engine.last_flags() == (0, 0)


@pytest.mark.parametrize("lanes", ["4", "16"])
@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("B", [1, 70, 300])
@pytest.mark.parametrize("T", MM.REP_T)
@pytest.mark.parametrize("N", MM.REP_N)
@pytest.mark.parametrize("kind", MM.REP_KINDS)
def test_loss_parity_representative(engine, cases, lanes_env, kind, N, T, B, space, lanes):
    """N = 4: one interior Z₂ maturity; 5: the first with n − 2 > 2; 33: three maturities per lane at L = 16; 90:
    many per lane.  Both lane counts forced."""
    os.environ["YFM_MSED_LANES"] = lanes
    engine.set_panel(panel_for(N, T), mats_for(N))
    got = engine.loglik(kind, theta_for(kind, space)[:, :B], space=space)
    ref = cases[f"float_{kind}_{N}_{T}_{space}"][:B]
    assert np.all(np.isfinite(ref))
    assert_parity(got, ref, truth_of_case(kind, N, T, space),
                  f"{P.KIND_NAMES[kind]} N {N} T {T} B {B} space {space} L {lanes}")
    assert engine.last_flags() == (0, 0)


@pytest.mark.parametrize("kind", MM.REP_KINDS)
def test_nan_columns_and_windows(engine, kind):
    """Ragged windows over 20 candidates on a panel whose column 20 is NaN: −Inf for the windows that reach it,
    the restatement's value for those that stop before, 0.0 exactly for a window of one column.  Then a panel whose
    first column is NaN: step 1 is prediction-only and every value is finite."""
    N, T, B = 5, 40, 20
    mats = mats_for(N)
    Y = panel_for(N, T).copy(order="F")
    Y[:, 19] = np.nan
    tu = np.array([1, 2, 3, 17, 40])[np.arange(B) % 5]
    Th = theta_for(kind, 1)[:, :B]
    engine.set_panel(Y, mats)
    got = engine.loglik(kind, Th, space=1, T_use=tu)
    ref = np.array([R.get_loss(kind, mats, Y, Th[:, b], 1, R.FLOAT, int(tu[b])) for b in range(B)])
    assert np.all(np.isneginf(ref[tu == 40])) and np.all(np.isfinite(ref[tu < 20]))
    assert np.all(ref[tu == 1] == 0.0) and np.all(got[tu == 1] == 0.0)
    assert_parity(got, ref, lambda b: R.get_loss(kind, mats, Y, Th[:, b], 1, R.TRUTH, int(tu[b])), f"windows {kind}")
    assert engine.last_flags() == (0, int((tu == 40).sum()))
    Y1 = panel_for(N, T).copy(order="F")
    Y1[:, 0] = np.nan
    engine.set_panel(Y1, mats)
    got = engine.loglik(kind, Th[:, :6], space=1, T_use=[12] * 6)
    ref = np.array([R.get_loss(kind, mats, Y1, Th[:, b], 1, R.FLOAT, 12) for b in range(6)])
    assert np.all(np.isfinite(ref))
    assert_parity(got, ref, lambda b: R.get_loss(kind, mats, Y1, Th[:, b], 1, R.TRUTH, 12), f"NaN first column {kind}")


@pytest.mark.parametrize("N", [30, 33])
@pytest.mark.parametrize("kind", MM.REP_KINDS)
def test_batch_independence(engine, lanes_env, kind, N):
    """A candidate's loss is bitwise the same alone, inside a batch of 70, with the batch reversed, with either
    lane count forced, and inside 8,260 candidates (past the 8,192 at which L goes from 16 to 4)."""
    T = 40
    engine.set_panel(panel_for(N, T), mats_for(N))
    Th = theta_for(kind, 0)[:, :70]
    base = engine.loglik(kind, Th, space=0).copy()
    assert np.all(np.isfinite(base))
    for b in (0, 33, 69):
        assert engine.loglik(kind, Th[:, b], space=0)[0] == base[b]
    np.testing.assert_array_equal(engine.loglik(kind, np.asfortranarray(Th[:, ::-1]), space=0)[::-1], base)
    for lanes in ("4", "16"):
        os.environ["YFM_MSED_LANES"] = lanes
        np.testing.assert_array_equal(engine.loglik(kind, Th, space=0), base)
    os.environ.pop("YFM_MSED_LANES")
    big = np.asfortranarray(np.tile(Th, (1, 118)))
    np.testing.assert_array_equal(engine.loglik(kind, big, space=0), np.tile(base, 118))


@pytest.mark.parametrize("N", [4, 30])
def test_ridge_branch(engine, N):
    """NNS with γ = 0: raw = 0, so Z₂ = e₁ and Z₃ = 0, the third pivot is exactly zero and the 1e-3 ridge solve runs:
    finite, and the restatement's.  A score-driven kind with ω = 0: the restatement decides the class (the score's
    ∂/∂Q at Q = 0 is not finite), the kernel lands in the same one."""
    T = 8
    mats, Y = mats_for(N), panel_for(N, T)
    engine.set_panel(Y, mats)
    for kind in (R.KIND_NNS, R.KIND_NNS_ANCHORED):
        th = S.theta0_constrained(kind)
        th[:18] = 0.0
        ref = R.get_loss(kind, mats, Y, th, 1, R.FLOAT)
        assert np.isfinite(ref) or kind == R.KIND_NNS_ANCHORED  # anchored: 0.9610/√0 is not finite, 0·Inf = NaN
        got = engine.loglik(kind, th, space=1)
        assert_parity(got, [ref], lambda b: R.get_loss(kind, mats, Y, th, 1, R.TRUTH), f"ridge kind {kind} N {N}")
    for kind in (R.sd_kind(0), R.sd_kind(2, True, True)):
        th = S.theta0_constrained(kind)
        lay = P.neural_layout(kind)
        th[lay.gamma_offset:lay.gamma_offset + 18] = 0.0
        ref = R.get_loss(kind, mats, Y, th, 1, R.FLOAT)
        got = engine.loglik(kind, th, space=1)
        assert_parity(got, [ref], lambda b: R.get_loss(kind, mats, Y, th, 1, R.TRUTH), f"ω = 0 kind {kind} N {N}")


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


@pytest.mark.parametrize("N", [4, 30])
@pytest.mark.parametrize("kind", TRAJ_KINDS)
def test_trajectory_outputs(engine, kind, N):
    """predict (preds, β, γ(18), both loading columns) on the NaN padding with ragged windows, get_loss_array and a
    forecast block, against the restatement."""
    T, h = 40, 6
    mats, Y = mats_for(N), panel_for(N, T)
    Th = theta_for(kind, 1)[:, :3]
    tu = np.array([40, 17, 1])
    engine.set_panel(Y, mats)
    out = engine.predict(kind, Th, space=1, T_use=tu, horizon=h)
    ncol = T + h - 1
    assert out["preds"].shape == (N, ncol, 3) and out["factors"].shape == (3, ncol, 3)
    assert out["states"].shape == (18, ncol, 3) and out["factor_loadings_2"].shape == (N, ncol, 3)
    for b in range(3):
        want = R.predict(kind, mats, Y, Th[:, b], 1, R.FLOAT, int(tu[b]), h)
        n = int(tu[b]) + h - 1
        for k in ("preds", "factors", "states", "factor_loadings_1", "factor_loadings_2"):
            assert np.all(np.isfinite(out[k][:, :n, b])), k
            _close(out[k][:, :n, b], want[k], f"predict {kind} {k} b {b}")
            assert np.all(np.isnan(out[k][:, n:, b])), k
        assert np.all(out["factor_loadings_1"][0, :n, b] == 1.0) and np.all(out["factor_loadings_1"][-2:, :n, b] == 0.0)
        assert np.all(out["factor_loadings_2"][[0, -1], :n, b] == 0.0)
    model, _ = M.create_neural_model(P.KIND_NAMES[kind], mats, N, 3)
    fb = M.forecast_batch(model, Y, Th, tu, h, space=1)
    assert fb.shape == (3 + 18 + N, h, 3)
    for b in range(3):
        _close(fb[:, :, b], R.forecast(kind, mats, Y, Th[:, b], int(tu[b]), h, 1, R.FLOAT), f"forecast {kind} b {b}")
    # per-step losses: NaN beyond each window, a −Inf row where a compared column holds a NaN
    Yn = Y.copy(order="F")
    Yn[1, 24] = np.nan
    engine.set_panel(Yn, mats)
    la = engine.loss_array(kind, Th, space=1, T_use=[40, 17, 1])
    assert la.shape == (T - 1, 3)
    assert np.all(np.isneginf(la[:, 0])) and np.all(np.isnan(la[16:, 1])) and np.all(np.isnan(la[:, 2]))
    _close(la[:16, 1], R.get_loss_array(kind, mats, Yn, Th[:, 1], 1, R.FLOAT, 17), f"loss array {kind}")
    assert engine.last_flags() == (0, 1)
    # the model-level forms
    M.set_params_(model, Th[:, 1])
    single = M.predict(model, Y)
    assert single["states"].shape == (18, T)
    _close(single["preds"], R.predict(kind, mats, Y, Th[:, 1], 1, R.FLOAT)["preds"], "model predict")
    arr = M.get_loss_array(model, Y)
    assert arr.shape == (T - 1,) and M.get_loss(model, Y) == pytest.approx(arr.sum() / T, rel=1e-12)
    assert M.get_loss_array(model, Yn) == -np.inf and M.get_loss(model, Yn) == -np.inf
    th_u = P.untransform_params(kind, Th[:, 1])
    assert M.compute_loss(model, Y, th_u) == pytest.approx(-arr.sum() / T, rel=1e-9)
    assert M.compute_loss_batch(model, Y, th_u[:, None])[0] == M.compute_loss(model, Y, th_u)
    assert M.get_loss_batch(model, Y, Th[:, 1:2])[0] == M.get_loss(model, Y)


@pytest.mark.parametrize("kind", MM.TRYINIT_KINDS)
def test_try_initializations_batch(engine, cases, monkeypatch, kind):
    """1SD-NNS (256 trials) and 1RWSD-NNS (16) on two windows: the winner index and parameters of the restatement's
    sequential walk (a trial wins only on a strict improvement, in trial order), the start and all trials of both
    windows in one launch.  Panel and start are ones on which the restatement's winner leads every other trial by
    ≥ 1e-8 relative (tests/golden/msedn/make_msedn.py): from θ₀ the trials tie to 1e-15 and no two Float64
    evaluations need agree on the winner."""
    N, T = MM.TRYINIT_N, MM.TRYINIT_T
    mats, Y = mats_for(N), MM.tryinit_panel()
    windows = np.array(MM.TRYINIT_WINDOWS)
    model, _ = M.create_neural_model(P.KIND_NAMES[kind], mats, N, 3)
    start = MM.tryinit_start(kind)
    n_trials = 256 if P.neural_has_b(kind) else 16
    grid = M._trial_grid(model)
    assert grid.shape[1] == n_trials
    calls = []
    real = engine.loglik

    def counted(*a, **k):
        out = real(*a, **k)
        calls.append(out.shape[0])
        return out

    monkeypatch.setattr(engine, "loglik", counted)
    W, L = M.try_initializations_batch(np.repeat(start[:, None], 2, axis=1), model, Y, T_use=windows)
    monkeypatch.undo()
    assert calls == [2 * (n_trials + 1)]  # one launch holds everything
    for w, tu in enumerate(windows):
        losses = cases[f"tryinit_{kind}_{tu}"]  # the restatement's walk: the start, then every trial
        assert losses.shape == (n_trials + 1,) and np.all(np.isfinite(losses))
        k_best = 0
        for k in range(1, n_trials + 1):
            if losses[k] < losses[k_best]:
                k_best = k
        want = start.copy()
        if k_best:
            want[:grid.shape[0]] = grid[:, k_best - 1]
        print("window", tu, "winner: trial", k_best, "loss", losses[k_best])
        np.testing.assert_array_equal(W[:, w], want)
        assert L[w] == pytest.approx(losses[k_best], rel=REL)
    one = M.try_initializations(start, model, np.asfortranarray(Y[:, :windows[0]]))
    np.testing.assert_array_equal(one[:, 0], W[:, 0])


def test_nm_block_equals_sequential_nelder_mead(engine):
    """yfm_nm_block on 1SD-NNS with the four (A₁, A₂, B₁, B₂) coordinates as the block, three chains on windows
    40, 24 and 12: bit for bit the sequential restatement of Optim's NelderMead run on engine.loglik."""
    kind = R.sd_kind(0)
    mats = mats_for(4)
    Y = S.simulate_panel(kind, 40, maturities=mats, seed=7)
    engine.set_panel(Y, mats)
    idx = np.arange(4)
    windows = np.array([40, 24, 12], dtype=np.int32)
    p0 = np.asfortranarray(theta_for(kind, 0)[:, :3])
    X, f, n_evals = engine.nm_block(kind, p0, idx, T_use=windows, iterations=40, g_tol=1e-6)
    assert n_evals > 0
    np.testing.assert_array_equal(X[4:], p0[4:])
    for r in range(3):
        def objective(x, r=r):
            th = p0[:, r].copy()
            th[idx] = x
            return -float(engine.loglik(kind, th, space=0, T_use=[int(windows[r])])[0])
        want = NM.nelder_mead(objective, p0[idx, r], iterations=40, g_tol=1e-6)
        np.testing.assert_array_equal(X[idx, r], want.x)
        assert f[r] == want.f and f[r] <= objective(p0[idx, r])


def test_device_entry_point(engine):
    N, T = 30, 40
    engine.set_panel(panel_for(N, T), mats_for(N))
    for kind in (R.KIND_NNS, R.sd_kind(2, False, True)):
        Th = theta_for(kind, 0)[:, :70]
        tu = (np.arange(70) % 40 + 1).astype(np.int32)
        assert_device_entry_matches(engine.loglik, engine.loglik_device, kind, Th, tu, space=0)


def test_unsupported_requests(engine, lanes_env):
    N, T = 5, 12
    mats, Y = mats_for(N), panel_for(N, 40)[:, :T].copy(order="F")
    engine.set_panel(Y, mats)
    for kind in (R.KIND_NNS, R.sd_kind(0), R.sd_kind(2, True, True, True)):
        th = S.theta0_constrained(kind)
        for call in (lambda: engine.filter_states(kind, th, space=1),
                     lambda: engine.estimate(kind, th, space=1, iterations=1),
                     lambda: engine.loglik_grad(kind, th, space=1),
                     lambda: engine.lambda_loss_grad(kind, th, space=1),
                     lambda: engine.loss_array(kind, th, space=1, K=2)):
            with pytest.raises(_lib.YFMError) as e:
                call()
            assert e.value.code == -4 and str(e.value), str(e.value)
        assert np.isfinite(engine.loglik(kind, th, space=1)[0])
    # N < 4: the transforms alias their anchor slots; N beyond the kernel's maximum
    kind = R.sd_kind(0)
    th = S.theta0_constrained(kind)
    for n in (3, 1025):
        m = np.arange(1, n + 1) * 1.0
        engine.set_panel(np.ones((n, 4), order="F"), m)
        with pytest.raises(_lib.YFMError) as e:
            engine.loglik(kind, th, space=1)
        assert e.value.code == -4 and "N = %d" % n in str(e.value)
    # the largest N, at both lane counts (L = 4 is the larger block record): the same bits
    engine.set_panel(np.asfortranarray(np.ones((1024, 3)) + np.arange(1024)[:, None] * 1e-3), np.arange(1, 1025) * 1.0)
    vals = []
    for lanes in ("16", "4"):
        os.environ["YFM_MSED_LANES"] = lanes
        vals.append(engine.loglik(R.KIND_NNS, S.theta0_constrained(R.KIND_NNS), space=1))
    assert vals[0].shape == (1,) and not np.isnan(vals[0][0]) and vals[0][0] == vals[1][0]
