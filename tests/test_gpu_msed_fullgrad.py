"""GPU tests of the λ models' loss with its full gradient (csrc/yfm_msed.hip lambda_fullgrad_kernel, include/yfm.h
yfm_lambda_loss_fullgrad_batch) against tests/golden/msed_fullgrad/: central differences of the 40-digit restatement
over all P rows, at the fixture's shapes.

Rule (tests/test_gpu_grad.py's): per candidate max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd over all P rows, in both
parameter spaces and with either lane count; a −Inf loss comes with P NaNs exactly where the fixture has them; the loss
is engine.loglik's and rows P−12 … P−1 are engine.lambda_loss_grad's, bit for bit; all P + 1 outputs of a candidate are
bitwise independent of the batch.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_device_entry_matches, same_bits
from grad_rule import REL, assert_candidate_rule as check_gradient
from yfm_amd import _lib
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

sys.path.insert(0, str(GOLDEN / "msed_fullgrad"))
import make_msed_fullgrad as MF  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = MF.KINDS


@pytest.fixture(scope="module")
def cases():
    return MF.load_cases()


@pytest.fixture
def lanes_env():
    old = os.environ.pop("YFM_MSED_LANES", None)
    yield
    os.environ.pop("YFM_MSED_LANES", None)
    if old is not None:
        os.environ["YFM_MSED_LANES"] = old


@pytest.mark.parametrize("lanes", ["4", "16"])
@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MF.case_names())
def test_full_gradient_matches_truth(engine, cases, lanes_env, name, space, lanes):
    """Every fixture case of every kind under both lane mappings: the rule above over all P rows, the loss bitwise
    engine.loglik's, rows P−12 … bitwise engine.lambda_loss_grad's, the −Inf count, nothing unavailable."""
    c = cases
    kind = int(name[1])
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    tu = c[f"{name}_T_use"]
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    os.environ["YFM_MSED_LANES"] = lanes
    loss, g = engine.lambda_loss_full_grad(kind, Th, space=space, T_use=tu)
    thrown, neg_inf = engine.last_flags()
    unavailable = engine.last_grad_unavailable()
    g_fd = c[f"{name}_g_fd_s{space}"]
    assert thrown == 0 and neg_inf == int(np.isnan(g_fd).any(axis=0).sum()) and unavailable == 0
    assert g.shape == Th.shape
    assert same_bits(loss, engine.loglik(kind, Th, space=space, T_use=tu))
    _, g12 = engine.lambda_loss_grad(kind, Th, space=space, T_use=tu)
    fin = np.isfinite(loss)
    assert same_bits(g[-12:, fin], g12[:, fin])
    assert np.isnan(g[:, ~fin]).all()
    check_gradient(g, g_fd, c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space} L={lanes}")


@pytest.mark.parametrize("kind", KINDS)
def test_chain_rule_between_spaces(engine, cases, kind):
    """The unconstrained gradient is the constrained one with row A multiplied by A, row B by B(1 − B) and the diagonal
    of Φ by 2y/(1 + y)², y = eˣ; everything else is the identity.  The two θ differ by the rounding of the transforms,
    so the comparison is held to the project's bar, 1e-9 of ‖g‖∞ (and of the loss), not to bits."""
    name = f"k{kind}_n33t40"
    c = cases
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    Th, Tc = c[f"{name}_theta"], c[f"{name}_theta_c"]
    l0, g0 = engine.lambda_loss_full_grad(kind, Th, space=0)
    l1, g1 = engine.lambda_loss_full_grad(kind, Tc, space=1)
    np.testing.assert_allclose(l0, l1, rtol=REL)
    want = g1.copy()
    if kind != 3:
        want[0] *= Tc[0]
    if kind in (4, 6):
        want[1] *= Tc[1] * (1 - Tc[1])
    for d in (0, 4, 8):
        y = np.exp(Th[-9 + d])
        want[-9 + d] *= 2 * y / (1 + y) ** 2
    print("max |g0 - chain(g1)| / |g|inf", np.max(np.abs(g0 - want) / np.max(np.abs(want), axis=0)))
    assert np.all(np.abs(g0 - want) <= REL * np.max(np.abs(want), axis=0))


@pytest.mark.parametrize("tag", ["n30t8", "n33t40"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence(engine, cases, lanes_env, kind, tag):
    """All P + 1 outputs of a candidate are the same bits alone, inside a batch of 70, with the batch reversed and with
    either lane count forced (the fixture's panels)."""
    name = f"k{kind}_{tag}"
    engine.set_panel(cases[f"{name}_Y"], cases[f"{name}_maturities"])
    Th = S.theta_batch(kind, 70, scale=0.1, seed=500 + kind, bad_frac=0.0)

    def both(X):
        loss, g = engine.lambda_loss_full_grad(kind, X, space=0)
        return np.vstack([loss[None, :], g])

    base = both(Th)
    assert base.shape == (Th.shape[0] + 1, 70) and np.all(np.isfinite(base))
    for b in (0, 33, 69):
        assert same_bits(both(Th[:, b])[:, 0], base[:, b])
    assert same_bits(both(np.asfortranarray(Th[:, ::-1]))[:, ::-1], base)
    for lanes in ("4", "16"):
        os.environ["YFM_MSED_LANES"] = lanes
        assert same_bits(both(Th), base)


def test_neg_inf_candidate_has_no_gradient(engine, cases):
    """Windows over a missing column: −Inf, P NaNs, counted by last_flags and not as unavailable; the short window
    beside them is finite."""
    for kind in KINDS:
        name = f"k{kind}_n4t8nan6"
        engine.set_panel(cases[f"{name}_Y"], cases[f"{name}_maturities"])
        loss, g = engine.lambda_loss_full_grad(kind, cases[f"{name}_theta"], space=0, T_use=cases[f"{name}_T_use"])
        assert np.isfinite(loss[0]) and np.isfinite(g[:, 0]).all()
        assert np.isneginf(loss[1:]).all() and np.isnan(g[:, 1:]).all()
        assert engine.last_flags() == (0, 2)
        assert engine.last_grad_unavailable() == 0


def test_window_without_a_compared_column(engine, cases):
    """T_use = 1 compares nothing: the loss engine.loglik gives and an exactly zero gradient."""
    for kind in KINDS:
        name = f"k{kind}_n4t8"
        engine.set_panel(cases[f"{name}_Y"], cases[f"{name}_maturities"])
        Th = cases[f"{name}_theta"]
        tu = np.array([1, 8, 1], dtype=np.int32)
        loss, g = engine.lambda_loss_full_grad(kind, Th, space=0, T_use=tu)
        assert same_bits(loss, engine.loglik(kind, Th, space=0, T_use=tu))
        assert np.all(g[:, [0, 2]] == 0.0) and np.all(np.isfinite(g[:, 1])) and np.any(g[:, 1] != 0.0)


def test_device_entry_point(engine, cases):
    """The _device entry on a side stream equals the synchronous one bit for bit (windows of every length)."""
    for kind in KINDS:
        name = f"k{kind}_n30t8"
        engine.set_panel(cases[f"{name}_Y"], cases[f"{name}_maturities"])
        Th = S.theta_batch(kind, 70, scale=0.1, seed=500 + kind, bad_frac=0.0)
        tu = (np.arange(70) % 8 + 1).astype(np.int32)
        assert_device_entry_matches(engine.lambda_loss_full_grad, engine.lambda_loss_full_grad_device, kind, Th, tu,
                                    space=0)


def test_model_layer_and_unsupported_kinds(engine, cases):
    """compute_lambda_loss_grad_batch and compute_loss_grad_batch are the reference's sign (−loss, −gradient) for a λ
    model; the Kalman and neural kinds return −4 from the C entry."""
    name = "k4_n4t8"
    mats, Y, Th = cases[f"{name}_maturities"], cases[f"{name}_Y"], cases[f"{name}_theta"]
    model, _ = M.create_model("SD-NS", mats, len(mats), 3)
    f, g = M.compute_lambda_loss_grad_batch(model, Y, Th)
    loss, grad = engine.lambda_loss_full_grad(4, Th, space=0)
    assert same_bits(f, -loss) and same_bits(g, -grad)
    f2, g2 = M.compute_loss_grad_batch(model, Y, Th)
    assert same_bits(f2, f) and same_bits(g2, g)
    assert same_bits(f, M.compute_loss_batch(model, Y, Th))
    mats30 = S.maturities_30()
    engine.set_panel(S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), mats30)
    neural = [P.KIND_NNS, M.create_neural_model("1SD-NNS", mats30, 30, 3)[0].kind]
    for kind in [P.KIND_DNS, P.KIND_TVL, P.KIND_GNS] + neural:
        with pytest.raises(_lib.YFMError) as e:
            engine.lambda_loss_full_grad(kind, S.theta0(kind), space=0)
        assert e.value.code == -4, str(e.value)
    dns, _ = M.create_model("1C", mats30, 30, 3)
    with pytest.raises(NotImplementedError):
        M.compute_lambda_loss_grad_batch(dns, S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), S.theta0(P.KIND_DNS))


def test_lambda_overflow_makes_the_gradient_unavailable(engine, cases):
    """NS with γ = 800: λ = Inf, the ridged OLS gives a finite loss (engine.loglik's) and lambda_loss_grad 12 finite
    rows, but ∂Z/∂γ is NaN: all P rows NaN, counted by last_grad_unavailable and not by last_flags."""
    engine.set_panel(cases["k3_n4t8_Y"], cases["k3_n4t8_maturities"])
    Th = np.asfortranarray(cases["k3_n4t8_theta"].copy())
    Th[0, 1] = 800.0
    loss, g = engine.lambda_loss_full_grad(3, Th, space=0)
    assert engine.last_flags() == (0, 0) and engine.last_grad_unavailable() == 1
    assert same_bits(loss, engine.loglik(3, Th, space=0)) and np.isfinite(loss).all()
    _, g12 = engine.lambda_loss_grad(3, Th, space=0)
    assert np.isnan(g[:, 1]).all() and np.isfinite(g12[:, 1]).all()
    assert same_bits(g[-12:, [0, 2]], g12[:, [0, 2]]) and np.isfinite(g[:, [0, 2]]).all()
