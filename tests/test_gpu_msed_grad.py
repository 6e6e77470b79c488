"""GPU tests of the λ models' loss with its δ/Φ gradient (csrc/yfm_msed.hip lambda_grad_kernel, include/yfm.h
yfm_lambda_loss_grad_batch) against tests/golden/msed_grad/: central differences of the 40-digit restatement.

Rule (tests/test_gpu_grad.py's): per candidate max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd, in both parameter spaces; a
−Inf loss comes with 12 NaNs exactly where the fixture has them; the loss beside the gradient is engine.loglik's
bit for bit; all 13 outputs of a candidate are bitwise independent of the batch and of the lane count.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_device_entry_matches
from grad_rule import REL, assert_candidate_rule as check_gradient
from yfm_amd import _lib
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

sys.path.insert(0, str(GOLDEN / "msed_grad"))
import make_msed_grad as MG  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = MG.KINDS
CODE = {3: "NS", 4: "SD-NS", 5: "RWSD-NS", 6: "SSD-NS", 8: "SRWSD-NS"}


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MG.case_names())
def test_gradient_matches_truth(engine, cases, name, space):
    """Every fixture case of every kind: the rule above, the loss bitwise engine.loglik's, the −Inf count."""
    c = cases
    kind = int(name[1])
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    tu = c[f"{name}_T_use"]
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    loss, g = engine.lambda_loss_grad(kind, Th, space=space, T_use=tu)
    thrown, neg_inf = engine.last_flags()
    g_fd = c[f"{name}_g_fd_s{space}"]
    assert thrown == 0 and neg_inf == int(np.isnan(g_fd).any(axis=0).sum())
    assert g.shape == (12, Th.shape[1])
    np.testing.assert_array_equal(loss, engine.loglik(kind, Th, space=space, T_use=tu))
    check_gradient(g, g_fd, c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


@pytest.mark.parametrize("kind", KINDS)
def test_chain_rule_between_spaces(engine, cases, kind):
    """The unconstrained gradient is the constrained one with the diagonal of Φ multiplied by 2y/(1 + y)², y = eˣ
    (from_R_to_11'); everything else is the identity.  The two θ differ by the rounding of the transform on Φ's
    diagonal, so the comparison is held to the project's bar, 1e-9 of ‖g‖∞ (and of the loss), not to bits."""
    name = f"k{kind}_n33t40"
    c = cases
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    Th, Tc = c[f"{name}_theta"], c[f"{name}_theta_c"]
    l0, g0 = engine.lambda_loss_grad(kind, Th, space=0)
    l1, g1 = engine.lambda_loss_grad(kind, Tc, space=1)
    np.testing.assert_allclose(l0, l1, rtol=REL)
    want = g1.copy()
    for d in (0, 4, 8):
        y = np.exp(Th[-9 + d])
        want[3 + d] *= 2 * y / (1 + y) ** 2
    print("max |g0 - chain(g1)| / |g|inf", np.max(np.abs(g0 - want) / np.max(np.abs(want), axis=0)))
    assert np.all(np.abs(g0 - want) <= REL * np.max(np.abs(want), axis=0))


@pytest.fixture
def lanes_env():
    old = os.environ.pop("YFM_MSED_LANES", None)
    yield
    os.environ.pop("YFM_MSED_LANES", None)
    if old is not None:
        os.environ["YFM_MSED_LANES"] = old


def mats_for(N):
    return S.maturities_30() if N == 30 else MG.maturities(N)


@pytest.mark.parametrize("N", [30, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence(engine, lanes_env, kind, N):
    """All 13 outputs of a candidate are the same bits alone, inside a batch of 70, with the batch reversed, with
    either lane count forced, and inside 8,260 candidates (past the 8,192 at which L goes from 16 to 4)."""
    T = 40
    mats = mats_for(N)
    Y = S.simulate_panel(kind, T, maturities=mats, seed=7)
    Th = S.theta_batch(kind, 70, scale=0.1, seed=500 + kind, bad_frac=0.0)
    engine.set_panel(Y, mats)

    def both(X):
        loss, g = engine.lambda_loss_grad(kind, X, space=0)
        return np.vstack([loss[None, :], g])

    base = both(Th)
    assert base.shape == (13, 70) and np.all(np.isfinite(base))
    for b in (0, 33, 69):
        np.testing.assert_array_equal(both(Th[:, b])[:, 0], base[:, b])
    np.testing.assert_array_equal(both(np.asfortranarray(Th[:, ::-1]))[:, ::-1], base)
    for lanes in ("4", "16"):
        os.environ["YFM_MSED_LANES"] = lanes
        np.testing.assert_array_equal(both(Th), base)
    os.environ.pop("YFM_MSED_LANES")
    big = np.asfortranarray(np.tile(Th, (1, 118)))
    np.testing.assert_array_equal(both(big), np.tile(base, (1, 118)))


def test_neg_inf_candidate_has_no_gradient(engine, cases):
    """Windows over a missing column: −Inf, 12 NaNs, counted by last_flags; the short window beside them is finite."""
    for kind in KINDS:
        name = f"k{kind}_n4t8nan6"
        engine.set_panel(cases[f"{name}_Y"], cases[f"{name}_maturities"])
        loss, g = engine.lambda_loss_grad(kind, cases[f"{name}_theta"], space=0, T_use=cases[f"{name}_T_use"])
        assert np.isfinite(loss[0]) and np.isfinite(g[:, 0]).all()
        assert np.isneginf(loss[1:]).all() and np.isnan(g[:, 1:]).all()
        assert engine.last_flags() == (0, 2)


def test_device_entry_point(engine):
    N, T = 30, 40
    mats = mats_for(N)
    Y = S.simulate_panel(P.KIND_SD_NS, T, maturities=mats, seed=7)
    engine.set_panel(Y, mats)
    for kind in KINDS:
        Th = S.theta_batch(kind, 70, scale=0.1, seed=500 + kind, bad_frac=0.0)
        tu = (np.arange(70) % 40 + 1).astype(np.int32)
        assert_device_entry_matches(engine.lambda_loss_grad, engine.lambda_loss_grad_device, kind, Th, tu, space=0)


def test_model_layer_and_unsupported_kinds(engine, cases):
    """compute_loss_grad_block is the reference's sign (−loss, −gradient); the Kalman kinds return −4."""
    name = "k4_n4t8"
    mats, Y, Th = cases[f"{name}_maturities"], cases[f"{name}_Y"], cases[f"{name}_theta"]
    model, _ = M.create_model("SD-NS", mats, len(mats), 3)
    f, g = M.compute_loss_grad_block(model, Y, Th)
    loss, grad = engine.lambda_loss_grad(4, Th, space=0)
    np.testing.assert_array_equal(f, -loss)
    np.testing.assert_array_equal(g, -grad)
    np.testing.assert_array_equal(f, M.compute_loss_batch(model, Y, Th))
    mats30 = S.maturities_30()
    engine.set_panel(S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), mats30)
    for kind in (P.KIND_DNS, P.KIND_TVL, P.KIND_GNS):
        with pytest.raises(_lib.YFMError) as e:
            engine.lambda_loss_grad(kind, S.theta0(kind), space=0)
        assert e.value.code == -4, str(e.value)
    dns, _ = M.create_model("1C", mats30, 30, 3)
    with pytest.raises(NotImplementedError):
        M.compute_loss_grad_block(dns, S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), S.theta0(P.KIND_DNS))
