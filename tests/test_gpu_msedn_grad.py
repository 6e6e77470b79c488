"""GPU tests of the neural models' loss with its δ/Φ gradient (csrc/yfm_msedn.hip neural_grad_kernel, include/yfm.h
yfm_neural_loss_grad_batch) against tests/golden/msedn_grad/: central differences of the 40-digit restatement.

Rule (the project's parity bar): per candidate max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd, in both parameter
spaces; a −Inf loss comes with 12 NaNs exactly where the fixture has them; the loss beside the gradient is
engine.loglik's bit for bit; all 13 outputs of a candidate are bitwise independent of the batch and of the lane count.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_device_entry_matches
from grad_rule import assert_candidate_rule as check_gradient
from yfm_amd import _lib
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

sys.path.insert(0, str(GOLDEN / "msedn_grad"))
sys.path.insert(0, str(GOLDEN / "msedn"))
import make_msedn as MN  # noqa: E402
import make_msedn_grad as MG  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = MG.kinds()


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MG.case_names())
def test_gradient_matches_truth(engine, cases, name, space):
    """Every fixture case of every kind: the rule above, the loss bitwise engine.loglik's, −Inf ⇔ 12 NaNs, the −Inf
    count."""
    c = cases
    kind = kind_of(name)
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    tu = c[f"{name}_T_use"]
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    loss, g = engine.neural_loss_grad(kind, Th, space=space, T_use=tu)
    thrown, neg_inf = engine.last_flags()
    g_fd = c[f"{name}_g_fd_s{space}"]
    assert thrown == 0 and neg_inf == int(np.isnan(g_fd).any(axis=0).sum())
    assert g.shape == (12, Th.shape[1])
    np.testing.assert_array_equal(loss, engine.loglik(kind, Th, space=space, T_use=tu))
    np.testing.assert_array_equal(np.isneginf(loss), np.isnan(g).all(axis=0))
    np.testing.assert_array_equal(np.isneginf(loss), np.isnan(g).any(axis=0))
    worst = check_gradient(g, g_fd, c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")
    print(f"{name} space {space}: worst max|g - g_fd| / |g_fd|inf = {worst:.3e}")


@pytest.fixture
def lanes_env():
    old = os.environ.pop("YFM_MSED_LANES", None)
    yield
    os.environ.pop("YFM_MSED_LANES", None)
    if old is not None:
        os.environ["YFM_MSED_LANES"] = old


@pytest.mark.parametrize("N", [4, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence(engine, lanes_env, kind, N):
    """All 13 outputs of a candidate are the same bits alone, inside a batch of 70, with the batch reversed, with
    either lane count forced, and (N = 4) inside 8,260 candidates — past the 8,192 at which L goes from 16 to 4."""
    mats, Y = MN.mats_for(N), MN.panel_for(N, 8)
    Th = np.asfortranarray(MN.theta_for(kind, 0)[:, :70])
    engine.set_panel(Y, mats)

    def both(X):
        loss, g = engine.neural_loss_grad(kind, X, space=0)
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
    if N == 4:
        big = np.asfortranarray(np.tile(Th, (1, 118)))
        assert big.shape[1] > 8192
        np.testing.assert_array_equal(both(big), np.tile(base, (1, 118)))


def test_device_entry_point(engine):
    """The device-pointer call on a stream of its own writes the host-pointer call's bits."""
    N, T = 30, 40
    mats, Y = MN.mats_for(N), MN.panel_for(N, T)
    engine.set_panel(Y, mats)
    for kind in KINDS:
        Th = np.asfortranarray(MN.theta_for(kind, 0)[:, :70])
        tu = (np.arange(70) % 40 + 1).astype(np.int32)
        assert_device_entry_matches(engine.neural_loss_grad, engine.neural_loss_grad_device, kind, Th, tu, space=0)


def test_model_layer_and_refusals(engine, cases):
    """compute_neural_loss_grad_block is the reference's sign (−loss, −gradient); a λ or Kalman kind, N = 3 and N above
    the gradient kernel's maximum return −4 (YFM_EUNSUPPORTED)."""
    kind = MN.R.sd_kind(0)
    name = f"k{kind}_n4t8"
    mats, Y, Th = cases[f"{name}_maturities"], cases[f"{name}_Y"], cases[f"{name}_theta"]
    model, _ = M.create_neural_model("1SD-NNS", mats, len(mats), 3)
    f, g = M.compute_neural_loss_grad_block(model, Y, Th)
    loss, grad = engine.neural_loss_grad(kind, Th, space=0)
    np.testing.assert_array_equal(f, -loss)
    np.testing.assert_array_equal(g, -grad)
    np.testing.assert_array_equal(f, M.compute_loss_batch(model, Y, Th))
    mats30 = S.maturities_30()
    engine.set_panel(S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), mats30)
    for other in (P.KIND_DNS, P.KIND_TVL, P.KIND_GNS, P.KIND_NS, P.KIND_SD_NS, P.KIND_SSD_NS):
        with pytest.raises(_lib.YFMError) as e:
            engine.neural_loss_grad(other, S.theta0(other), space=0)
        assert e.value.code == -4, str(e.value)
    th = MN.theta_for(kind, 0)[:, 0]
    for N in (3, 1025):
        m = np.arange(1, N + 1) * 3.0
        engine.set_panel(np.ones((N, 4)), m)
        with pytest.raises(_lib.YFMError) as e:
            engine.neural_loss_grad(kind, th, space=0)
        assert e.value.code == -4, (N, str(e.value))
    # the largest N is served, with the loss kernel's bits
    engine.set_panel(np.asfortranarray(np.ones((1024, 3)) + np.arange(1024)[:, None] * 1e-3), np.arange(1, 1025) * 1.0)
    tn = S.theta0_constrained(P.KIND_NNS)
    loss, grad = engine.neural_loss_grad(P.KIND_NNS, tn, space=1)
    np.testing.assert_array_equal(loss, engine.loglik(P.KIND_NNS, tn, space=1))
    assert np.isneginf(loss[0]) == bool(np.isnan(grad).all())
    sdns, _ = M.create_model("SD-NS", mats30, 30, 3)
    with pytest.raises(NotImplementedError):
        M.compute_neural_loss_grad_block(sdns, S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), S.theta0(P.KIND_SD_NS))
