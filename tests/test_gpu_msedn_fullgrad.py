"""GPU tests of the neural models' loss with its full gradient (csrc/yfm_msedn_adj.hip nns_sweep_kernel and
nns_adjoint_kernel, include/yfm.h yfm_neural_loss_fullgrad_batch) against tests/golden/msedn_fullgrad/: central
differences of the 40-digit restatement over the leading rows, at the fixture's shapes.

Rule (tests/test_gpu_msed_fullgrad.py's): per candidate max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd over the leading rows,
in both parameter spaces where stored and with either lane count; a −Inf loss comes with P NaNs exactly where the
fixture has them; the loss is engine.loglik's and rows P−12 … P−1 are engine.neural_loss_grad's, bit for bit; all P + 1
outputs of a candidate are bitwise independent of the batch, of the lane count and of the launch's chunks.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_device_entry_matches, same_bits
from grad_rule import REL, assert_candidate_rule as check_leading
from yfm_amd import _lib
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

sys.path.insert(0, str(GOLDEN / "msedn"))
sys.path.insert(0, str(GOLDEN / "msedn_grad"))
sys.path.insert(0, str(GOLDEN / "msedn_fullgrad"))
import make_msedn as MN  # noqa: E402
import make_msedn_fullgrad as MF  # noqa: E402
import make_msedn_grad as MG  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = MF.kinds()


@pytest.fixture(scope="module")
def cases():
    return MF.load_cases()


@pytest.fixture
def env():
    keys = ("YFM_MSED_LANES", "YFM_NNS_TRAJ_BYTES")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k in keys:
        os.environ.pop(k, None)
        if old[k] is not None:
            os.environ[k] = old[k]


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


@pytest.mark.parametrize("lanes", ["4", "16"])
@pytest.mark.parametrize("name", MF.case_names())
def test_full_gradient_matches_truth(engine, cases, env, name, lanes):
    """Every fixture case of every kind under both lane mappings, in the spaces stored: the rule above over the leading
    rows, the loss bitwise engine.loglik's, rows P−12 … bitwise engine.neural_loss_grad's, the −Inf count, nothing
    unavailable."""
    c = cases
    kind = kind_of(name)
    tu = c[f"{name}_T_use"]
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    os.environ["YFM_MSED_LANES"] = lanes
    for space in MF.case_spaces(name):
        Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
        loss, g = engine.neural_loss_full_grad(kind, Th, space=space, T_use=tu)
        thrown, neg_inf = engine.last_flags()
        unavailable = engine.last_grad_unavailable()
        g_fd = c[f"{name}_g_fd_s{space}"]
        assert thrown == 0 and neg_inf == int(np.isnan(g_fd).any(axis=0).sum()) and unavailable == 0
        assert g.shape == Th.shape
        assert same_bits(loss, engine.loglik(kind, Th, space=space, T_use=tu))
        _, g12 = engine.neural_loss_grad(kind, Th, space=space, T_use=tu)
        fin = np.isfinite(loss)
        assert same_bits(g[-12:, fin], g12[:, fin])
        assert np.isnan(g[:, ~fin]).all()
        check_leading(g, g_fd, c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space} L={lanes}")


@pytest.mark.parametrize("kind", KINDS)
def test_chain_rule_between_spaces(engine, cases, kind):
    """The unconstrained gradient is the constrained one with the rows of A multiplied by A, those of B by B(1 − B) and
    the diagonal of Φ by 2y/(1 + y)², y = eˣ; everything else is the identity.  The two θ differ by the rounding of the
    transforms, so the comparison is held to the project's bar, 1e-9 of ‖g‖∞ (and of the loss), not to bits."""
    name = f"k{kind}_n4t8"
    c = cases
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    Th, Tc = c[f"{name}_theta"], c[f"{name}_theta_c"]
    l0, g0 = engine.neural_loss_full_grad(kind, Th, space=0)
    l1, g1 = engine.neural_loss_full_grad(kind, Tc, space=1)
    np.testing.assert_allclose(l0, l1, rtol=REL)
    want = g1.copy()
    nu = 0 if kind in (P.KIND_NNS, P.KIND_NNS_ANCHORED) else (2, 6, 18)[kind & 3]
    want[:nu] *= Tc[:nu]
    if nu and not (kind >> 2) & 1:
        want[nu:2 * nu] *= Tc[nu:2 * nu] * (1 - Tc[nu:2 * nu])
    for d in (0, 4, 8):
        y = np.exp(Th[-9 + d])
        want[-9 + d] *= 2 * y / (1 + y) ** 2
    print("max |g0 - chain(g1)| / |g|inf", np.max(np.abs(g0 - want) / np.max(np.abs(want), axis=0)))
    assert np.all(np.abs(g0 - want) <= REL * np.max(np.abs(want), axis=0))


def _outputs(engine, kind, X, tu=None):
    loss, g = engine.neural_loss_full_grad(kind, X, space=0, T_use=tu)
    return np.vstack([loss[None, :], g])


@pytest.mark.parametrize("kind", KINDS)
def test_batch_lane_and_chunk_independence(engine, env, kind):
    """All P + 1 outputs of a candidate are the same bits alone, inside a batch of 70, with the batch reversed, with
    either lane count forced, and with the trajectory workspace capped so that the batch of 70 runs as five chunks of
    one block (N = 33, T = 40: more than one maturity per lane, two panel chunks; windows of every length)."""
    N, T = 33, 40
    engine.set_panel(MN.panel_for(N, T), MN.mats_for(N))
    Th = np.asfortranarray(MN.theta_for(kind, 0)[:, :70])
    tu = (T - np.arange(70) % 7).astype(np.int32)
    base = _outputs(engine, kind, Th, tu)
    assert base.shape == (Th.shape[0] + 1, 70) and np.all(np.isfinite(base[0]))
    assert np.isfinite(base).all(axis=0).sum() >= 35
    for b in (0, 33, 69):
        assert same_bits(_outputs(engine, kind, Th[:, b], tu[b:b + 1])[:, 0], base[:, b])
    assert same_bits(_outputs(engine, kind, np.asfortranarray(Th[:, ::-1]), tu[::-1].copy())[:, ::-1], base)
    for lanes in ("4", "16"):
        os.environ["YFM_MSED_LANES"] = lanes
        assert same_bits(_outputs(engine, kind, Th, tu), base)
    # the cap's floor is one block of candidates: 16 at L = 16, so 70 candidates are 5 launches of the two sweeps
    os.environ["YFM_MSED_LANES"] = "16"
    os.environ["YFM_NNS_TRAJ_BYTES"] = "1"
    assert same_bits(_outputs(engine, kind, Th, tu), base)
    assert same_bits(engine.neural_loss_full_grad(kind, Th, space=0, T_use=tu)[0],
                     engine.loglik(kind, Th, space=0, T_use=tu))
    assert engine.last_flags() == (0, 0)


def test_neg_inf_candidate_has_no_gradient(engine, cases):
    """Windows over a missing column: −Inf, P NaNs, counted by last_flags and not as unavailable; the short window
    beside them is finite."""
    for kind in KINDS:
        name = f"k{kind}_n4t8nan6"
        engine.set_panel(cases[f"{name}_Y"], cases[f"{name}_maturities"])
        loss, g = engine.neural_loss_full_grad(kind, cases[f"{name}_theta"], space=0, T_use=cases[f"{name}_T_use"])
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
        tu = np.array([1, 8], dtype=np.int32)
        loss, g = engine.neural_loss_full_grad(kind, Th, space=0, T_use=tu)
        assert same_bits(loss, engine.loglik(kind, Th, space=0, T_use=tu))
        assert np.all(g[:, 0] == 0.0) and np.all(np.isfinite(g[:, 1])) and np.any(g[:, 1] != 0.0)


def test_device_entry_point(engine):
    """The _device entry on a side stream equals the synchronous one bit for bit (windows of every length)."""
    N, T = 33, 8
    engine.set_panel(MN.panel_for(N, T), MN.mats_for(N))
    for kind in KINDS:
        Th = np.asfortranarray(MN.theta_for(kind, 0)[:, :70])
        tu = (np.arange(70) % 8 + 1).astype(np.int32)
        assert_device_entry_matches(engine.neural_loss_full_grad, engine.neural_loss_full_grad_device, kind, Th, tu,
                                    space=0)


def test_model_layer_and_unsupported_kinds(engine, cases):
    """compute_neural_loss_fullgrad_batch is the reference's sign (−loss, −gradient); the λ and Kalman kinds return −4
    from the C entry, and yfm_lambda_loss_fullgrad_batch keeps refusing the neural kinds."""
    name = "k32_n4t8"
    mats, Y, Th = cases[f"{name}_maturities"], cases[f"{name}_Y"], cases[f"{name}_theta"]
    model, _ = M.create_neural_model("1SD-NNS", mats, len(mats), 3)
    assert model.kind == 32
    f, g = M.compute_neural_loss_fullgrad_batch(model, Y, Th)
    loss, grad = engine.neural_loss_full_grad(32, Th, space=0)
    assert same_bits(f, -loss) and same_bits(g, -grad)
    assert same_bits(f, M.compute_loss_batch(model, Y, Th))
    mats30 = S.maturities_30()
    engine.set_panel(S.simulate_panel(P.KIND_DNS, 12, maturities=mats30), mats30)
    for kind in (P.KIND_DNS, P.KIND_TVL, P.KIND_GNS, P.KIND_NS, P.KIND_SD_NS, P.KIND_SSD_NS):
        with pytest.raises(_lib.YFMError) as e:
            engine.neural_loss_full_grad(kind, S.theta0(kind), space=0)
        assert e.value.code == -4, str(e.value)
    with pytest.raises(_lib.YFMError) as e:
        engine.lambda_loss_full_grad(32, S.theta0(32), space=0)
    assert e.value.code == -4


def test_scaled_zero_average_makes_the_gradient_unavailable(engine):
    """3SRWSD-NNS-Anchored at N = 5 on the δ/Φ fixture's candidates (found with the host form,
    tests/msedn_fullgrad_host_check.cpp, which reports them unavailable): the maturities 72 … 360 saturate hidden units,
    whose score components are exactly 0, so the root of their running average is 0 and the update's adjoint divides
    by it.  The loss stays finite (engine.loglik's) and neural_loss_grad has 12 finite rows, but all P rows are NaN —
    counted by last_grad_unavailable and not by last_flags."""
    c = MG.load_cases()
    name, kind = "k62_n5t8", 62
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    Th = c[f"{name}_theta"]
    loss, g = engine.neural_loss_full_grad(kind, Th, space=0)
    assert engine.last_flags() == (0, 0) and engine.last_grad_unavailable() == Th.shape[1]
    assert same_bits(loss, engine.loglik(kind, Th, space=0)) and np.isfinite(loss).all()
    _, g12 = engine.neural_loss_grad(kind, Th, space=0)
    assert np.isnan(g).all() and np.isfinite(g12).all()
