"""GPU test of the batched DNS log-likelihood gradient (csrc/yfm_grad.hip through yfm_loglik_grad_batch).

The checker uses no derivative code: tests/golden/grad/grad_cases.npz holds fourth-order central differences
of the binary128 truth at two steps (make_grad.py), g_fd and the bound e_fd of its own error.  Per case and
compared candidate (every truth evaluation finite, e_fd ≤ 1e-9·‖g_fd‖∞; at least 75% of a case):

    max_i |g_gpu − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]

(1e-9: the project's parity bar, norm-wise); gradients that are exactly zero (T_use ≤ 2) must be 0.0.  The
logliks pass test_gpu_parity.assert_parity against the fixture's dense oracle and truth.

Observed on MI355X (largest |g_gpu − g_fd| / (1e-9·‖g_fd‖∞ + e_fd) and / ‖g_fd‖∞ over the compared): see
DESIGN.md §3.5.
References: optimization.jl:367 (the ForwardDiff gradient of compute_loss), filter.jl:182-209.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_batch_independent, assert_device_entry_matches
from grad_rule import REL, assert_gradient_rule, bad_sigma, chain_factor, collinear
from test_gpu_parity import assert_parity
from yfm_amd import KIND_DNS, KIND_GNS, KIND_TVL, _lib
from yfm_amd import synthetic as S
from yfm_amd.params import n_params, transform_params

sys.path.insert(0, str(GOLDEN / "grad"))
import make_grad as MG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


@pytest.mark.parametrize("name", MG.CASE_NAMES)
def test_gradient_matches_truth_differences(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    ll, g = engine.loglik_grad(KIND_DNS, c["Theta"], space=0, T_use=c["T_use"])
    assert_gradient_rule(g, c, label=f"case {name}", short_windows_zero=name == "A-windows")
    if name == "A-windows":
        assert int((c["T_use"] <= 2).sum()) == 28
    assert_parity(ll, c["loglik_oracle"], c["loglik_truth"])
    assert engine.last_grad_unavailable() == 0


def test_chain_rule_between_the_spaces(engine, cases):
    """grad(space 0, θ) = grad(space 1, θ_c) · dθ_c/dθ: θ_c for the exp entries, (1 − θ_c²)/2 on the Φ diagonal."""
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"][:, :16]
    Tc = transform_params(KIND_DNS, Th)
    ll0, g0 = engine.loglik_grad(KIND_DNS, Th, space=0)
    ll1, g1 = engine.loglik_grad(KIND_DNS, Tc, space=1)
    f = chain_factor(KIND_DNS, Tc)
    np.testing.assert_allclose(ll0, ll1, rtol=1e-12)  # (the host's exp and the device's differ in the last bit)
    assert np.all(np.abs(g0 - g1 * f).max(axis=0) <= REL * np.abs(g0).max(axis=0))


def test_patterns(engine, cases):
    c = cases["A"]
    Y, m = c["Y"], c["maturities"]
    engine.set_panel(Y, m)
    good = c["Theta"][:, 0]
    # −Inf loglik: NaN gradient, counted in n_neg_inf
    ll, g = engine.loglik_grad(KIND_DNS, np.stack([good, bad_sigma(KIND_DNS, good)], axis=1))
    assert np.isfinite(ll[0]) and np.isfinite(g[:, 0]).all()
    assert np.isneginf(ll[1]) and np.isnan(g[:, 1]).all()
    assert engine.last_flags() == (0, 1) and engine.last_grad_unavailable() == 0
    # the reference would throw in initialize_filter (constrained Φ = I): NaN loglik and gradient
    tc = transform_params(KIND_DNS, good)
    tc[11:20] = np.eye(3).reshape(-1)
    ll, g = engine.loglik_grad(KIND_DNS, tc, space=1)
    assert np.isnan(ll[0]) and np.isnan(g).all()
    assert engine.last_flags()[0] == 1
    # deferral class (γ = 5: exactly collinear loadings): the loglik of engine.loglik, NaN gradient, counted
    Thd = np.stack([good, collinear(good), collinear(c["Theta"][:, 1])], axis=1)
    ll, g = engine.loglik_grad(KIND_DNS, Thd)
    assert engine.last_grad_unavailable() == 2 == engine.last_deferred()
    np.testing.assert_array_equal(ll, engine.loglik(KIND_DNS, Thd))
    assert np.isfinite(g[:, 0]).all() and np.isnan(g[:, 1:]).all()
    # … and an N = 2 panel (fewer maturities than states)
    engine.set_panel(Y[:2], m[:2])
    Th4 = c["Theta"][:, :4]
    ll, g = engine.loglik_grad(KIND_DNS, Th4)
    assert engine.last_grad_unavailable() == 4 == engine.last_deferred()
    np.testing.assert_array_equal(ll, engine.loglik(KIND_DNS, Th4))
    assert np.isnan(g).all()


def test_unsupported_requests(engine, cases):
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    for kind in (KIND_TVL, KIND_GNS):
        with pytest.raises(_lib.YFMError) as e:
            engine.loglik_grad(kind, S.theta_batch(kind, 2, seed=3, bad_frac=0))
        assert e.value.code == -4 and "DNS" in str(e.value)
    m65 = np.linspace(3, 360, 65)
    engine.set_panel(S.simulate_panel(KIND_DNS, 8, m65, 3), m65)
    with pytest.raises(_lib.YFMError) as e:
        engine.loglik_grad(KIND_DNS, c["Theta"][:, :2])
    assert e.value.code == -4 and "65" in str(e.value)
    assert np.isfinite(engine.loglik(KIND_DNS, c["Theta"][:, :2])).all()  # the value itself is supported


def test_outputs_do_not_depend_on_the_batch(engine, cases):
    """Case A's good candidates interleaved with the pattern candidates, reversed, and alone (B = 1): bitwise
    the same loglik and gradient per candidate."""
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    good = c["Theta"][:, c["compared"]][:, :14]
    cols, pos = [], []
    for k in range(good.shape[1]):
        pos.append(len(cols))
        cols.append(good[:, k])
        if k % 3 == 0:
            cols.append(bad_sigma(KIND_DNS, good[:, k]))
        if k % 5 == 0:
            cols.append(collinear(good[:, k]))
    Th = np.asfortranarray(np.stack(cols, axis=1))
    # and inside the 70-candidate batch of the fixture (three workgroups, a ragged tail)
    idx = np.flatnonzero(c["compared"])[:14]
    ll, g = assert_batch_independent(lambda X: engine.loglik_grad(KIND_DNS, X), Th, range(Th.shape[1]),
                                     inside=(c["Theta"], idx, pos))
    assert np.isfinite(g).all(axis=0).sum() == good.shape[1]


def test_device_entry_point_on_a_torch_stream(engine, cases):
    c = cases["A-windows"]
    engine.set_panel(c["Y"], c["maturities"])
    assert_device_entry_matches(engine.loglik_grad, engine.loglik_grad_device, KIND_DNS, c["Theta"], c["T_use"])
    assert engine.last_grad_unavailable() == 0
    assert n_params(KIND_DNS) == c["Theta"].shape[0]
