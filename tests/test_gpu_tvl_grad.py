"""GPU test of the batched TVλ log-likelihood gradient (csrc/yfm_tvl_grad.hip through yfm_tvl_loglik_grad_batch).

The checker uses no derivative code: tests/golden/tvl_grad/tvl_grad_cases.npz holds fourth-order central
differences of the binary128 truth on a ladder of steps (make_tvl_grad.py), g_fd and the bound e_fd of its own
error.  Per case and compared candidate (every truth evaluation finite, e_fd ≤ 1e-9·‖g_fd‖∞, the dense FP64 oracle
within 1e-9 of the truth; at least 75% of a case):

    max_i |g_gpu − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]

(1e-9: the project's parity bar, norm-wise); gradients that are exactly zero (T_use ≤ 2) must be 0.0.  The
logliks pass test_gpu_parity.assert_parity against the fixture's dense oracle and truth.
References: optimization.jl:367 (the ForwardDiff gradient of compute_loss), filter.jl:12-80, :182-209.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_batch_independent, assert_device_entry_matches
from grad_rule import REL, assert_gradient_rule, bad_sigma, chain_factor
from test_gpu_parity import assert_parity
from yfm_amd import KIND_DNS, KIND_GNS, KIND_NS, KIND_TVL, _lib
from yfm_amd import synthetic as S
from yfm_amd.params import n_params, transform_params

sys.path.insert(0, str(GOLDEN / "tvl_grad"))
import make_tvl_grad as MG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


@pytest.mark.parametrize("name", MG.CASE_NAMES)
def test_gradient_matches_truth_differences(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    ll, g = engine.tvl_loglik_grad(KIND_TVL, c["Theta"], space=0, T_use=c["T_use"])
    assert_gradient_rule(g, c, label=f"case {name}", short_windows_zero=name == "A-windows")
    if name == "A-windows":
        assert int((c["T_use"] <= 2).sum()) == 10
        assert np.all(ll[c["T_use"] <= 2] == 0.0)
    assert_parity(ll, c["loglik_oracle"], c["loglik_truth"])
    assert engine.last_grad_unavailable() == 0


def test_chain_rule_between_the_spaces(engine, cases):
    """grad(space 0, θ) = grad(space 1, θ_c) · dθ_c/dθ: θ_c for the exp entries, (1 − θ_c²)/2 on the Φ diagonal."""
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"][:, :16]
    Tc = transform_params(KIND_TVL, Th)
    ll0, g0 = engine.tvl_loglik_grad(KIND_TVL, Th, space=0)
    ll1, g1 = engine.tvl_loglik_grad(KIND_TVL, Tc, space=1)
    f = chain_factor(KIND_TVL, Tc)
    np.testing.assert_allclose(ll0, ll1, rtol=1e-12)  # (the host's exp and the device's differ in the last bit)
    assert np.all(np.abs(g0 - g1 * f).max(axis=0) <= REL * np.abs(g0).max(axis=0))


def test_gradient_is_the_same_under_both_precisions(engine, cases):
    """The value follows the context's precision (bitwise engine.loglik under the same setting); the gradient is
    the FP64 tangent recursion either way, bit for bit."""
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    old = engine.precision
    out = {}
    try:
        for mode in (_lib.PREC_CERTIFIED, _lib.PREC_FP64):
            engine.precision = mode
            ll, g = engine.tvl_loglik_grad(KIND_TVL, c["Theta"])
            np.testing.assert_array_equal(ll, engine.loglik(KIND_TVL, c["Theta"]))
            out[mode] = g
    finally:
        engine.precision = old
    np.testing.assert_array_equal(out[_lib.PREC_CERTIFIED], out[_lib.PREC_FP64])


def test_patterns(engine, cases):
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    good = c["Theta"][:, np.flatnonzero(c["compared"])[0]]
    # −Inf loglik: NaN gradient, counted in n_neg_inf
    ll, g = engine.tvl_loglik_grad(KIND_TVL, np.stack([good, bad_sigma(KIND_TVL, good)], axis=1))
    assert np.isfinite(ll[0]) and np.isfinite(g[:, 0]).all()
    assert np.isneginf(ll[1]) and np.isnan(g[:, 1]).all()
    assert engine.last_flags() == (0, 1)
    # the reference would throw in initialize_filter (constrained Φ = I): NaN loglik and gradient
    tc = transform_params(KIND_TVL, good)
    tc[15:31] = np.eye(4).reshape(-1)
    ll, g = engine.tvl_loglik_grad(KIND_TVL, tc, space=1)
    assert np.isnan(ll[0]) and np.isnan(g).all()
    assert engine.last_flags()[0] == 1
    # λ overflow (the committed edge candidate): its gradient column is NaN, its neighbours' are finite
    with np.load(GOLDEN / "edge" / "tvl_lambda_overflow.npz", allow_pickle=False) as z:
        Yo, mo, tho = np.asfortranarray(z["Y"]), z["maturities"], z["Theta"][:, 0]
    engine.set_panel(Yo, mo)
    nb = S.theta_batch(KIND_TVL, 2, 0.02, 11, bad_frac=0)
    ll, g = engine.tvl_loglik_grad(KIND_TVL, np.stack([nb[:, 0], tho, nb[:, 1]], axis=1))
    assert np.isnan(g[:, 1]).all()
    assert np.isfinite(g[:, [0, 2]]).all() and np.isfinite(ll[[0, 2]]).all()
    assert engine.last_grad_unavailable() == (1 if np.isfinite(ll[1]) else 0)


def test_refusals(engine, cases):
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    for kind in (KIND_DNS, KIND_GNS, KIND_NS):
        with pytest.raises(_lib.YFMError) as e:
            engine.tvl_loglik_grad(kind, S.theta_batch(kind, 2, seed=3, bad_frac=0))
        assert e.value.code == -4


def test_outputs_do_not_depend_on_the_batch(engine, cases):
    """Case A's compared candidates interleaved with pattern candidates, reversed, alone (B = 1) and inside the
    fixture's 24-batch: bitwise the same loglik and gradient per candidate."""
    c = cases["A"]
    engine.set_panel(c["Y"], c["maturities"])
    idx = np.flatnonzero(c["compared"])[:10]
    good = c["Theta"][:, idx]
    cols, pos = [], []
    for k in range(good.shape[1]):
        pos.append(len(cols))
        cols.append(good[:, k])
        if k % 3 == 0:
            cols.append(bad_sigma(KIND_TVL, good[:, k]))
    Th = np.asfortranarray(np.stack(cols, axis=1))
    ll, g = assert_batch_independent(lambda X: engine.tvl_loglik_grad(KIND_TVL, X), Th, pos,
                                     inside=(c["Theta"], idx, pos))
    assert np.isfinite(g).all(axis=0).sum() == good.shape[1]


def test_device_entry_point_on_a_torch_stream(engine, cases):
    c = cases["A-windows"]
    engine.set_panel(c["Y"], c["maturities"])
    assert_device_entry_matches(engine.tvl_loglik_grad, engine.tvl_loglik_grad_device, KIND_TVL, c["Theta"], c["T_use"])
    assert engine.last_grad_unavailable() == 0
    assert n_params(KIND_TVL) == c["Theta"].shape[0] == 31
