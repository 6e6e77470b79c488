"""Host mirror of the λ models (yfm_amd.params / yfm_amd.models): layouts, transforms, create_model codes and
parameter groups — no GPU."""
from __future__ import annotations

import numpy as np
import pytest

import msed_reference as R
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

KINDS = P.LAMBDA_KINDS


def test_kind_values_and_counts():
    assert KINDS == (3, 4, 5, 6, 8) == R.KINDS
    assert [P.n_params(k) for k in KINDS] == [13, 15, 14, 15, 14]
    assert all(P.state_dim(k) == 3 and P.gamma_dim(k) == 1 for k in KINDS)
    # the three existing kinds keep theirs
    assert [P.n_params(k) for k in (0, 1, 2)] == [20, 31, 48]


@pytest.mark.parametrize("kind", KINDS)
def test_transforms_round_trip(kind):
    rng = np.random.default_rng(kind)
    th = S.theta0(kind)[:, None] + 0.3 * rng.standard_normal((P.n_params(kind), 5))
    tc = P.transform_params(kind, th)
    np.testing.assert_allclose(P.untransform_params(kind, tc), th, rtol=0, atol=1e-12)
    # the maps, entry by entry: A → exp, B → 1/(1 + e^−x), the diagonal of Φ → 2eˣ/(1 + eˣ) − 1, the rest identity
    lay = P.lambda_layout(kind)
    codes = P.transform_codes(kind)
    assert len(codes) == lay.P
    for i in range(lay.P):
        x = th[i]
        want = {P.ID: x, P.POS: np.exp(x), P.U01: 1 / (1 + np.exp(-x)), P.R11: 2 * np.exp(x) / (1 + np.exp(x)) - 1}[codes[i]]
        np.testing.assert_array_equal(tc[i], want)
    assert [int(c) for c in codes[lay.phi_offset:]] == [P.R11, 0, 0, 0, P.R11, 0, 0, 0, P.R11]
    assert [int(c) for c in codes[:lay.n_lead]] == ([] if kind == 3 else [P.POS, P.U01] if P.lambda_has_b(kind) else [P.POS])
    # and they are the restatement's
    for b in range(5):
        np.testing.assert_allclose(R.transform_params(kind, th[:, b]), tc[:, b], rtol=1e-15)


@pytest.mark.parametrize("kind", KINDS)
def test_phi_is_column_major(kind):
    lay = P.lambda_layout(kind)
    th = S.theta0_constrained(kind)
    th[lay.phi_offset + 1] = 0.123  # the second entry of vec Φ is Φ[2, 1] (reshape), not Φ[1, 2]
    m = R.set_params(kind, th, S.maturities_30())
    assert m.Phi[1, 0] == 0.123 and m.Phi[0, 1] != 0.123
    # θ₀ carries the DNS Φ, whose own layout is row-major
    dns = S.theta0_constrained(P.KIND_DNS)
    phi = dns[P.param_layout(P.KIND_DNS).phi_offset:].reshape(3, 3)
    np.testing.assert_array_equal(R.set_params(kind, S.theta0_constrained(kind), S.maturities_30()).Phi, phi)


def test_theta0_values():
    th = S.theta0_constrained(P.KIND_SD_NS)
    assert th[0] == 1e-3 and th[1] == 0.98 and th[2] == np.log(0.0609 - 0.01)
    assert S.theta0_constrained(P.KIND_RWSD_NS)[1] == np.log(0.0609 - 0.01)
    assert S.theta0_constrained(P.KIND_NS)[0] == np.log(0.0609 - 0.01)


CODES = {"NS": ("NS", 3), "2": ("NS", 3), "SD-NS": ("SD-NS", 4), "4": ("SD-NS", 4), "RWSD-NS": ("RWSD-NS", 5),
         "5": ("RWSD-NS", 5), "SSD-NS": ("SSD-NS", 6), "6": ("SSD-NS", 6), "SRWSD-NS": ("SRWSD-NS", 8),
         "7": ("SRWSD-NS", 8)}


@pytest.mark.parametrize("code", sorted(CODES))
def test_create_model_maps_the_code(code):
    mats = S.maturities_30()
    model, std = M.create_model(code, mats, 30, 3)
    assert std == CODES[code][0]
    assert model.kind == CODES[code][1]
    assert model.base.model_string == code  # model_dictionary.jl passes the caller's string on
    assert model.base.M == 3 and model.base.L == 1 and model.base.N == 30
    if model.kind == 3:
        assert isinstance(model, M.StaticLambdaModel)
    else:
        assert isinstance(model, M.MSEDLambdaModel)
        assert model.random_walk == (model.kind in (5, 8)) and model.scale_grad == (model.kind in (6, 8))
    M.set_params_(model, S.theta0_constrained(model.kind))
    np.testing.assert_array_equal(M.get_params(model), S.theta0_constrained(model.kind))
    with pytest.raises(ValueError):
        M.set_params_(model, np.zeros(20))


def test_other_codes_still_raise():
    for code in ("NNS", "3", "8", "RW", "1SD-NNS"):
        with pytest.raises(ValueError):
            M.create_model(code, S.maturities_30(), 30, 3)
    # and the Kalman codes still map
    assert M.create_model("1C", S.maturities_30(), 30, 3)[1] == "1C"


def test_param_groups_defaults():
    for code, n1 in (("NS", 1), ("SD-NS", 3), ("RWSD-NS", 2), ("SSD-NS", 3), ("SRWSD-NS", 2)):
        model, _ = M.create_model(code, S.maturities_30(), 30, 3)
        assert M.get_param_groups(model, []) == ["1"] * n1 + ["2"] * 12
        mine = [str(i % 4) for i in range(P.n_params(model.kind))]
        assert M.get_param_groups(model, mine) == mine
        assert M.get_param_groups(model, mine[:-1]) == ["1"] * n1 + ["2"] * 12


def test_synthetic_draws():
    """The λ branches of synthetic.py draw as the existing kinds do and leave those alone (bench.py and the existing
    tests use them): θ₀ + scale·N(0, I) from PCG64(seed), the DNS panel."""
    for kind in (P.KIND_DNS, P.KIND_SD_NS, P.KIND_NS):
        rng = np.random.Generator(np.random.PCG64(3))
        want = S.theta0(kind)[:, None] + 0.1 * rng.standard_normal((P.n_params(kind), 16))
        np.testing.assert_array_equal(S.theta_batch(kind, 16, seed=3, bad_frac=0.0), want)
    np.testing.assert_array_equal(S.simulate_panel(P.KIND_SD_NS, 12), S.simulate_panel(P.KIND_DNS, 12))
