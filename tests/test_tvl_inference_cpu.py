"""CPU test of yfm_amd.inference.tvl_standard_errors_batch on a stub engine, as tests/test_inference_cpu.py does for
DNS: the call reaches Engine.tvl_loglik_info at θ_u with the hessian / opg flags of the covariance kind, the delta
method uses the TVλ transform's Jacobian, and other kinds are refused before any launch."""
from __future__ import annotations

import numpy as np
import pytest

from yfm_amd import engine, models
from yfm_amd import inference as INF
from yfm_amd import synthetic as S
from yfm_amd.params import KIND_DNS, KIND_GNS, KIND_NNS, KIND_SD_NS, KIND_TVL, transform_params


class StubEngine:
    """Answers tvl_loglik_info with a fixed concave problem and records the call; has no loglik_info at all."""

    def __init__(self):
        self.calls = []

    def tvl_loglik_info(self, kind, theta, space=0, T_use=None, lags=0, step=None, hessian=True, opg=True):
        P, B = theta.shape
        self.calls.append(dict(kind=kind, space=space, T_use=T_use, lags=lags, step=step, hessian=hessian, opg=opg,
                               theta=theta.copy()))
        H = np.repeat(-2.0 * np.eye(P)[:, :, None], B, axis=2) if hessian else None
        J = np.repeat(3.0 * np.eye(P)[:, :, None], B, axis=2) if opg else None
        return dict(ll=np.full(B, 1.5), grad=np.zeros((P, B)), hess=H, opg=J)

    def last_grad_unavailable(self):
        return 0


def test_the_tvl_transform_jacobian():
    Th = S.theta_batch(KIND_TVL, 3, 0.02, 8, bad_frac=0)
    D = INF.transform_jacobian(KIND_TVL, Th)
    # csrc/yfm_tvl_grad.hpp chain_factor: θ_c for σ² and the diagonal of U, (1 − θ_c²)/2 for the diagonal of Φ, 1 elsewhere
    Tc = transform_params(KIND_TVL, Th)
    f = np.ones_like(Tc)
    pos, r11 = [0, 1, 3, 6, 10], [15, 20, 25, 30]
    f[pos] = Tc[pos]
    f[r11] = (1.0 - Tc[r11] ** 2) / 2.0
    np.testing.assert_allclose(D, f, rtol=1e-13)
    h = 1e-6
    np.testing.assert_allclose(D, (transform_params(KIND_TVL, Th + h) - transform_params(KIND_TVL, Th - h)) / (2 * h),
                               rtol=1e-8)


def test_tvl_standard_errors_batch_evaluates_at_theta_u_and_applies_the_delta_method(monkeypatch):
    stub = StubEngine()
    monkeypatch.setattr(models, "_engine", lambda model, data: stub)
    mats = S.maturities_30()
    tvl, _ = models.create_model("TVλ", mats, 30, 3)
    assert tvl.kind == KIND_TVL
    Th = S.theta_batch(KIND_TVL, 2, 0.02, 9, bad_frac=0)
    Tc = transform_params(KIND_TVL, Th)
    r = INF.tvl_standard_errors_batch(tvl, np.zeros((30, 8)), Tc, T_use=[8, 5], cov="sandwich", lags=2, step=1e-3)
    call = stub.calls[-1]
    assert (call["kind"], call["space"], call["lags"], call["step"], call["hessian"], call["opg"]) == \
        (KIND_TVL, 0, 2, 1e-3, True, True)
    assert call["T_use"] == [8, 5]
    np.testing.assert_allclose(call["theta"], Th, rtol=1e-12, atol=1e-12)
    D = INF.transform_jacobian(KIND_TVL, call["theta"])
    np.testing.assert_allclose(r["se_u"], np.full((31, 2), np.sqrt(0.75)))  # H⁻¹ J H⁻¹ = 3/4 I
    np.testing.assert_allclose(r["se_c"], np.sqrt(0.75) * D)
    assert set(r) == {"cov_u", "se_u", "cov_c", "se_c", "ll", "grad", "pd", "unavailable"}
    assert r["pd"].all() and r["unavailable"] == 0 and np.all(r["ll"] == 1.5)
    INF.tvl_standard_errors_batch(tvl, np.zeros((30, 8)), Tc, cov="hessian")
    assert (stub.calls[-1]["hessian"], stub.calls[-1]["opg"]) == (True, False)
    INF.tvl_standard_errors_batch(tvl, np.zeros((30, 8)), Tc, cov="opg")
    assert (stub.calls[-1]["hessian"], stub.calls[-1]["opg"]) == (False, True)
    one = INF.tvl_standard_errors_(tvl, np.zeros((30, 8)), Tc[:, 0])
    assert one["se_c"].shape == (31,) and one["cov_c"].shape == (31, 31) and one["pd"] is True
    with pytest.raises(ValueError):
        INF.tvl_standard_errors_batch(tvl, np.zeros((30, 8)), Tc, cov="robust")


@pytest.mark.parametrize("code", ["1C", "GNS5", "SD-NS", "NNS"])
def test_the_other_kinds_are_refused_by_the_tvl_host_mirror(monkeypatch, code):
    monkeypatch.setattr(models, "_engine", lambda model, data: pytest.fail("no launch for a refused kind"))
    mats = S.maturities_30()
    make = models.create_neural_model if code == "NNS" else models.create_model
    model, _ = make(code, mats, 30, 5 if code == "GNS5" else 3)
    assert model.kind in (KIND_DNS, KIND_GNS, KIND_SD_NS, KIND_NNS)
    with pytest.raises(NotImplementedError, match="TVλ"):
        INF.tvl_standard_errors_batch(model, np.zeros((30, 8)), S.theta0(model.kind))
    eng = object.__new__(engine.Engine)  # no context: the refusal comes before any call into the library
    for call in (eng.tvl_loglik_scores, eng.tvl_loglik_info):
        with pytest.raises(NotImplementedError, match="TVλ"):
            call(model.kind, S.theta0(model.kind))
    with pytest.raises(NotImplementedError, match="TVλ"):
        eng.tvl_loglik_scores_device(model.kind, 0, 1, 1, 0, 0)
