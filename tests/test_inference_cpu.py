"""CPU tests of yfm_amd.inference: the covariance kinds and the delta method against numpy.linalg.inv on random
symmetric positive definite inputs, the not-positive-definite rule (NaN and pd = False, never an exception), and the
host mirror's refusals for the kinds without scores (checked with a stub engine: no device)."""
import numpy as np
import pytest

from yfm_amd import inference as INF
from yfm_amd import engine, models
from yfm_amd import synthetic as S
from yfm_amd.params import KIND_DNS, KIND_GNS, KIND_NNS, KIND_SD_NS, KIND_TVL, transform_params


def spd(rng, P, B):
    A = rng.standard_normal((P, P + 3, B))
    return np.einsum("ikb,jkb->ijb", A, A) + 0.1 * np.eye(P)[:, :, None]


def test_covariance_kinds_against_numpy_inverse():
    rng = np.random.default_rng(5)
    P, B = 20, 6
    nH, J = spd(rng, P, B), spd(rng, P, B)
    H = -nH
    for kind in INF.COV_KINDS:
        cov, pd = INF.covariance(H, J, kind)
        assert cov.shape == (P, P, B) and pd.all()
        for b in range(B):
            Hi = np.linalg.inv(H[:, :, b])
            ref = {"hessian": -Hi, "opg": np.linalg.inv(J[:, :, b]), "sandwich": Hi @ J[:, :, b] @ Hi}[kind]
            np.testing.assert_allclose(cov[:, :, b], ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max())
            np.testing.assert_array_equal(cov[:, :, b], cov[:, :, b].T)
    # a single matrix, and the matrix a kind does not use left out
    cov1, pd1 = INF.covariance(H[:, :, 0], None, "hessian")
    np.testing.assert_array_equal(cov1[:, :, 0], INF.covariance(H, J, "hessian")[0][:, :, 0])
    assert pd1.tolist() == [True] and INF.covariance(None, J, "opg")[1].all()
    with pytest.raises(ValueError):
        INF.covariance(H, None, "sandwich")
    with pytest.raises(ValueError):
        INF.covariance(H, J, "robust")


def test_a_matrix_that_is_not_positive_definite_gives_nan_not_an_exception():
    rng = np.random.default_rng(6)
    P, B = 5, 4
    nH, J = spd(rng, P, B), spd(rng, P, B)
    H = -nH
    H[:, :, 1] = -H[:, :, 1]          # a minimum, not a maximum
    H[:, :, 2] = np.nan               # an unavailable candidate
    J[:, :, 3] = np.diag([1.0, 1.0, 1.0, 1.0, -1.0])  # indefinite J
    cov, pd = INF.covariance(H, J, "hessian")
    assert pd.tolist() == [True, False, False, True]
    assert np.isnan(cov[:, :, 1:3]).all() and np.isfinite(cov[:, :, [0, 3]]).all()
    cov, pd = INF.covariance(H, J, "sandwich")
    assert pd.tolist() == [True, False, False, False] and np.isnan(cov[:, :, 1:]).all()
    cov, pd = INF.covariance(H, J, "opg")
    assert pd.tolist() == [True, True, True, False] and np.isnan(cov[:, :, 3]).all()
    singular = np.zeros((P, P, 1))
    assert INF.covariance(singular, singular, "sandwich")[1].tolist() == [False]


def test_delta_method_and_the_transform_jacobian():
    rng = np.random.default_rng(7)
    Th = S.theta_batch(KIND_DNS, 3, 0.1, 8, bad_frac=0)
    D = INF.transform_jacobian(KIND_DNS, Th)
    # the factors tests/test_grad_host_cpu.py::test_host_chain_rule lists: θ_c, (1 − θ_c²)/2, 1
    Tc = transform_params(KIND_DNS, Th)
    f = np.ones_like(Tc)
    f[[1, 2, 4, 7]] = Tc[[1, 2, 4, 7]]
    f[[11, 15, 19]] = (1.0 - Tc[[11, 15, 19]] ** 2) / 2.0
    np.testing.assert_allclose(D, f, rtol=1e-13)
    # … and a central difference of the transform itself
    h = 1e-6
    np.testing.assert_allclose(D, (transform_params(KIND_DNS, Th + h) - transform_params(KIND_DNS, Th - h)) / (2 * h),
                               rtol=1e-8)
    cov_u = spd(rng, 20, 3)
    cov_c = INF.delta_method(cov_u, D)
    for b in range(3):
        np.testing.assert_allclose(cov_c[:, :, b], np.diag(D[:, b]) @ cov_u[:, :, b] @ np.diag(D[:, b]), rtol=1e-14)
    with pytest.raises(NotImplementedError):
        INF.transform_jacobian(KIND_SD_NS, np.zeros(15))


class StubEngine:
    """Answers loglik_info with a fixed concave problem and records the call."""

    def __init__(self):
        self.calls = []

    def loglik_info(self, kind, theta, space=0, T_use=None, lags=0, step=None, hessian=True, opg=True):
        P, B = theta.shape
        self.calls.append(dict(kind=kind, space=space, T_use=T_use, lags=lags, step=step, hessian=hessian, opg=opg,
                               theta=theta.copy()))
        H = np.repeat(-2.0 * np.eye(P)[:, :, None], B, axis=2) if hessian else None
        J = np.repeat(3.0 * np.eye(P)[:, :, None], B, axis=2) if opg else None
        return dict(ll=np.full(B, 1.5), grad=np.zeros((P, B)), hess=H, opg=J)

    def last_grad_unavailable(self):
        return 0


def test_standard_errors_batch_evaluates_at_theta_u_and_applies_the_delta_method(monkeypatch):
    stub = StubEngine()
    monkeypatch.setattr(models, "_engine", lambda model, data: stub)
    mats = S.maturities_30()
    dns, _ = models.create_model("1C", mats, 30, 3)
    Th = S.theta_batch(KIND_DNS, 2, 0.1, 9, bad_frac=0)
    Tc = transform_params(KIND_DNS, Th)
    r = INF.standard_errors_batch(dns, np.zeros((30, 8)), Tc, T_use=[8, 5], cov="sandwich", lags=2, step=1e-3)
    call = stub.calls[-1]
    assert (call["space"], call["lags"], call["step"], call["hessian"], call["opg"]) == (0, 2, 1e-3, True, True)
    np.testing.assert_allclose(call["theta"], Th, rtol=1e-12, atol=1e-12)
    D = INF.transform_jacobian(KIND_DNS, call["theta"])
    np.testing.assert_allclose(r["se_u"], np.full((20, 2), np.sqrt(0.75)))  # H⁻¹ J H⁻¹ = 3/4 I
    np.testing.assert_allclose(r["se_c"], np.sqrt(0.75) * D)
    assert r["pd"].all() and r["unavailable"] == 0 and np.all(r["ll"] == 1.5)
    INF.standard_errors_batch(dns, np.zeros((30, 8)), Tc, cov="hessian")
    assert (stub.calls[-1]["hessian"], stub.calls[-1]["opg"]) == (True, False)
    INF.standard_errors_batch(dns, np.zeros((30, 8)), Tc, cov="opg")
    assert (stub.calls[-1]["hessian"], stub.calls[-1]["opg"]) == (False, True)
    one = INF.standard_errors_(dns, np.zeros((30, 8)), Tc[:, 0])
    assert one["se_c"].shape == (20,) and one["cov_c"].shape == (20, 20) and one["pd"] is True


@pytest.mark.parametrize("code", ["TVλ", "GNS5", "SD-NS", "NNS"])
def test_the_other_kinds_are_refused_by_the_host_mirror(monkeypatch, code):
    monkeypatch.setattr(models, "_engine", lambda model, data: pytest.fail("no launch for a refused kind"))
    mats = S.maturities_30()
    make = models.create_neural_model if code == "NNS" else models.create_model
    model, _ = make(code, mats, 30, 5 if code == "GNS5" else 3)
    assert model.kind in (KIND_TVL, KIND_GNS, KIND_SD_NS, KIND_NNS)
    with pytest.raises(NotImplementedError, match="DNS"):
        INF.standard_errors_batch(model, np.zeros((30, 8)), S.theta0(model.kind))
    eng = object.__new__(engine.Engine)  # no context: the refusal comes before any call into the library
    for call in (eng.loglik_scores, eng.loglik_info):
        with pytest.raises(NotImplementedError, match="DNS"):
            call(model.kind, S.theta0(model.kind))
    with pytest.raises(NotImplementedError, match="DNS"):
        eng.loglik_scores_device(model.kind, 0, 1, 1, 0, 0)
