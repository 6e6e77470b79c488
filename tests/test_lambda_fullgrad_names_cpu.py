"""The λ models' full gradient's public names: include/yfm.h declares the two entry points, yfm_amd._lib binds them
with the argument lists of the δ/Φ pair, the ABI version stays 5 (the change is additive), and the model layer routes a
λ model's compute_loss_grad_batch to the full gradient, not to the Kalman kinds' loglik_grad (checked with a stub
engine: no device)."""
import inspect
import re

import numpy as np
import pytest

from conftest import ROOT
from yfm_amd import _lib, engine, groups, models
from yfm_amd import synthetic as S

NAMES = ("yfm_lambda_loss_fullgrad_batch", "yfm_lambda_loss_fullgrad_batch_device")


def test_header_declares_the_entry_points():
    h = (ROOT / "include" / "yfm.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    doc = h[h.index("with respect to EVERY row"):h.index("int yfm_lambda_loss_fullgrad_batch(")]
    for ref in ("filter.jl:209-243", "filter.jl:175", "optimization.jl:329-410", "yfm_last_batch_grad_unavailable"):
        assert ref in doc, ref
    assert "finite-difference" in doc  # says what the gradient is the derivative of
    assert "are not formed:" not in h  # the δ/Φ entry no longer says nobody forms the leading derivatives


def test_lib_binds_them_like_the_delta_phi_pair():
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "yfm_lambda_loss_grad_batch" in v)
    assert table["yfm_lambda_loss_fullgrad_batch"] == table["yfm_lambda_loss_grad_batch"]
    assert table["yfm_lambda_loss_fullgrad_batch_device"] == table["yfm_lambda_loss_grad_batch_device"]
    assert _lib.ABI_VERSION == 5


def test_engine_and_models_expose_the_feature():
    assert hasattr(engine.Engine, "lambda_loss_full_grad") and hasattr(engine.Engine, "lambda_loss_full_grad_device")
    assert callable(models.compute_lambda_loss_grad_batch)
    for fn in (models.estimate_steps_batch, models.estimate_steps_):
        par = inspect.signature(fn).parameters
        assert "full_gradient" in par and par["full_gradient"].default is False


class StubEngine:
    """Records which gradient method the model layer calls."""

    def __init__(self):
        self.calls = []

    def _answer(self, name, kind, theta, space, T_use):
        Th = np.asarray(theta, dtype=np.float64)
        Th = Th.reshape(Th.shape[0], -1)
        self.calls.append((name, kind, space, None if T_use is None else tuple(np.atleast_1d(T_use))))
        return np.full(Th.shape[1], 2.0), np.ones(Th.shape)

    def lambda_loss_full_grad(self, kind, theta, space=0, T_use=None):
        return self._answer("lambda_loss_full_grad", kind, theta, space, T_use)

    def loglik_grad(self, kind, theta, space=0, T_use=None):
        return self._answer("loglik_grad", kind, theta, space, T_use)

    def tvl_loglik_grad(self, kind, theta, space=0, T_use=None):
        return self._answer("tvl_loglik_grad", kind, theta, space, T_use)


@pytest.mark.parametrize("code,kind", [("NS", 3), ("SD-NS", 4), ("RWSD-NS", 5), ("SSD-NS", 6), ("SRWSD-NS", 8)])
def test_a_lambda_model_is_routed_to_the_full_gradient(monkeypatch, code, kind):
    stub = StubEngine()
    monkeypatch.setattr(models, "_engine", lambda model, data: stub)
    mats = np.array([3.0, 12.0, 60.0, 120.0])
    model, _ = models.create_model(code, mats, 4, 3)
    assert model.kind == kind
    Th = S.theta_batch(kind, 2, scale=0.1, seed=1, bad_frac=0.0)
    f, g = models.compute_loss_grad_batch(model, np.zeros((4, 8)), Th, T_use=[8, 5])
    assert stub.calls == [("lambda_loss_full_grad", kind, 0, (8, 5))]
    assert np.all(f == -2.0) and g.shape == Th.shape and np.all(g == -1.0)  # the reference's sign
    f, g = models.compute_lambda_loss_grad_batch(model, np.zeros((4, 8)), Th)
    assert stub.calls[-1] == ("lambda_loss_full_grad", kind, 0, None) and g.shape == Th.shape


def test_the_kalman_kinds_keep_their_routes(monkeypatch):
    stub = StubEngine()
    monkeypatch.setattr(models, "_engine", lambda model, data: stub)
    mats = S.maturities_30()
    dns, _ = models.create_model("1C", mats, 30, 3)
    models.compute_loss_grad_batch(dns, np.zeros((30, 8)), S.theta0(dns.kind))
    assert stub.calls[-1][0] == "loglik_grad"
    with pytest.raises(NotImplementedError):
        models.compute_lambda_loss_grad_batch(dns, np.zeros((30, 8)), S.theta0(dns.kind))


def test_check_groups_still_refuses_a_leading_parameter():
    with pytest.raises(NotImplementedError, match="leading"):
        groups.check_groups(["2"] * 15, 3)
    assert groups.check_groups(["2"] * 15, 0) == ["2"]
