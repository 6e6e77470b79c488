"""The neural models' full gradient's public names: include/yfm.h declares the two entry points, the library exports
them at ABI version 5, yfm_amd._lib binds them with the argument lists of the λ pair, the Julia shim has the call, the
engine and the model layer expose the feature under names of the neural models' own, those names refuse λ and Kalman
models, and estimate_neural_steps_batch still refuses an L-BFGS group with a leading parameter unless
full_gradient=True is passed."""
from __future__ import annotations

import inspect
import re

import numpy as np
import pytest

import yfm_amd
from conftest import ROOT
from yfm_amd import _lib, engine as E, models as M, synthetic as S

NAMES = ("yfm_neural_loss_fullgrad_batch", "yfm_neural_loss_fullgrad_batch_device")


def test_header_declares_the_entry_points():
    h = (ROOT / "include" / "yfm.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    doc = h[h.index("The neural kinds' loss WITH its gradient"):h.index("int yfm_neural_loss_fullgrad_batch(")]
    for ref in ("filter.jl:209-243", "filter.jl:175", "yfm_last_batch_grad_unavailable", "YFM_NNS_TRAJ_BYTES",
                "finite-difference", "512"):
        assert ref in doc, ref


def test_library_exports_them_at_abi_5():
    lib = _lib.load()
    assert lib.yfm_abi_version() == 5 == _lib.ABI_VERSION
    for n in NAMES:
        assert hasattr(lib, n), n


def test_lib_binds_them_like_the_lambda_pair():
    for n in NAMES:
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n.replace("neural", "lambda")]


def test_julia_shim_and_integration_notes_have_the_call():
    jl = (ROOT / "yieldfactormodels.jl_amd" / "julia" / "YFMAMD.jl").read_text()
    assert "@ccall LIB.yfm_neural_loss_fullgrad_batch(" in jl and "function neural_loss_fullgrad_batch(" in jl
    assert "YFMAMD.neural_loss_fullgrad_batch(" in (ROOT / "INTEGRATION.md").read_text()


def test_engine_and_models_expose_the_feature():
    assert callable(E.Engine.neural_loss_full_grad) and callable(E.Engine.neural_loss_full_grad_device)
    for name in ("compute_neural_loss_fullgrad_batch", "estimate_neural_lbfgs_batch", "estimate_neural_"):
        assert name in yfm_amd.__all__ and callable(getattr(yfm_amd, name)), name
    par = inspect.signature(M.estimate_neural_steps_batch).parameters
    assert "full_gradient" in par and par["full_gradient"].default is False
    assert inspect.signature(M.estimate_neural_lbfgs_batch).parameters.keys() == \
        inspect.signature(M.estimate_lbfgs_batch).parameters.keys()
    assert inspect.signature(M.estimate_neural_).parameters.keys() == inspect.signature(M.estimate_).parameters.keys()


def test_new_names_refuse_lambda_and_kalman_models():
    mats = S.maturities_30()
    Y = np.zeros((30, 8))
    for code in ("SD-NS", "1C"):
        m, _ = M.create_model(code, mats, 30, 3)
        th = S.theta0_constrained(m.kind)
        for call in (lambda: M.compute_neural_loss_fullgrad_batch(m, Y, th[:, None]),
                     lambda: M.estimate_neural_lbfgs_batch(m, Y, th[:, None]),
                     lambda: M.estimate_neural_(m, Y, th[:, None])):
            with pytest.raises(NotImplementedError):
                call()


class StubEngine:
    """Records which gradient method the model layer calls."""

    def __init__(self):
        self.calls = []

    def neural_loss_full_grad(self, kind, theta, space=0, T_use=None):
        Th = np.asarray(theta, dtype=np.float64)
        Th = Th.reshape(Th.shape[0], -1)
        self.calls.append(("neural_loss_full_grad", kind, space, None if T_use is None else tuple(np.atleast_1d(T_use))))
        return np.full(Th.shape[1], 2.0), np.ones(Th.shape)


def test_a_neural_model_is_routed_to_the_full_gradient(monkeypatch):
    stub = StubEngine()
    monkeypatch.setattr(M, "_engine", lambda model, data: stub)
    mats = S.maturities_30()
    m, _ = M.create_neural_model("1SD-NNS", mats, 30, 3)
    Th = S.theta_batch(m.kind, 2, scale=0.1, seed=1, bad_frac=0.0)
    f, g = M.compute_neural_loss_fullgrad_batch(m, np.zeros((30, 8)), Th, T_use=[8, 5])
    assert stub.calls == [("neural_loss_full_grad", m.kind, 0, (8, 5))]
    assert np.all(f == -2.0) and g.shape == Th.shape and np.all(g == -1.0)  # the reference's sign


def test_old_names_and_the_default_keep_refusing():
    mats = S.maturities_30()
    Y = np.zeros((30, 8))
    m, _ = M.create_neural_model("NNS", mats, 30, 3)
    tn = S.theta0_constrained(m.kind)
    with pytest.raises(NotImplementedError, match="leading"):
        M.estimate_neural_steps_batch(m, Y, tn[:, None], param_groups=["2"] * 30)
    for call in (lambda: M.estimate_(m, Y, tn[:, None]), lambda: M.estimate_lbfgs_batch(m, Y, tn[:, None])):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "neural" in str(e.value) and "not built" in str(e.value)
        assert "estimate_neural_lbfgs_batch" in str(e.value)
