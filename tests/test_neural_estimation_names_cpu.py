"""The neural models' estimation is served under names of its own: they exist and are exported, the names the λ and
Kalman models use keep refusing a neural model (and now say where to go), and the library still answers ABI version 5
with the two additive symbols present."""
from __future__ import annotations

import re

import numpy as np
import pytest

import yfm_amd
from conftest import ROOT
from yfm_amd import _lib, driver as D, engine as E, forecasting as F, models as M, synthetic as S


def test_new_names_exist_and_are_exported():
    for name in ("compute_neural_loss_grad_block", "estimate_neural_steps_", "estimate_neural_steps_batch",
                 "run_neural_estimation_"):
        assert name in yfm_amd.__all__ and callable(getattr(yfm_amd, name)), name
    assert yfm_amd.run_neural_estimation_ is D.run_neural_estimation_
    assert callable(E.Engine.neural_loss_grad) and callable(E.Engine.neural_loss_grad_device)
    for sym in ("yfm_neural_loss_grad_batch", "yfm_neural_loss_grad_batch_device"):
        assert _lib.SIGNATURES[sym] == _lib.SIGNATURES[sym.replace("neural", "lambda")]
    jl = (ROOT / "yieldfactormodels.jl_amd" / "julia" / "YFMAMD.jl").read_text()
    assert "yfm_neural_loss_grad_batch" in jl and "neural_loss_grad_batch" in jl


def test_library_has_the_symbols_at_abi_5():
    lib = _lib.load()
    assert lib.yfm_abi_version() == 5 == _lib.ABI_VERSION
    assert hasattr(lib, "yfm_neural_loss_grad_batch") and hasattr(lib, "yfm_neural_loss_grad_batch_device")
    txt = (ROOT / "include" / "yfm.h").read_text()
    assert re.search(r"#define YFM_ABI_VERSION 5\b", txt)
    assert "int yfm_neural_loss_grad_batch(" in txt and "int yfm_neural_loss_grad_batch_device(" in txt


def test_old_names_refuse_and_point_to_the_new_ones():
    mats = S.maturities_30()
    Y = np.zeros((30, 8))
    m, _ = M.create_neural_model("1SD-NNS", mats, 30, 3)
    th = S.theta0_constrained(m.kind)
    for call, where in ((lambda: M.estimate_steps_(m, Y, th[:, None]), "estimate_neural_steps_"),
                        (lambda: M.estimate_steps_batch(m, Y, th[:, None]), "estimate_neural_steps_batch"),
                        (lambda: M.compute_loss_grad_block(m, Y, th[:, None]), "compute_neural_loss_grad_block"),
                        (lambda: M.estimate_batch(m, Y, th[:, None]), "estimate_neural_steps_batch"),
                        (lambda: M.estimate_(m, Y, th[:, None]), "not built"),
                        (lambda: D.run_estimation_(m, Y, 8, th[:, None], ["1"] * len(th), 1, 1e-8),
                         "run_neural_estimation_")):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "neural" in str(e.value) and where in str(e.value), str(e.value)


def test_new_names_refuse_the_other_models_and_what_is_out_of_scope():
    mats = S.maturities_30()
    Y = np.zeros((30, 8))
    sd, _ = M.create_model("SD-NS", mats, 30, 3)
    th = S.theta0_constrained(sd.kind)
    for call in (lambda: M.estimate_neural_steps_batch(sd, Y, th[:, None]),
                 lambda: M.estimate_neural_steps_(sd, Y, th[:, None]),
                 lambda: M.compute_neural_loss_grad_block(sd, Y, th[:, None]),
                 lambda: D.run_neural_estimation_(sd, Y, 8, th[:, None], [], 1, 1e-8)):
        with pytest.raises(NotImplementedError):
            call()
    # Adam groups and an L-BFGS group holding a leading parameter are refused before any launch
    m, _ = M.create_neural_model("NNS", mats, 30, 3)
    tn = S.theta0_constrained(m.kind)
    for groups in (["3"] * 18 + ["2"] * 12, ["2"] * 30):
        with pytest.raises(NotImplementedError):
            M.estimate_neural_steps_batch(m, Y, tn[:, None], param_groups=groups)
    # a process group is refused for the neural kinds as for the λ kinds
    with pytest.raises(NotImplementedError) as e:
        F._estimate_tasks(m, Y, np.array([8], dtype=np.int32), tn, 1, 1e-8, 10, group=object())
    assert "neural" in str(e.value)
