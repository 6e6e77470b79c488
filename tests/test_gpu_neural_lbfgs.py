"""GPU test of the batched L-BFGS estimate on the neural models (yfm_amd.lbfgs over yfm_neural_loss_fullgrad_batch;
models.estimate_neural_ mirrors estimate!, optimization.jl:329-410) and of the full-gradient opt-in of the grouped
estimate.

1SD-NNS and NNS on N = 4, T = 40, windows of 40 and 24 columns, from θ₀.  The reference
(tests/golden/msedn_fullgrad/make_estimate_full.py) is the same optimiser on central differences of the Float64
restatement, run at two step sizes: the chain must reach ll ≥ ll_ref − G, G = max(1e-6, 10 × the two runs' difference).
No parity with Optim.jl's iterates is claimed: the driver is judged on the optimum.
"""
from __future__ import annotations

import importlib.util

import numpy as np
import pytest

from conftest import GOLDEN
from yfm_amd import create_neural_model, estimate_neural_, estimate_neural_lbfgs_batch, estimate_neural_steps_batch
from yfm_amd.params import transform_params

# the λ models' generator has the same file name (tests/golden/msed_fullgrad/): this one is loaded under a name of its own
_spec = importlib.util.spec_from_file_location("make_neural_estimate_full",
                                               GOLDEN / "msedn_fullgrad" / "make_estimate_full.py")
ME = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ME)

pytestmark = pytest.mark.gpu

CODE = {32: "1SD-NNS", 16: "NNS"}


@pytest.fixture(scope="module")
def ref():
    return ME.load()


@pytest.fixture(scope="module")
def chains(ref):
    """Per kind: the two windows' chains in one batch."""
    out = {}
    for kind in ME.KINDS:
        model, _ = create_neural_model(CODE[kind], ref["maturities"], 4, 3)
        start = np.repeat(ref[f"k{kind}_start_c"][:, None], 2, axis=1)
        out[kind] = (model, start, estimate_neural_lbfgs_batch(model, ref["Y"], start, space=1, T_use=ref["windows"]))
    return out


@pytest.mark.parametrize("kind", ME.KINDS)
def test_chains_reach_the_reference_optimum(engine, ref, chains, kind):
    model, start, r = chains[kind]
    print(CODE[kind], "ll0", r["ll0"], "ll", r["ll"], "iterations", r["iterations"], "status", r["status"], "evals",
          r["n_evals"], "rounds", r["rounds"])
    assert np.all(np.isfinite(r["ll"])) and np.all(r["ll"] >= r["ll0"])
    for k, w in enumerate(ref["windows"]):
        pre = f"k{kind}_w{w}"
        assert abs(r["ll0"][k] - ref[f"{pre}_ll_start"]) <= 1e-9 * abs(ref[f"{pre}_ll_start"])
        print(pre, "ll", r["ll"][k], "ll_ref", float(ref[f"{pre}_ll_ref"]), "G", float(ref[f"{pre}_G"]))
        assert r["ll"][k] >= ref[f"{pre}_ll_ref"] - ref[f"{pre}_G"], (pre, r["ll"][k])
    # the returned optimum is what the library evaluates there
    engine.set_panel(ref["Y"], ref["maturities"])
    np.testing.assert_array_equal(engine.loglik(kind, r["p"], space=0, T_use=ref["windows"]), r["ll"])
    np.testing.assert_array_equal(r["theta_c"], transform_params(kind, r["p"]))


@pytest.mark.parametrize("kind", ME.KINDS)
def test_two_chains_are_the_chains_run_alone(ref, chains, kind):
    model, start, r = chains[kind]
    for k, w in enumerate(ref["windows"]):
        one = estimate_neural_lbfgs_batch(model, ref["Y"], start[:, k], space=1, T_use=int(w))
        for key in ("p", "theta_c", "init_c"):
            np.testing.assert_array_equal(one[key][:, 0], r[key][:, k], err_msg=key)
        for key in ("ll", "ll0", "status", "iterations"):
            np.testing.assert_array_equal(one[key][0], r[key][k], err_msg=key)


@pytest.mark.parametrize("kind", ME.KINDS)
def test_estimate_returns_the_best_start(ref, kind):
    """estimate_neural_ on the whole panel from two starts (θ₀ and θ₀ with δ halved): the tuple of the start that ends
    best."""
    model, _ = create_neural_model(CODE[kind], ref["maturities"], 4, 3)
    A = np.repeat(ref[f"k{kind}_start_c"][:, None], 2, axis=1)
    A[-12:-9, 1] *= 0.5
    r = estimate_neural_lbfgs_batch(model, ref["Y"], A, space=1)
    init_p, ll, best_p, ir = estimate_neural_(model, ref["Y"], A)
    j = int(np.argmax(r["ll"]))
    assert ll == r["ll"][j] and ir == (0 if r["status"][j] == 0 else 1)
    np.testing.assert_array_equal(init_p, r["init_c"][:, j])
    np.testing.assert_array_equal(best_p, r["theta_c"][:, j])
    assert ll >= ref[f"k{kind}_w40_ll_ref"] - ref[f"k{kind}_w40_G"]
    if kind == 32:  # constrained outputs: A positive, B inside (0, 1)
        assert np.all(best_p[:2] > 0) and np.all((0 < best_p[2:4]) & (best_p[2:4] < 1))
    assert np.all(np.abs(best_p[[-9, -5, -1]]) < 1)  # the diagonal of Φ inside (−1, 1)


@pytest.mark.parametrize("kind", ME.KINDS)
def test_group_two_may_hold_leading_parameters_with_the_full_gradient(ref, kind):
    model, _ = create_neural_model(CODE[kind], ref["maturities"], 4, 3)
    start = np.repeat(ref[f"k{kind}_start_c"][:, None], 2, axis=1)
    groups = ["2"] * start.shape[0]
    with pytest.raises(NotImplementedError, match="leading"):
        estimate_neural_steps_batch(model, ref["Y"], start, T_use=ref["windows"], param_groups=groups)
    r = estimate_neural_steps_batch(model, ref["Y"], start, T_use=ref["windows"], param_groups=groups,
                                    full_gradient=True, max_group_iters=2)
    print(CODE[kind], "ll", r["ll"], "status", r["status"], "evals", r["n_evals"], r["evals_by_group"])
    assert np.all(np.isfinite(r["ll"]))
    for k, w in enumerate(ref["windows"]):
        assert r["ll"][k] >= ref[f"k{kind}_w{w}_ll_start"]
    assert r["evals_by_group"]["2"] > 0
