"""GPU tests of the neural models' grouped estimation (yfm_amd.models.estimate_neural_steps_batch: estimate_steps! of
src/optimization.jl:137-312 over the parameter groups, R chains in lockstep) and of the rolling driver on top of it.

Group "2" alone: with the leading parameters fixed, the best loss over (δ, Φ) is a linear least-squares optimum L*
(tests/golden/msedn_grad/make_estimate_groups.py computes it from the restatement's loadings and β).  The chain must
not pass it, must not end below its start, and must come as close as the reference run — the same L-BFGS with the
same options and start on the Float64 restatement's value and gradient, on the CPU — within G = max(1e-6, 10 × that
run's gap): the two may stop an iteration apart under f_abstol.  G is stored with the fixture (0.07–0.28 here: opt2's
f_abstol = 1e-6 stops the reference run 7e-3 to 3e-2 short of L*)."""
from __future__ import annotations

import importlib.util
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from yfm_amd import forecasting as F
from yfm_amd import io as IO
from yfm_amd import models as M
from yfm_amd import params as P

# the λ models' script has the same file name: this one is loaded under a name of its own
_spec = importlib.util.spec_from_file_location("make_neural_estimate_groups",
                                               GOLDEN / "msedn_grad" / "make_estimate_groups.py")
EG = importlib.util.module_from_spec(_spec)
sys.modules["make_neural_estimate_groups"] = EG
_spec.loader.exec_module(EG)

pytestmark = pytest.mark.gpu

CODE = {16: "NNS", 32: "1SD-NNS"}


@pytest.fixture(scope="module")
def ref():
    return EG.load()


@pytest.mark.parametrize("kind", [32, 16])
def test_group_two_alone_reaches_the_least_squares_optimum(engine, ref, kind):
    Y, mats, windows = ref["Y"], ref["maturities"], ref["windows"]
    model, _ = M.create_neural_model(CODE[kind], mats, 4, 3)
    n_lead = P.n_params(kind) - 12
    # the start after the walk: try_initializations keeps a start that is its own best trial
    Theta0 = np.stack([ref[f"k{kind}_w{w}_start_c"] for w in windows], axis=1)
    r = M.estimate_neural_steps_batch(model, Y, Theta0, T_use=windows, param_groups=["-1"] * n_lead + ["2"] * 12)
    assert np.all(r["status"] == 0) and set(r["evals_by_group"]) == {"2"}
    for k, w in enumerate(windows):
        pre = f"k{kind}_w{w}"
        np.testing.assert_allclose(r["init_c"][:, k], ref[f"{pre}_start_c"], rtol=1e-12)
        np.testing.assert_array_equal(r["theta_c"][:n_lead, k], r["init_c"][:n_lead, k])
        # L* from the restatement's trajectory at the leading parameters the chain actually held
        Lstar = EG.optimum(EG.trajectory(kind, Y, r["theta_c"][:, k], int(w)), Y, int(w))
        ll = r["ll"][k]
        ll_start = engine.loglik(kind, r["init_c"][:, k], space=1, T_use=[int(w)])[0]
        G = float(ref[f"{pre}_G"])
        print(f"{pre}: ll_start {ll_start:.9f} ll {ll:.9f} L* {Lstar:.9f} gap {Lstar - ll:.3e} "
              f"reference gap {Lstar - float(ref[pre + '_ll_ref']):.3e} G {G:.3e} "
              f"group iterations {r['group_iters'][k]}")
        assert Lstar == pytest.approx(float(ref[f"{pre}_Lstar"]), rel=1e-9)
        assert ll <= Lstar + 1e-9 * abs(Lstar)
        assert ll >= ll_start
        assert Lstar - ll <= G
        assert ll == -M.compute_loss_batch(model, Y, r["p"][:, k:k + 1], T_use=[int(w)])[0]


@pytest.mark.parametrize("kind", [32, 16])
def test_default_groups(engine, ref, kind):
    """Default groups, two group iterations of at most 40 optimiser iterations: ll is −compute_loss at the returned
    parameters, at least the try_initializations loss, and init_c is the reference's init_p."""
    Y, mats, windows = ref["Y"], ref["maturities"], ref["windows"]
    model, _ = M.create_neural_model(CODE[kind], mats, 4, 3)
    start = ref[f"k{kind}_w40_start0_c"]  # the searched start: the walk's winner leads by more than rounding
    Theta0 = np.repeat(start[:, None], 2, axis=1)
    r = M.estimate_neural_steps_batch(model, Y, Theta0, T_use=windows, max_group_iters=2, iterations=40)
    assert np.all(r["status"] == 0) and set(r["evals_by_group"]) == {"1", "2"}
    assert r["n_evals"] >= sum(r["evals_by_group"].values()) > 0
    for k, w in enumerate(windows):
        w = int(w)
        pre = f"k{kind}_w{w}"
        assert r["ll"][k] == -M.compute_loss_batch(model, Y, r["p"][:, k:k + 1], T_use=[w])[0]
        np.testing.assert_allclose(r["theta_c"][:, k], P.transform_params(kind, r["p"][:, k]), rtol=0, atol=0)
        # init_p: transform(untransform(the restatement's try_initializations winner, stored with the fixture)) —
        # finite, and a finite loss: nothing rescaled.  NNS keeps its start (max_tries = 0)
        win = ref[f"{pre}_start_c"]
        if kind == 16:
            np.testing.assert_array_equal(win, start)
        want_init = P.transform_params(kind, P.untransform_params(kind, win))
        np.testing.assert_array_equal(r["init_c"][:, k], want_init)
        ll_start = float(ref[f"{pre}_ll_start"])
        assert r["ll"][k] >= ll_start - 1e-9 * abs(ll_start)
        print(f"kind {kind} window {w}: start ll {ll_start:.9f} → ll {r['ll'][k]:.9f}, evaluations "
              f"{r['evals_by_group']}, rounds {r['rounds_by_group']}")
    # estimate_neural_steps_ is the one-chain form with the reference's return tuple
    init_p, ll, best_p, ir = M.estimate_neural_steps_(model, Y[:, :24], start[:, None], max_group_iters=2,
                                                      iterations=40)
    assert ir == 0 and ll == r["ll"][1]
    np.testing.assert_array_equal(best_p, r["theta_c"][:, 1])
    np.testing.assert_array_equal(init_p, r["init_c"][:, 1])


def test_rolling_forecasts_write_the_window_csvs(engine, ref, tmp_path):
    """run_rolling_forecasts on three tasks of a 1SD-NNS model from create_neural_model: the estimation goes through
    estimate_neural_steps_batch, and the expanding-window CSVs hold finite forecasts."""
    Y, mats = ref["Y"], ref["maturities"]
    start = ref["k32_w40_start0_c"]
    model, _ = M.create_neural_model("1SD-NNS", mats, 4, 3, results_location=str(tmp_path) + "/")
    out = F.run_rolling_forecasts(model, Y, "t1", in_sample_end=38, in_sample_start=1, forecast_horizon=3,
                                  init_params=start, window_type="expanding", max_group_iters=1, iterations=20)
    res = out["expanding"]
    assert res["tasks"].tolist() == [38, 39, 40] and res["params"].shape == (P.n_params(32), 3)
    assert np.all(res["status"] == 0) and np.all(np.isfinite(res["loss"]))
    assert res["preds"].shape == (4, 3, 3) and np.all(np.isfinite(res["preds"]))
    assert not np.array_equal(res["params"][:, 0], start)  # re-estimated
    for what in ("forecasts", "fitted_params", "fl1", "fl2", "factors", "states"):
        tbl = IO.readdlm(res["files"][what])
        assert tbl.size and np.all(np.isfinite(tbl)), what
    with pytest.raises(NotImplementedError):
        F.run_rolling_forecasts(model, Y, "t1", 38, 1, 3, start, window_type="expanding", group=object())
    # one estimation on the in-sample columns, every origin forecast with it (forecasting.jl:228-283)
    nw = F.run_forecast_no_window(model, Y, "t1", 38, 3, start, max_group_iters=1, iterations=20, write_csv=False)
    assert nw["status"] == 0 and np.isfinite(nw["loss"]) and np.all(np.isfinite(nw["all_results"]))
    np.testing.assert_array_equal(nw["params"], res["params"][:, 0])  # the same chain as the first task's
