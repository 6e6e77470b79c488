"""GPU test of the TVλ log-likelihood gradient (csrc/yfm_tvl_grad.hip) at estimation length: T = 200 and T = 600 at
N = 30, and windows over a NaN column late in the panel (tests/golden/tvl_grad/tvl_grad_long_cases.npz,
make_tvl_grad_long.py: make_tvl_grad.py's recipe over a longer ladder of steps).

The rule is tests/test_gpu_tvl_grad.py's: per case and compared candidate (at least 75% of a case)

    max_i |g_gpu − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]

under both precisions of the context; the value follows the precision, the gradient is the same bits under both.
Observed on MI355X: DESIGN.md §3.8.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_batch_independent
from grad_rule import assert_gradient_rule
from test_gpu_parity import assert_parity
from yfm_amd import KIND_TVL, _lib

sys.path.insert(0, str(GOLDEN / "tvl_grad"))
import make_tvl_grad_long as ML  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return ML.load_cases()


@pytest.mark.parametrize("name", ML.CASE_NAMES)
def test_gradient_matches_truth_differences(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    old = engine.precision
    out = {}
    try:
        for mode in (_lib.PREC_CERTIFIED, _lib.PREC_FP64):
            engine.precision = mode
            ll, g = engine.tvl_loglik_grad(KIND_TVL, c["Theta"], space=0, T_use=c["T_use"])
            unavailable = engine.last_grad_unavailable()
            assert_gradient_rule(g, c, label=f"case {name}, precision {mode}")
            np.testing.assert_array_equal(ll, engine.loglik(KIND_TVL, c["Theta"], space=0, T_use=c["T_use"]))
            if mode == _lib.PREC_CERTIFIED:
                assert_parity(ll, c["loglik_oracle"], c["loglik_truth"])
            assert unavailable == 0
            out[mode] = g
    finally:
        engine.precision = old
    np.testing.assert_array_equal(out[_lib.PREC_CERTIFIED], out[_lib.PREC_FP64])


def test_outputs_do_not_depend_on_the_batch(engine, cases):
    """The last candidate of L600 alone, inside the batch of 16 and with the batch reversed: the same bits."""
    c = cases["L600"]
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"]
    last = Th.shape[1] - 1
    ll, g = assert_batch_independent(lambda X: engine.tvl_loglik_grad(KIND_TVL, X), Th, [last])
    assert np.isfinite(g[:, last]).all()
