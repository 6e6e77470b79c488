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
from test_gpu_parity import assert_parity
from yfm_amd import KIND_TVL, _lib

sys.path.insert(0, str(GOLDEN / "tvl_grad"))
import make_tvl_grad_long as ML  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-9


@pytest.fixture(scope="module")
def cases():
    return ML.load_cases()


@pytest.mark.parametrize("name", ML.CASE_NAMES)
def test_gradient_matches_truth_differences(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    cmp_ = c["compared"]
    assert cmp_.mean() >= 0.75
    gn = np.abs(c["g_fd"]).max(axis=0)
    bound = REL * gn + c["e_fd"]
    nz = cmp_ & (gn > 0)
    old = engine.precision
    out = {}
    try:
        for mode in (_lib.PREC_CERTIFIED, _lib.PREC_FP64):
            engine.precision = mode
            ll, g = engine.tvl_loglik_grad(KIND_TVL, c["Theta"], space=0, T_use=c["T_use"])
            unavailable = engine.last_grad_unavailable()
            err = np.abs(g - c["g_fd"]).max(axis=0)
            print(f"case {name}, precision {mode}: compared {int(cmp_.sum())}/{cmp_.size}, max err/bound "
                  f"{np.max(err[nz] / bound[nz]):.3e}, max err/|g| {np.max(err[nz] / gn[nz]):.3e}")
            assert np.all(err[cmp_] <= bound[cmp_]), (np.flatnonzero(cmp_ & ~(err <= bound)), np.max(err[nz] / gn[nz]))
            assert np.all(g[(c["g_fd"] == 0.0) & cmp_[None, :]] == 0.0)
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
    ll, g = engine.tvl_loglik_grad(KIND_TVL, Th)
    l1, g1 = engine.tvl_loglik_grad(KIND_TVL, Th[:, last])
    llr, gr = engine.tvl_loglik_grad(KIND_TVL, np.asfortranarray(Th[:, ::-1]))
    assert np.isfinite(g[:, last]).all()
    np.testing.assert_array_equal(l1[0], ll[last])
    np.testing.assert_array_equal(g1[:, 0], g[:, last])
    np.testing.assert_array_equal(llr[::-1], ll)
    np.testing.assert_array_equal(gr[:, ::-1], g)
