"""GPU test of the λ models' full loss gradient (csrc/yfm_msed.hip lambda_fullgrad_kernel) at estimation length:
N = 30, T = 600, every kind, both parameter spaces and both lane counts, against central differences of the 40-digit
restatement (tests/golden/msed_fullgrad/msed_fullgrad_long.npz, make_msed_fullgrad_long.py).

tests/test_gpu_msed_fullgrad.py's rule and body: per candidate max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd over all P rows;
a −Inf loss (the window over the missing column 450) comes with P NaNs exactly where the fixture has them; the loss
is engine.loglik's and rows P−12 … P−1 are engine.lambda_loss_grad's, bit for bit — which holds the δ/Φ kernel to the
same truth at T = 600.  Observed on MI355X: DESIGN.md §3.9.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import same_bits
from grad_rule import assert_candidate_rule as check_gradient
from test_gpu_msed_fullgrad import lanes_env  # noqa: F401  (lanes_env is a fixture)

sys.path.insert(0, str(GOLDEN / "msed_fullgrad"))
import make_msed_fullgrad_long as ML  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return ML.load_cases()


@pytest.mark.parametrize("lanes", ["4", "16"])
@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", ML.case_names())
def test_full_gradient_matches_truth(engine, cases, lanes_env, name, space, lanes):
    c = cases
    kind = int(name[1])
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    tu = c[f"{name}_T_use"]
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    os.environ["YFM_MSED_LANES"] = lanes
    loss, g = engine.lambda_loss_full_grad(kind, Th, space=space, T_use=tu)
    thrown, neg_inf = engine.last_flags()
    unavailable = engine.last_grad_unavailable()
    g_fd, e_fd = c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"]
    assert thrown == 0 and neg_inf == int(np.isnan(g_fd).any(axis=0).sum()) and unavailable == 0
    assert g.shape == Th.shape
    assert same_bits(loss, engine.loglik(kind, Th, space=space, T_use=tu))
    _, g12 = engine.lambda_loss_grad(kind, Th, space=space, T_use=tu)
    fin = np.isfinite(loss)
    assert same_bits(g[-12:, fin], g12[:, fin])
    assert np.isnan(g[:, ~fin]).all()
    for b in np.flatnonzero(np.isfinite(g_fd).all(axis=0) & np.isfinite(g).all(axis=0)):
        top = np.max(np.abs(g_fd[:, b]))
        err = np.max(np.abs(g[:, b] - g_fd[:, b]))
        print(f"{name} space {space} L={lanes} b={b}: err/bound {err / (1e-9 * top + e_fd[b]):.3e}, "
              f"err/|g| {err / top:.3e}")
    check_gradient(g, g_fd, e_fd, loss, f"{name} space {space} L={lanes}")
