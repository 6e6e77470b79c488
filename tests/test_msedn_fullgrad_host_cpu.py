"""CPU test of the neural models' full loss gradient (csrc/yfm_msedn_adj.hpp loss_and_fullgrad — the step routines and
the adjoint step the gfx950 kernels run) compiled for the host (tests/msedn_fullgrad_host_check.cpp,
-ffp-contract=off, -fsanitize=address,undefined, a stand-alone program) against tests/golden/msedn_fullgrad/: central
differences of the 40-digit restatement over the leading rows.  Every fixture candidate, in the spaces stored, passes
max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd over the leading rows; the loss and the last 12 rows are loss_and_grad's bit for
bit; a −Inf loss comes with P NaNs, exactly where the fixture has them."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from grad_rule import assert_candidate_rule as check_leading
from gpu_scenarios import same_bits
from host_check_io import build_host_check, run_fullgrad_host as run_host

sys.path.insert(0, str(GOLDEN / "msedn_fullgrad"))
import make_msedn_fullgrad as MF  # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "msedn_fullgrad_host_check", sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return MF.load_cases()


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


@pytest.mark.parametrize("name", MF.case_names())
def test_host_full_gradient_matches_truth(harness, cases, tmp_path, name):
    c = cases
    for space in MF.case_spaces(name):
        Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
        loss, loss12, un, g, g12 = run_host(harness, tmp_path, kind_of(name), c[f"{name}_Y"], c[f"{name}_maturities"],
                                            Th, c[f"{name}_T_use"], space)
        assert same_bits(loss, loss12) and not un.any()
        fin = np.isfinite(loss)
        assert same_bits(g[-12:, fin], g12[:, fin]) and np.isnan(g[:, ~fin]).all()
        want = c[f"{name}_loss_s{space}"]
        assert np.array_equal(np.isneginf(loss), np.isneginf(want))
        assert np.all(np.abs(loss[fin] - want[fin]) <= 1e-9 * np.abs(want[fin]))
        check_leading(g, c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


def test_window_without_a_compared_column(harness, cases, tmp_path):
    """T_use = 1: the loss of loss_and_grad and an exactly zero gradient (no trajectory record is touched)."""
    for kind in MF.kinds():
        name = f"k{kind}_n4t8"
        c = cases
        loss, loss12, un, g, _ = run_host(harness, tmp_path, kind, c[f"{name}_Y"], c[f"{name}_maturities"],
                                          c[f"{name}_theta"], [1, 8], 0)
        assert same_bits(loss, loss12) and not un.any()
        assert np.all(g[:, 0] == 0.0) and np.any(g[:, 1] != 0.0)
