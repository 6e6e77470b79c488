"""CPU test of the neural models' δ/Φ loss gradient (csrc/yfm_msedn.hpp loss_and_grad with csrc/yfm_msed.hpp's accum_zv,
grad_accum, grad_finish — the functions the gfx950 gradient kernel runs) compiled for the host
(tests/msedn_grad_host_check.cpp, -ffp-contract=off, -fsanitize=address,undefined, a stand-alone program) against
tests/golden/msedn_grad/: central differences of the 40-digit restatement.  Every fixture candidate, in both parameter
spaces, passes the rule of tests/test_gpu_grad.py, max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd; a −Inf loss comes with 12
NaNs, exactly where the fixture has them."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from grad_rule import assert_candidate_rule as check_gradient
from host_check_io import build_host_check, run_kind_grad_host as run_host

sys.path.insert(0, str(GOLDEN / "msedn_grad"))
import make_msedn_grad as MG  # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "msedn_grad_host_check", sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MG.case_names())
def test_host_gradient_matches_truth(harness, cases, tmp_path, name, space):
    c = cases
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    loss, loss_plain, g = run_host(harness, tmp_path, kind_of(name), c[f"{name}_Y"], c[f"{name}_maturities"], Th,
                                   c[f"{name}_T_use"], space)
    # the loss beside the gradient is get_loss's, sum for sum
    assert np.array_equal(loss, loss_plain), (loss, loss_plain)
    want = c[f"{name}_loss_s{space}"]
    assert np.array_equal(np.isneginf(loss), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(loss[fin] - want[fin]) <= 1e-9 * np.abs(want[fin]))  # the project's parity bar
    check_gradient(g, c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


def test_fixture_covers_the_special_cases(cases):
    """The window over the missing column is −Inf with no gradient; the leading NaN column leaves every gradient
    finite; the restatement's own analytic gradient is ten times inside the bar for every stored candidate."""
    for kind in MG.kinds():
        assert np.isnan(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 1:]).all()
        assert np.isfinite(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 0]).all()
        assert np.isnan(cases[f"k{kind}_n4t8nan6_Y"][:, 5]).all()
        for tag in ("n4t8nan0", "n30t8nan0"):
            assert np.isnan(cases[f"k{kind}_{tag}_Y"][:, 0]).all()
            assert np.isfinite(cases[f"k{kind}_{tag}_g_fd_s1"]).all()
    for name in MG.case_names():
        for space in (0, 1):
            g_fd, e_fd, rerr = (cases[f"{name}_{k}_s{space}"] for k in ("g_fd", "e_fd", "rerr"))
            fin = np.isfinite(e_fd)
            assert np.all(rerr[fin] <= MG.SELF_REL * np.max(np.abs(g_fd[:, fin]), axis=0) + e_fd[fin]), (name, space)
    print("worst restatement error relative to |g_fd|inf:", float(cases["worst_restatement_rel"]))
