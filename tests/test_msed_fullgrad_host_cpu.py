"""CPU test of the λ models' full loss gradient (csrc/yfm_msed.hpp: the tangent functions the gfx950 full-gradient
kernel runs, driven by get_loss_fullgrad) compiled for the host (tests/msed_fullgrad_host_check.cpp,
-ffp-contract=off, -fsanitize=address,undefined, a stand-alone program) against tests/golden/msed_fullgrad/: central
differences of the 40-digit restatement over all P rows.  Every fixture candidate, in both parameter spaces, passes
max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd; the loss is get_loss's and the last 12 rows are get_loss_grad's, bit for bit;
a −Inf loss comes with P NaNs, exactly where the fixture has them.  The N = 30, T = 600 cases of msed_fullgrad_long.npz
(make_msed_fullgrad_long.py) run through the same program."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from grad_rule import assert_candidate_rule as check_gradient
from gpu_scenarios import same_bits
from host_check_io import build_host_check, run_fullgrad_host as run_host

sys.path.insert(0, str(GOLDEN / "msed_fullgrad"))
import make_msed_fullgrad as MF  # noqa: E402
import make_msed_fullgrad_long as MFL  # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "msed_fullgrad_host_check", sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return MF.load_cases()


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MF.case_names())
def test_host_full_gradient_matches_truth(harness, cases, tmp_path, name, space):
    c = cases
    kind = int(name[1])
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    loss, loss_plain, un, g, g12 = run_host(harness, tmp_path, kind, c[f"{name}_Y"], c[f"{name}_maturities"], Th,
                                            c[f"{name}_T_use"], space)
    assert same_bits(loss, loss_plain), (loss, loss_plain)  # the loss beside the gradient is get_loss's, sum for sum
    assert not un.any()
    fin = np.isfinite(loss)
    assert same_bits(g[-12:, fin], g12[:, fin])  # … and the last 12 rows are get_loss_grad's
    want = c[f"{name}_loss_s{space}"]
    assert np.array_equal(np.isneginf(loss), np.isneginf(want))
    f = np.isfinite(want)
    assert np.all(np.abs(loss[f] - want[f]) <= 1e-9 * np.abs(want[f]))  # the project's parity bar
    check_gradient(g, c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MFL.case_names())
def test_host_full_gradient_matches_truth_at_estimation_length(harness, tmp_path, name, space):
    """The same assertions on msed_fullgrad_long.npz (make_msed_fullgrad_long.py): N = 30, T = 600, and for two kinds
    the windows 300 and 600 over a missing column 450 (the long one is −Inf with no gradient)."""
    c = MFL.load_cases()
    kind = int(name[1])
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    loss, loss_plain, un, g, g12 = run_host(harness, tmp_path, kind, c[f"{name}_Y"], c[f"{name}_maturities"], Th,
                                            c[f"{name}_T_use"], space)
    assert same_bits(loss, loss_plain), (loss, loss_plain)
    assert not un.any()
    fin = np.isfinite(loss)
    assert same_bits(g[-12:, fin], g12[:, fin])
    want = c[f"{name}_loss_s{space}"]
    assert np.array_equal(np.isneginf(loss), np.isneginf(want))
    f = np.isfinite(want)
    assert np.all(np.abs(loss[f] - want[f]) <= 1e-9 * np.abs(want[f]))
    check_gradient(g, c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


def test_fixture_covers_the_special_cases(cases):
    """The window over the missing column is −Inf with no gradient, the leading NaN leaves every gradient finite, and
    every stored leading row is at least 1e-6 of its gradient's largest entry (the generator's screen)."""
    for kind in MF.KINDS:
        assert np.isnan(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 1:]).all()
        assert np.isfinite(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 0]).all()
        for tag in ("n4t8nan0", "n30t8nan0"):
            assert np.isnan(cases[f"k{kind}_{tag}_Y"][0, 0])
            assert np.isfinite(cases[f"k{kind}_{tag}_g_fd_s1"]).all()
    for name in MF.case_names():
        K = MF.n_lead(int(name[1]))
        for space in (0, 1):
            g = cases[f"{name}_g_fd_s{space}"]
            assert g.shape[0] == K + 12
            for b in range(3):
                if np.isfinite(g[:, b]).all():
                    assert np.all(np.abs(g[:K, b]) >= MF.SCREEN * np.max(np.abs(g[:, b]))), (name, space, b)


def test_lambda_overflow_makes_the_gradient_unavailable(harness, cases, tmp_path):
    """NS with γ = 800: λ = Inf, Z = [1 0 0], the ridged OLS gives a finite loss and get_loss_grad 12 finite rows, but
    ∂Z/∂γ is NaN — all P rows NaN and the candidate reported as unavailable; its neighbours are untouched."""
    c = cases
    Th = c["k3_n4t8_theta"].copy()
    Th[0, 1] = 800.0
    loss, loss_plain, un, g, g12 = run_host(harness, tmp_path, 3, c["k3_n4t8_Y"], c["k3_n4t8_maturities"], Th,
                                            c["k3_n4t8_T_use"], 0)
    assert same_bits(loss, loss_plain) and np.isfinite(loss).all()
    assert un.tolist() == [0.0, 1.0, 0.0]
    assert np.isnan(g[:, 1]).all() and np.isfinite(g12[:, 1]).all()
    assert np.isfinite(g[:, [0, 2]]).all() and same_bits(g[-12:, [0, 2]], g12[:, [0, 2]])
