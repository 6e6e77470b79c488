"""CPU test of the TVλ gradient's tangent algebra (csrc/yfm_tvl_grad.hpp): the functions the gfx950 kernel runs,
compiled for the host (tests/tvl_grad_host_check.cpp, -ffp-contract=off) and run one candidate at a time on every
case of the fixture (tests/golden/tvl_grad), held to the GPU test's rule:

    max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]   for every compared candidate, at least 75% compared.

The estimation-length cases of tvl_grad_long_cases.npz (T = 200 and 600, make_tvl_grad_long.py) run through the same
program.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from grad_rule import REL, assert_gradient_rule, chain_factor
from host_check_io import build_host_check, run_grad_host as run_host

sys.path.insert(0, str(GOLDEN / "tvl_grad"))
import make_tvl_grad as MG  # noqa: E402
import make_tvl_grad_long as ML  # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "tvl_grad_host_check")


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


def check_case(name, c, ll, g):
    """The recursion's own FP64 value is not what the library returns (that is the loglik launch's): its distance from
    the truth is printed only."""
    assert_gradient_rule(g, c, label=f"case {name}", short_windows_zero=True, primal=ll, primal_mask=c["compared"],
                         primal_asserted=False)


@pytest.mark.parametrize("name", MG.CASE_NAMES)
def test_host_gradient_matches_truth_differences(harness, cases, tmp_path, name):
    c = cases[name]
    ll, g = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], c["T_use"])
    check_case(name, c, ll, g)


@pytest.mark.parametrize("name", ML.CASE_NAMES)
def test_host_gradient_matches_truth_differences_at_estimation_length(harness, tmp_path, name):
    """The same rule on tvl_grad_long_cases.npz (make_tvl_grad_long.py): T = 200 and 600, windows over a NaN column
    late in the panel."""
    c = ML.load_cases()[name]
    ll, g = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], c["T_use"])
    check_case(name, c, ll, g)


def test_host_chain_rule(harness, cases, tmp_path):
    """grad(space 0, θ) = grad(space 1, θ_c) · dθ_c/dθ: θ_c for the exp entries, (1 − θ_c²)/2 for the Φ diagonal."""
    from yfm_amd import KIND_TVL
    from yfm_amd.params import transform_params
    c = cases["C"]
    Th = c["Theta"]
    Tc = np.stack([transform_params(KIND_TVL, Th[:, b]) for b in range(Th.shape[1])], axis=1)
    _, g0 = run_host(harness, tmp_path, c["Y"], c["maturities"], Th, c["T_use"], 0)
    _, g1 = run_host(harness, tmp_path, c["Y"], c["maturities"], Tc, c["T_use"], 1)
    f = chain_factor(KIND_TVL, Tc)
    assert np.all(np.abs(g0 - g1 * f).max(axis=0) <= REL * np.abs(g0).max(axis=0))
