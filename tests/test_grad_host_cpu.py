"""CPU test of the DNS gradient's tangent algebra (csrc/yfm_grad.hpp): the functions the gfx950 kernel runs,
compiled for the host (tests/grad_host_check.cpp, -ffp-contract=off) and run one candidate at a time on the
fixture cases B (N = 10, one NaN entry) and E (N = 4), held to the GPU test's rule:

    max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]   for every compared candidate, at least 75% compared.

The estimation-length cases of grad_long_cases.npz (T up to 600, make_grad_long.py) run through the same program.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from grad_rule import REL, assert_gradient_rule, chain_factor
from host_check_io import build_host_check, run_grad_host as run_host

sys.path.insert(0, str(GOLDEN / "grad"))
import make_grad as MG  # noqa: E402
import make_grad_long as ML  # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "grad_host_check")


@pytest.mark.parametrize("name", ["B", "E"])
def test_host_gradient_matches_truth_differences(harness, tmp_path, name):
    c = MG.load_cases()[name]
    ll, g = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], c["T_use"])
    assert_gradient_rule(g, c, label=f"case {name}", primal=ll)


def check_long_case(name, c, ll, g):
    """The same rule on a case of grad_long_cases.npz (make_grad_long.py).  Read from the fixture alone: a `hard`
    candidate of L-hard (the dense FP64 oracle's own loglik is more than 1e-9 from the truth) may instead be as close
    to the truth as the plain FP64 reference gradient, err ≤ ref_err; the host build has no deferral, so the L-band
    candidates with a stored κ₁(Z'Z) ≥ 5e5 are left to the GPU test."""
    sel = c["compared"] & (c["kappa1"] < 5e5) if name == "L-band" else c["compared"]
    hard = None
    if name == "L-hard":
        assert c["hard"].tolist() == [True, True, True, True, False, False]
        hard = c["hard"]
    # the recursion's own FP64 value: held to the bar where the dense FP64 oracle is inside it too
    assert_gradient_rule(g, c, label=f"case {name}", sel=sel, second_clause=hard, primal=ll,
                         primal_mask=sel & ~c["hard"])


@pytest.mark.parametrize("name", ML.CASE_NAMES)
def test_host_gradient_matches_truth_differences_at_estimation_length(harness, tmp_path, name):
    c = ML.load_cases()[name]
    ll, g = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], c["T_use"])
    check_long_case(name, c, ll, g)


def test_host_chain_rule(harness, tmp_path):
    """grad(space 0, θ) = grad(space 1, θ_c) · dθ_c/dθ: θ_c for the exp entries, (1 − θ_c²)/2 for the Φ diagonal."""
    from yfm_amd import KIND_DNS
    from yfm_amd.params import transform_params
    c = MG.load_cases()["E"]
    Th = c["Theta"]
    Tc = np.stack([transform_params(KIND_DNS, Th[:, b]) for b in range(Th.shape[1])], axis=1)
    _, g0 = run_host(harness, tmp_path, c["Y"], c["maturities"], Th, c["T_use"], 0)
    _, g1 = run_host(harness, tmp_path, c["Y"], c["maturities"], Tc, c["T_use"], 1)
    f = chain_factor(KIND_DNS, Tc)
    assert np.all(np.abs(g0 - g1 * f).max(axis=0) <= REL * np.abs(g0).max(axis=0))
