"""CPU test of the DNS score series' algebra (csrc/yfm_grad.hpp score_value over the step functions): what the
gfx950 kernel dns_score_kernel stores, compiled for the host (tests/score_host_check.cpp, -ffp-contract=off) and run
one candidate at a time on the score cases of tests/golden/info/info_cases.npz under the GPU test's rule:

    max |S − s_truth| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]   for every stored candidate.

The same program is built once more with -fsanitize=address,undefined (a stand-alone program: no preloading) and run on
the smallest case and on windows that end early.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from host_check_io import build_host_check, run_score_host as run_host

sys.path.insert(0, str(GOLDEN / "info"))
import make_info as MI  # noqa: E402

REL = 1e-9


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "score_host_check")


def check_case(c, ll, g, Sc):
    T = c["Y"].shape[1]
    err = np.abs(Sc - c["s_truth"]).max(axis=(0, 1))
    gn = np.abs(c["g_fd"]).max(axis=0)
    bound = REL * gn + c["e_fd"]
    print("max err / bound:", np.max(err / bound), "max err / |g|:", np.max(err / gn))
    assert np.all(err <= bound), err / bound
    assert np.all(Sc[:, 0, :] == 0.0)
    # the terms sum to the gradient the same recursion accumulates, up to the order of the sum
    gap = np.abs(Sc.sum(axis=1) - g)
    assert np.all(gap <= REL * gn), (gap / gn).max()
    np.testing.assert_allclose(ll, c["loglik_truth"], rtol=REL)


@pytest.mark.parametrize("name", MI.SCORE_CASES)
def test_host_scores_match_truth_differences(harness, tmp_path, name):
    c = MI.load_cases()[name]
    B = c["Theta"].shape[1]
    ll, g, Sc = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], np.full(B, c["Y"].shape[1]))
    check_case(c, ll, g, Sc)


def test_host_scores_under_the_sanitizers(tmp_path):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the stand-alone program: the smallest case on its whole
    window and on windows of 1, 2 and 3 columns (no term, no term, one term)."""
    exe = build_host_check(tmp_path, "score_host_check", sanitize=True)
    c = MI.load_cases()["S-E"]
    T = c["Y"].shape[1]
    Th = np.repeat(c["Theta"][:, :1], 4, axis=1)
    tu = np.array([T, 1, 2, 3])
    ll, g, Sc = run_host(exe, tmp_path, c["Y"], c["maturities"], Th, tu)
    assert np.all(Sc[:, :, 1:3] == 0.0) and np.all(ll[1:3] == 0.0)
    assert np.all(Sc[:, 2:, 3] == 0.0) and np.abs(Sc[:, 1, 3]).max() > 0
    np.testing.assert_array_equal(Sc[:, 1, 3], Sc[:, 1, 0])  # a step's term does not depend on the window's end
    err = np.abs(Sc[:, :, 0] - c["s_truth"][:, :, 0]).max()
    assert err <= REL * np.abs(c["g_fd"][:, 0]).max() + c["e_fd"][0]
