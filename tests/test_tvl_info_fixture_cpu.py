"""CPU test of the TVλ score series' algebra and of the Hessian stencil at the default step: what the gfx950 kernels
tvl_score_kernel and tvl_grad_kernel compute, compiled for the host (tests/tvl_score_host_check.cpp,
-ffp-contract=off) and run one candidate at a time on tests/golden/tvl_info/tvl_info_cases.npz under the GPU tests' rules:

    scores    max |S − s_truth| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]
    sum rule  |Σ_k S[d, k, b] − g[d, b]| ≤ 4·T·2⁻⁵³·Σ_k |S[d, k, b]| against the host gradient
    Hessian   max |H − H_truth| ≤ ref_err[b] + e_fd[b] at h = YFM_TVL_INFO_DEFAULT_STEP

for every stored candidate.  The same program is built once more with -fsanitize=address,undefined (a stand-alone
program: no preloading) and run on the smallest case and on windows that end early.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from host_check_io import build_host_check, run_score_host as run_host
from yfm_amd import _lib

sys.path.insert(0, str(GOLDEN / "tvl_info"))
sys.path.insert(0, str(ROOT / "tools"))
import make_tvl_info as MI  # noqa: E402
import tvl_hessian_step_table as ST  # noqa: E402

REL = 1e-9
U = 2.0 ** -53


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "tvl_score_host_check")


@pytest.fixture(scope="module")
def cases():
    return MI.load_cases()


@pytest.mark.parametrize("name", MI.SCORE_CASES)
def test_host_scores_match_truth_differences_and_sum_to_the_gradient(harness, cases, tmp_path, name):
    c = cases[name]
    B, T = c["Theta"].shape[1], c["Y"].shape[1]
    ll, g, Sc = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], np.full(B, T))
    err = np.abs(Sc - c["s_truth"]).max(axis=(0, 1))
    gn = np.abs(c["g_fd"]).max(axis=0)
    bound = REL * gn + c["e_fd"]
    print("max err / bound:", np.max(err / bound), "max err / |g|:", np.max(err / gn))
    assert np.all(err <= bound), err / bound  # every stored candidate
    assert np.all(Sc[:, 0, :] == 0.0)
    gap = np.abs(Sc.sum(axis=1) - g)
    sb = 4 * T * U * np.abs(Sc).sum(axis=1)
    print("sum rule worst gap / bound:", np.max(gap[sb > 0] / sb[sb > 0]))
    assert np.all(gap <= sb), np.argwhere(gap > sb)
    np.testing.assert_allclose(ll, c["loglik_truth"], rtol=REL)


@pytest.mark.parametrize("name", MI.HESS_CASES)
def test_host_hessian_at_the_default_step_is_as_close_as_the_fp64_reference(harness, cases, tmp_path, name):
    c = cases[name]
    for b in range(c["Theta"].shape[1]):
        H = ST.hessian(harness, tmp_path, c["Y"], c["maturities"], c["Theta"][:, b], _lib.TVL_INFO_DEFAULT_STEP)
        Ht = c["H_truth"][:, :, b]
        err, scale = np.abs(H - Ht).max(), np.abs(Ht).max()
        print(f"case {name} candidate {b}: err/|H|max {err / scale:.3e}, plain FP64 reference's "
              f"{c['ref_err'][b] / scale:.3e}, e_fd/|H|max {c['e_fd'][b] / scale:.3e}")
        assert err <= c["ref_err"][b] + c["e_fd"][b], (b, err / (c["ref_err"][b] + c["e_fd"][b]))


def test_host_scores_under_the_sanitizers(cases, tmp_path):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the stand-alone program: the smallest case on its whole
    window and on windows of 1, 2 and 3 columns (no term, no term, one term)."""
    exe = build_host_check(tmp_path, "tvl_score_host_check", sanitize=True)
    c = cases["S-n4"]
    T = c["Y"].shape[1]
    Th = np.repeat(c["Theta"][:, :1], 4, axis=1)
    tu = np.array([T, 1, 2, 3])
    ll, g, Sc = run_host(exe, tmp_path, c["Y"], c["maturities"], Th, tu)
    assert np.all(Sc[:, :, 1:3] == 0.0) and np.all(ll[1:3] == 0.0)
    assert np.all(Sc[:, 2:, 3] == 0.0) and np.abs(Sc[:, 1, 3]).max() > 0
    np.testing.assert_array_equal(Sc[:, 1, 3], Sc[:, 1, 0])  # a step's term does not depend on the window's end
    err = np.abs(Sc[:, :, 0] - c["s_truth"][:, :, 0]).max()
    assert err <= REL * np.abs(c["g_fd"][:, 0]).max() + c["e_fd"][0]
