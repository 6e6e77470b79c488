"""CPU test of the TVλ smoother's algebra (csrc/yfm_tvl_smooth.hpp with csrc/yfm_smooth.hpp and csrc/yfm_tvl_grad.hpp):
what the gfx950 kernel tvl_smooth_kernel computes, compiled for the host (tests/tvl_smooth_host_check.cpp,
-ffp-contract=off; the predicted moments the device reads from the forward launch's record come from
yfm_smooth.hpp's predict) and run on every case and window of tests/golden/tvl_smooth/tvl_smooth_cases.npz, in both
parameter spaces, under the rule of tests/test_gpu_states.py (factor 1): per array, with a step's error measured
normwise against the truth's magnitude at that step, the result is within 1e-9 of the dense FP64 checker, or at least
as close to the 40-digit truth as the checker is.

The same program is built once more with -fsanitize=address,undefined (a stand-alone program: no preloading) and run on
the smallest case and on windows of 1, 2 and 3 columns.
"""
from __future__ import annotations

import numpy as np
import pytest

import tvl_smooth_fixture as TF
from host_check_io import build_host_check, run_smooth_host as run_host


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_check(tmp_path_factory, "tvl_smooth_host_check")


@pytest.mark.parametrize("space", (0, 1))
@pytest.mark.parametrize("name,n", TF.CASE_WINDOWS)
def test_host_smoother_meets_the_rule(exe, tmp_path, name, n, space):
    c = TF.cases()[name]
    n = TF.window_of(c, n)
    Th = c["Theta"] if space == 0 else c["Theta_c"]
    B = Th.shape[1]
    bs, V, C = run_host(exe, tmp_path, 4, c["Y"], c["maturities"], Th, np.full(B, n), space)
    for b in range(B):
        TF.assert_candidate(name, n, b, space, bs[..., b], V[..., b], C[..., b])


def test_host_smoother_under_the_sanitizers(tmp_path):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the stand-alone program: the smallest case on its whole window
    and on windows of 1, 2 and 3 columns (one update and no C; one C; two), each against the dense checker on the
    same window."""
    san = build_host_check(tmp_path, "tvl_smooth_host_check", sanitize=True)
    c = TF.cases()["T-E"]
    T = c["Y"].shape[1]
    Th = np.repeat(c["Theta"][:, :1], 4, axis=1)
    tu = np.array([T, 1, 2, 3])
    bs, V, C = run_host(san, tmp_path, 4, c["Y"], c["maturities"], Th, tu)
    TF.assert_candidate("T-E", T, 0, 0, bs[..., 0], V[..., 0], C[..., 0])
    for k, n in enumerate(tu[1:], start=1):
        assert np.isfinite(bs[:, :n, k]).all() and np.isnan(bs[:, n:, k]).all()
        assert np.isfinite(C[:, :, :n - 1, k]).all() and np.isnan(C[:, :, n - 1:, k]).all()
        ref = TF.TR.smooth_dense(c["maturities"], c["Y"], Th[:, 0], 0, int(n))
        for g, r in zip((bs[:, :n, k], V[:, :, :n, k], C[:, :, :n - 1, k]), ref):
            assert TF.TR.traj_err(g, r, r) <= 1e-9
