"""CPU test of the smoother's algebra (csrc/yfm_smooth.hpp): what the gfx950 kernel smooth_kernel computes, compiled for
the host (tests/smooth_host_check.cpp, -ffp-contract=off; the predicted moments the device reads from the forward
launch's record come from the header's own predict) and run on every case and window of
tests/golden/smooth/smooth_cases.npz, in both parameter spaces, under the rule of tests/test_gpu_states.py (factor 1):
per array, with a step's error measured normwise against the truth's magnitude at that step, the result is within 1e-9
of the dense FP64 checker, or at least as close to the 40-digit truth as the checker is.

The same program is built once more with -fsanitize=address,undefined (a stand-alone program: no preloading) and run on
the smallest case and on windows of 1, 2 and 3 columns.
"""
from __future__ import annotations

import numpy as np
import pytest

import smooth_fixture as SF
from host_check_io import build_host_check, run_smooth_host as run_host


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("smooth")
    return {M: build_host_check(d, "smooth_host_check", M=M) for M in (3, 5)}


@pytest.mark.parametrize("space", (0, 1))
@pytest.mark.parametrize("name,n", SF.CASE_WINDOWS)
def test_host_smoother_meets_the_rule(harness, tmp_path, name, n, space):
    c = SF.cases()[name]
    n = SF.window_of(c, n)
    M = SF.SR.STATE_DIM[c["kind"]]
    Th = c["Theta"] if space == 0 else c["Theta_c"]
    B = Th.shape[1]
    bs, V, C = run_host(harness[M], tmp_path, M, c["Y"], c["maturities"], Th, np.full(B, n), space)
    for b in range(B):
        SF.assert_candidate(name, n, b, space, bs[..., b], V[..., b], C[..., b])


def test_host_smoother_under_the_sanitizers(tmp_path):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the stand-alone program: the smallest case on its whole window
    and on windows of 1, 2 and 3 columns (one update and no C; one C; two), each against the dense checker on the
    same window."""
    exe = build_host_check(tmp_path, "smooth_host_check", sanitize=True, M=3)
    c = SF.cases()["S-E"]
    T = c["Y"].shape[1]
    Th = np.repeat(c["Theta"][:, :1], 4, axis=1)
    tu = np.array([T, 1, 2, 3])
    bs, V, C = run_host(exe, tmp_path, 3, c["Y"], c["maturities"], Th, tu)
    SF.assert_candidate("S-E", T, 0, 0, bs[..., 0], V[..., 0], C[..., 0])
    for k, n in enumerate(tu[1:], start=1):
        assert np.isfinite(bs[:, :n, k]).all() and np.isnan(bs[:, n:, k]).all()
        assert np.isfinite(C[:, :, :n - 1, k]).all() and np.isnan(C[:, :, n - 1:, k]).all()
        ref = SF.SR.smooth_dense(c["kind"], c["maturities"], c["Y"], Th[:, 0], 0, int(n))
        for g, r in zip((bs[:, :n, k], V[:, :, :n, k], C[:, :, :n - 1, k]), ref):
            assert SF.SR.traj_err(g, r, r) <= 1e-9
