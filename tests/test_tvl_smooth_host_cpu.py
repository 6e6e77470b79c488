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

import subprocess

import numpy as np
import pytest

import tvl_smooth_fixture as TF
from conftest import ROOT
from host_check_io import run_program

SRC = ROOT / "tests" / "tvl_smooth_host_check.cpp"
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
M = 4


def run_host(exe, tmp_path, Y, m, Th, tu, space=0):
    """(beta_s[4, T, B], V_s[4, 4, T, B], C_s[4, 4, T − 1, B]) of tvl_smooth_host_check: T lines per candidate."""
    T, B = Y.shape[1], Th.shape[1]
    rows = np.array(run_program(exe, tmp_path, Y, m, Th, tu, space)).reshape(B, T, M + 2 * M * M)
    bs = rows[:, :, :M].transpose(2, 1, 0)
    V = rows[:, :, M:M + M * M].reshape(B, T, M, M).transpose(3, 2, 1, 0)  # column-major 4 × 4 per line
    C = rows[:, :, M + M * M:].reshape(B, T, M, M).transpose(3, 2, 1, 0)[:, :, :T - 1]
    return bs, V, C


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("tvl_smooth") / "tvl_smooth_host_check"
    subprocess.run(["g++", "-O2", *FLAGS, str(SRC), "-o", str(out)], check=True)
    return out


@pytest.mark.parametrize("space", (0, 1))
@pytest.mark.parametrize("name,n", TF.CASE_WINDOWS)
def test_host_smoother_meets_the_rule(exe, tmp_path, name, n, space):
    c = TF.cases()[name]
    n = TF.window_of(c, n)
    Th = c["Theta"] if space == 0 else c["Theta_c"]
    B = Th.shape[1]
    bs, V, C = run_host(exe, tmp_path, c["Y"], c["maturities"], Th, np.full(B, n), space)
    for b in range(B):
        TF.assert_candidate(name, n, b, space, bs[..., b], V[..., b], C[..., b])


def test_host_smoother_under_the_sanitizers(tmp_path):
    """AddressSanitizer and UndefinedBehaviorSanitizer on the stand-alone program: the smallest case on its whole window
    and on windows of 1, 2 and 3 columns (one update and no C; one C; two), each against the dense checker on the
    same window."""
    san = tmp_path / "tvl_smooth_host_check_san"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, str(SRC),
                    "-o", str(san)], check=True)
    c = TF.cases()["T-E"]
    T = c["Y"].shape[1]
    Th = np.repeat(c["Theta"][:, :1], 4, axis=1)
    tu = np.array([T, 1, 2, 3])
    bs, V, C = run_host(san, tmp_path, c["Y"], c["maturities"], Th, tu)
    TF.assert_candidate("T-E", T, 0, 0, bs[..., 0], V[..., 0], C[..., 0])
    for k, n in enumerate(tu[1:], start=1):
        assert np.isfinite(bs[:, :n, k]).all() and np.isnan(bs[:, n:, k]).all()
        assert np.isfinite(C[:, :, :n - 1, k]).all() and np.isnan(C[:, :, n - 1:, k]).all()
        ref = TF.TR.smooth_dense(c["maturities"], c["Y"], Th[:, 0], 0, int(n))
        for g, r in zip((bs[:, :n, k], V[:, :, :n, k], C[:, :, :n - 1, k]), ref):
            assert TF.TR.traj_err(g, r, r) <= 1e-9
