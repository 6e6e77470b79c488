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

import subprocess

import numpy as np
import pytest

import smooth_fixture as SF
from conftest import ROOT
from host_check_io import run_program

SRC = ROOT / "tests" / "smooth_host_check.cpp"
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]


def run_host(exe, tmp_path, M, Y, m, Th, tu, space=0):
    """(beta_s[M, T, B], V_s[M, M, T, B], C_s[M, M, T − 1, B]) of smooth_host_check: T lines per candidate."""
    T, B = Y.shape[1], Th.shape[1]
    rows = np.array(run_program(exe, tmp_path, Y, m, Th, tu, space)).reshape(B, T, M + 2 * M * M)
    bs = rows[:, :, :M].transpose(2, 1, 0)
    V = rows[:, :, M:M + M * M].reshape(B, T, M, M).transpose(3, 2, 1, 0)  # column-major M × M per line
    C = rows[:, :, M + M * M:].reshape(B, T, M, M).transpose(3, 2, 1, 0)[:, :, :T - 1]
    return bs, V, C


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("smooth")
    exes = {}
    for M in (3, 5):
        exes[M] = d / f"smooth_host_check_{M}"
        subprocess.run(["g++", "-O2", *FLAGS, f"-DYFM_SMOOTH_M={M}", str(SRC), "-o", str(exes[M])], check=True)
    return exes


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
    exe = tmp_path / "smooth_host_check_san"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS,
                    "-DYFM_SMOOTH_M=3", str(SRC), "-o", str(exe)], check=True)
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
