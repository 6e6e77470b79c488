"""CPU test of the TVλ smoother's algebra (csrc/yfm_tvl_smooth.hpp) at estimation length:
tests/tvl_smooth_host_check.cpp, unchanged (host build, -ffp-contract=off; the forward moments come from
yfm_smooth.hpp's predict), on every case and window of tests/golden/tvl_smooth_long/tvl_smooth_long_cases.npz under the
rule of tests/smooth_long_fixture.py — an ordinary candidate within 1e-9 of the dense FP64 checker, a hard one within 1e-9
of it or at least as close to the stored 40-digit truth as the checker is.

Observed, worst array, window and ordinary candidate, result − checker as a fraction of the 1e-9 bar: TL-chunk 4.1e-4,
TL-n90 3.0e-3, TL-600 9.6e-4.  TL-n90's candidate 1 is hard by a hair (checker − truth 1.03e-10 in C):
(result − checker, result − truth, checker − truth) β̂ 2.98e-11, 2.58e-12, 2.72e-11; V 5.99e-11, 5.21e-12, 5.47e-11;
C 1.13e-10, 5.42e-11, 1.03e-10.
"""
from __future__ import annotations

import numpy as np
import pytest

import smooth_long_fixture as LF
from host_check_io import build_host_check, run_smooth_host as run_host


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_check(tmp_path_factory, "tvl_smooth_host_check")


@pytest.mark.parametrize("name,n", LF.case_windows("tvl"))
def test_host_smoother_meets_the_rule(exe, tmp_path, name, n):
    c = LF.cases("tvl")[name]
    B = c["Theta"].shape[1]
    bs, V, C = run_host(exe, tmp_path, 4, c["Y"], c["maturities"], c["Theta"], np.full(B, n))
    for b in range(B):
        LF.assert_candidate("tvl", name, n, b, bs[..., b], V[..., b], C[..., b])


@pytest.mark.parametrize("name,n,b,what", LF.hard_params("tvl"))
def test_hard_candidate_meets_the_rule(exe, tmp_path, name, n, b, what):
    c = LF.cases("tvl")[name]
    bs, V, C = run_host(exe, tmp_path, 4, c["Y"], c["maturities"], c["Theta"][:, b:b + 1], np.full(1, n))
    LF.assert_hard_array("tvl", name, n, b, what, bs[..., 0], V[..., 0], C[..., 0])


def test_mixed_windows_in_one_call_are_the_solo_windows(exe, tmp_path):
    """T_use = (1, 64, 65, 128, 129, 192, 193, 200) over copies of one θ of TL-chunk, each under the rule on its own
    window: the reference that the GPU's mixed-window test leans on."""
    c = LF.cases("tvl")["TL-chunk"]
    tu = np.array(LF.MIXED_WINDOWS)
    Th = np.repeat(c["Theta"][:, :1], len(tu), axis=1)
    bs, V, C = run_host(exe, tmp_path, 4, c["Y"], c["maturities"], Th, tu)
    for k, n in enumerate(tu):
        LF.assert_candidate("tvl", "TL-chunk", int(n), 0, bs[..., k], V[..., k], C[..., k])
