"""CPU test of the smoother's algebra (csrc/yfm_smooth.hpp) at estimation length: tests/smooth_host_check.cpp, unchanged
(host build, -ffp-contract=off, M = 3 and 5; the forward moments come from the header's own predict), on every case and
window of tests/golden/smooth_long/smooth_long_cases.npz under the rule of tests/smooth_long_fixture.py — an ordinary
candidate within 1e-9 of the dense FP64 checker, a hard one within 1e-9 of it or at least as close to the stored 40-digit
truth as the checker is.

Observed, worst array, window and ordinary candidate, result − checker as a fraction of the 1e-9 bar: SL-chunk 2.1e-4,
SL-n64 4.7e-4, SL-hard (bench columns 0, 1) 1.2e-4, GL-chunk 5.1e-3, GL-n30 2.3e-3.  Hard candidates of SL-hard,
(result − checker, result − truth, checker − truth): column 10283 β̂ 5.11e-10, 5.61e-12, 5.17e-10; V 3.41e-9, 7.73e-10,
3.48e-9; C 4.51e-9, 8.14e-10, 5.32e-9; column 1679 β̂ 2.72e-10, 3.93e-13, 2.72e-10; V 1.32e-9, 2.49e-10, 1.35e-9;
C 1.25e-9, 2.49e-10, 1.28e-9.  With a_{t|t} = a_t + P_ts_t, as the header had it before these cases, β̂ of column 10283 was
1.17e-9, 6.52e-10, 5.17e-10 and missed the rule.
"""
from __future__ import annotations

import numpy as np
import pytest

import smooth_long_fixture as LF
from host_check_io import build_host_check, run_smooth_host as run_host


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("smooth_long")
    return {M: build_host_check(d, "smooth_host_check", M=M) for M in (3, 5)}


@pytest.mark.parametrize("name,n", LF.case_windows("fixed"))
def test_host_smoother_meets_the_rule(harness, tmp_path, name, n):
    c = LF.cases("fixed")[name]
    M = LF.SR.STATE_DIM[c["kind"]]
    B = c["Theta"].shape[1]
    bs, V, C = run_host(harness[M], tmp_path, M, c["Y"], c["maturities"], c["Theta"], np.full(B, n))
    for b in range(B):
        LF.assert_candidate("fixed", name, n, b, bs[..., b], V[..., b], C[..., b])


@pytest.mark.parametrize("name,n,b,what", LF.hard_params("fixed"))
def test_hard_candidate_meets_the_rule(harness, tmp_path, name, n, b, what):
    c = LF.cases("fixed")[name]
    M = LF.SR.STATE_DIM[c["kind"]]
    bs, V, C = run_host(harness[M], tmp_path, M, c["Y"], c["maturities"], c["Theta"][:, b:b + 1], np.full(1, n))
    LF.assert_hard_array("fixed", name, n, b, what, bs[..., 0], V[..., 0], C[..., 0])


def test_mixed_windows_in_one_call_are_the_solo_windows(harness, tmp_path):
    """The host program treats candidates one at a time; this pins the reference the GPU's mixed-window test leans on:
    T_use = (1, 64, 65, 128, 129, 192, 193, 200) over copies of one θ of SL-chunk, each under the rule on its window."""
    c = LF.cases("fixed")["SL-chunk"]
    tu = np.array(LF.MIXED_WINDOWS)
    Th = np.repeat(c["Theta"][:, :1], len(tu), axis=1)
    bs, V, C = run_host(harness[3], tmp_path, 3, c["Y"], c["maturities"], Th, tu)
    for k, n in enumerate(tu):
        LF.assert_candidate("fixed", "SL-chunk", int(n), 0, bs[..., k], V[..., k], C[..., k])
