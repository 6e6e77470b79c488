"""CPU test of the LDS layouts of the two TVλ loglik kernels (csrc/yfm_tvl_layout.hpp: TvlSmem, TvlDdSmem), which
the kernels carve their shared memory from and whose bytes() their launchers pass.  tests/tvl_layout_host_check.cpp, a
stand-alone program built with -fsanitize=address,undefined, holds both structs to the pointer chains and the two
byte-count formulas they replace: equal totals, equal offsets, 16-byte alignment of the double2 / dd regions wherever
the former chain had it, disjoint regions.

Cases: N ∈ {1, 3, 4, 7, 30, 33, 360, 2047}, the columns per chunk chunk_columns gives for each N, L ∈ {1 … 64} (FP64)
and {4 … 64} (dd); and the dd launcher's 160 KiB refusal at the first N where it triggers (N = 2,758 at L = 4: beyond
the N ≤ 2,048 the chunk rule admits, which the program also asserts).
"""
from __future__ import annotations

import subprocess

from host_check_io import build_host_check


def test_layout_structs_match_the_former_chains(tmp_path):
    exe = build_host_check(tmp_path, "tvl_layout_host_check", sanitize=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    assert "96 layouts checked, 0 failures" in out.stdout
    assert "dd L=4: LDS refusal first at N=2758" in out.stdout
