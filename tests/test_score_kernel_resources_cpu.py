"""Register and scratch budget of the score and OPG kernels (csrc/yfm_score.hip), read from the gfx950 code object in
the in-tree library the way test_grad_kernel_resources_cpu.py reads the gradient kernel's: dns_score_kernel runs
dns_grad_kernel's recursion and stores a term per step, so it has no scratch and no more registers than that kernel
(DESIGN.md §3.11 states no allowance on top); opg_kernel has no scratch."""
import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata, only


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_score_and_opg_kernels_within_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)

    grad, score, opg = only(meta, "dns_grad_kernel"), only(meta, "dns_score_kernel"), only(meta, "opg_kernel")
    assert score["private_segment_fixed_size"] == 0 and score["vgpr_spill_count"] == 0, score
    assert score["vgpr_count"] <= grad["vgpr_count"] and score["agpr_count"] <= grad["agpr_count"], (score, grad)
    assert opg["private_segment_fixed_size"] == 0 and opg["vgpr_spill_count"] == 0, opg
    assert opg["vgpr_count"] <= 128, opg
