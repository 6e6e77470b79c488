"""Register and scratch budget of the TVλ score kernel (csrc/yfm_tvl_score.hip) and of the 31-row OPG kernel
(csrc/yfm_score.hip), read from the gfx950 code object in the in-tree library the way
test_tvl_grad_kernel_resources_cpu.py reads the gradient kernel's.  tvl_score_kernel runs tvl_grad_kernel's recursion,
which fills the 512 registers of a 256-thread block, and stores a term per step: everything the store needs is formed at
the store, so it has no scratch and no spilled VGPR either.  opg31_kernel has opg_kernel's limits."""
import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata, only


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_tvl_score_and_opg31_kernels_within_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)

    score, opg = only(meta, "tvl_score_kernel"), only(meta, "opg31_kernel")
    assert score["private_segment_fixed_size"] == 0 and score["vgpr_spill_count"] == 0, score
    assert score["vgpr_count"] <= 512, score  # VGPRs and AGPRs together (gfx950's unified file)
    assert opg["private_segment_fixed_size"] == 0 and opg["vgpr_spill_count"] == 0, opg
    assert opg["vgpr_count"] <= 128 and opg.get("group_segment_fixed_size", 0) == 0, opg
