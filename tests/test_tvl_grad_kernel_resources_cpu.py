"""Register and scratch budget of the TVλ gradient kernel (csrc/yfm_tvl_grad.hip), read from the gfx950 code object
in the in-tree library: one instantiation (one lane mapping, whatever the batch), zero scratch and at most 512
registers per lane (the committed build: 256 VGPR + 212 AGPR, nothing spilled).

This test is the only guard of the kernel's zero scratch, which rests on three places where a loop-invariant value is
hidden from the optimiser so that it is formed where it is used instead of being carried in a register across the step
loop: the group's LDS offset and each direction's index pass through an empty asm, and the lane's index in its group
is formed again from mbcnt (fresh_group_lane).  A compiler that sees through them, or a source change that adds live
state, brings the spills back (16 lanes × 2 directions spills 57 VGPRs, 8 × 4 spills 421): the remedy is fewer live
values or more lanes per candidate, not scratch."""
import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_tvl_grad_kernel_within_register_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = [(n, m) for n, m in meta.items() if "tvl_grad_kernel" in n]
    assert len(hits) == 1, sorted(meta)
    name, m = hits[0]
    print(name, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= 512, m
