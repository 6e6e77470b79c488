"""Register and scratch budget of the smoother's backward sweep (csrc/yfm_smooth.hip), read from the gfx950 code object
in the in-tree library the way test_kernel_resources_cpu.py reads the filter kernels': both instantiations of
smooth_kernel (M = 3 DNS, M = 5 GNS5) run without scratch and without spills, one wave per block, with the per-chunk
operands, Z and the P_1 system in LDS."""
import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_smooth_kernels_have_no_scratch_and_no_spills(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "smooth_kernelILi" in n}
    assert len(hits) == 2 and any("ILi3E" in n for n in hits) and any("ILi5E" in n for n in hits), sorted(meta)
    for n, m in hits.items():
        print(n, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (n, m)
        assert m["vgpr_count"] <= 512, (n, m)
        # 64 columns of s, W, L (M + 2M² doubles each), Z (64 × M) and the P_1 system
        assert m["group_segment_fixed_size"] <= 34 * 1024, (n, m)
    mark = [m for n, m in meta.items() if "smooth_mark_deferred_kernel" in n]
    assert len(mark) == 1 and mark[0]["private_segment_fixed_size"] == 0
