"""Register and scratch budget of the TVλ smoother's backward sweep (csrc/yfm_tvl_smooth.hip), read from the gfx950 code
object in the in-tree library the way test_kernel_resources_cpu.py reads the filter kernels': tvl_smooth_kernel runs
without scratch and without spills, one wave per block, within the register file and within 64 KiB of LDS at the largest
N the TVλ kernels take."""
import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata

TVL_MAX_N = 8 * 256 - 1  # csrc/yfm_tvl.hip tvl_max_n()


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_tvl_smooth_kernel_has_no_scratch_and_no_spills(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "tvl_smooth_kernel" in n}
    assert len(hits) == 1, sorted(meta)
    for n, m in hits.items():
        print(n, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (n, m)
        assert m["vgpr_count"] <= 512, (n, m)
        # static: 64 columns of s, W, L (36 doubles each) and the P_1 system; dynamic: (m, 1/m) per maturity
        assert m["group_segment_fixed_size"] <= 20 * 1024, (n, m)
        assert m["group_segment_fixed_size"] + 16 * TVL_MAX_N <= 64 * 1024, (n, m)
