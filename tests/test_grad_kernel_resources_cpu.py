"""Register and scratch budget of the DNS gradient kernel (csrc/yfm_grad.hip), read from the gfx950 code object in
the in-tree library: zero scratch and at most 512 registers per lane, as for the other hot kernels.  The
kernel carries 3 tangent directions per lane; a change that makes it spill must move to more lanes per candidate
instead."""
import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_grad_kernel_within_register_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = [(n, m) for n, m in meta.items() if "dns_grad_kernel" in n]
    assert len(hits) == 1, sorted(meta)
    name, m = hits[0]
    print(name, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= 512, m
