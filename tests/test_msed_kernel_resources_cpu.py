"""Register and scratch budget of the λ-model kernels (csrc/yfm_msed.hip), read from the gfx950 code object in the
in-tree library: every instantiation — 2 lane counts × 5 model variants × {loss, record} — has zero scratch.
The counts recorded here are the ones DESIGN.md §3.6 quotes; one candidate per lane (L = 1) was built and is not
instantiated because its in-lane summation tree spilled (650–770 bytes of scratch)."""
import re

import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata

# registers per lane (arch VGPRs + AGPRs the allocator uses as copies; no scratch), by (L, static, has B, scaled, record)
RECORDED_MAX = {16: 232, 4: 306}


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_msed_kernels_have_no_scratch(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "msed_kernel" in n}
    assert len(hits) == 20, sorted(hits)
    seen = set()
    for name, m in sorted(hits.items()):
        L, st, hb, sc, rec = re.search(r"msed_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        print(f"L={L} static={st} hasB={hb} scaled={sc} record={rec}: vgpr {m['vgpr_count']} agpr {m['agpr_count']}")
        seen.add((int(L), st, hb, sc, rec))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 512, (name, m)
        # a build that needs many more registers than recorded has changed shape: look before raising these
        assert m["vgpr_count"] <= RECORDED_MAX[int(L)] + 32, (name, m)
    assert len(seen) == 20
