"""Register and scratch budget of the neural-model kernels (csrc/yfm_msedn.hip), read from the gfx950 code object
in the in-tree library: 2 lane counts × 5 step variants (static; B or random walk × plain or scaled) × {loss,
record} = 20 instantiations.  Every L = 16 instantiation — the lane count of every launch up to 8,192 candidates —
has zero scratch.  The L = 4 instantiations are pinned at the bytes of the build DESIGN.md §3.7 describes: a
change in either direction is a change of shape to look at."""
import re

import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata

# scratch bytes per lane at L = 4 by (static, has B, scaled, record); everything not listed: 0
# the three scaled instantiations below keep one double of the step in scratch (stored once, reloaded two or three
# times per step: 8 bytes, 12 with the slot's padding)
L4_SCRATCH = {("0", "0", "1", "0"): 12, ("0", "0", "1", "1"): 12, ("0", "1", "1", "0"): 12}


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_msedn_kernels_scratch(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "msedn_kernel" in n}
    assert len(hits) == 20, sorted(hits)
    seen = set()
    for name, m in sorted(hits.items()):
        L, st, hb, sc, rec = re.search(r"msedn_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        print(f"L={L} static={st} hasB={hb} scaled={sc} record={rec}: vgpr {m['vgpr_count']} agpr {m['agpr_count']} "
              f"scratch {m['private_segment_fixed_size']} spilled {m['vgpr_spill_count']}")
        seen.add((int(L), st, hb, sc, rec))
        assert m["vgpr_count"] <= 512, (name, m)
        if int(L) == 16:
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        else:
            assert m["private_segment_fixed_size"] == L4_SCRATCH.get((st, hb, sc, rec), 0), (name, m)
    assert len(seen) == 20
