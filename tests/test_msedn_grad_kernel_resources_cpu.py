"""Register and scratch budget of the neural models' gradient kernels (csrc/yfm_msedn.hip neural_grad_kernel), read
from the gfx950 code object in the in-tree library: 2 lane counts × 5 model variants.  Every L = 16 instantiation —
the one an estimation's gradient launches use — has zero scratch with the 12 accumulators, the kept β and Z'v
replicated on every lane of a group.  The L = 4 instantiations (batches above 8,192 candidates) are pinned at what
they come out with: 12 bytes in the two scaled score-driven variants, as three of the loss kernel's L = 4
instantiations have, none in the others (DESIGN.md §3.7 quotes the counts)."""
import re

import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata

# (static, hasB, scaled) → bytes of scratch at L = 4
L4_SCRATCH = {("1", "0", "0"): 0, ("0", "0", "0"): 0, ("0", "1", "0"): 0, ("0", "0", "1"): 12, ("0", "1", "1"): 12}


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_neural_grad_kernel_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "neural_grad_kernel" in n}
    assert len(hits) == 10, sorted(hits)
    assert not any("msedn_kernel" in n for n in hits)  # the loss kernel's resources test counts that substring
    seen = set()
    for name, m in sorted(hits.items()):
        L, st, hb, sc = re.search(r"neural_grad_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        print(f"L={L} static={st} hasB={hb} scaled={sc}: vgpr {m['vgpr_count']} agpr {m['agpr_count']} "
              f"scratch {m['private_segment_fixed_size']} spills {m['vgpr_spill_count']}")
        seen.add((int(L), st, hb, sc))
        assert m["vgpr_count"] <= 512, (name, m)
        if int(L) == 16:
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        else:
            assert m["private_segment_fixed_size"] == L4_SCRATCH[(st, hb, sc)], (name, m)
            assert m["vgpr_spill_count"] <= 4, (name, m)
    assert len(seen) == 10
