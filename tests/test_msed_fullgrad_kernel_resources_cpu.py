"""Register and scratch budget of the λ models' full-gradient kernels (csrc/yfm_msed.hip lambda_fullgrad_kernel), read
from the gfx950 code object in the in-tree library: every instantiation — 2 lane counts × 5 model variants — with the
candidate's record (δ/Φ accumulators, tangents, leading accumulators) in LDS.  The scaled kinds at 4 lanes keep 12
bytes of scratch (6 spilled registers), everything else none (DESIGN.md §3.9 quotes the counts)."""
import re

import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata

# (L, static, hasB, scaled) → scratch bytes
SCRATCH = {(4, "0", "0", "1"): 12, (4, "0", "1", "1"): 12}


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_lambda_fullgrad_kernels_keep_their_scratch_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "lambda_fullgrad_kernel" in n}
    assert len(hits) == 10, sorted(hits)
    seen = set()
    for name, m in sorted(hits.items()):
        L, st, hb, sc = re.search(r"lambda_fullgrad_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        print(f"L={L} static={st} hasB={hb} scaled={sc}: vgpr {m['vgpr_count']} agpr {m['agpr_count']} "
              f"scratch {m['private_segment_fixed_size']} spilled {m['vgpr_spill_count']}")
        key = (int(L), st, hb, sc)
        seen.add(key)
        assert m["private_segment_fixed_size"] == SCRATCH.get(key, 0), (name, m)
        assert m["vgpr_count"] <= 512, (name, m)
    assert len(seen) == 10
