"""Register and scratch budget of the λ models' gradient kernels (csrc/yfm_msed.hip lambda_grad_kernel), read from
the gfx950 code object in the in-tree library: every instantiation — 2 lane counts × 5 model variants — has zero
scratch with the 12 accumulators replicated on every lane of a group (DESIGN.md §3.6 quotes the counts)."""
import re

import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_lambda_grad_kernels_have_no_scratch(tmp_path):
    meta = _kernel_metadata(tmp_path)
    hits = {n: m for n, m in meta.items() if "lambda_grad_kernel" in n}
    assert len(hits) == 10, sorted(hits)
    seen = set()
    for name, m in sorted(hits.items()):
        L, st, hb, sc = re.search(r"lambda_grad_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        print(f"L={L} static={st} hasB={hb} scaled={sc}: vgpr {m['vgpr_count']} agpr {m['agpr_count']}")
        seen.add((int(L), st, hb, sc))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 512, (name, m)
    assert len(seen) == 10
