"""Register and scratch budget of the neural models' full-gradient kernels (csrc/yfm_msedn_adj.hip), read from the
gfx950 code object in the in-tree library.  nns_sweep_kernel, the forward sweep: 2 lane counts × 5 model variants, every
L = 16 instantiation — the one an estimation's launches use — with zero scratch, the L = 4 instantiations pinned at
what they come out with: 12 bytes in the two scaled score-driven variants, as neural_grad_kernel's have, none in the
others.  nns_adjoint_kernel, the backward sweep, is built for 16 lanes alone (it serves either forward lane count: a
candidate's outputs do not depend on it): 5 variants, zero scratch.  Neither name contains one of the substrings the
older kernels' resource tests count by (DESIGN.md §3.10 quotes the counts)."""
import re

import pytest

from test_kernel_resources_cpu import LIB, READELF, _kernel_metadata

# (static, hasB, scaled) → bytes of scratch of the forward sweep at L = 4
L4_SCRATCH = {("1", "0", "0"): 0, ("0", "0", "0"): 0, ("0", "1", "0"): 0, ("0", "0", "1"): 12, ("0", "1", "1"): 12}
OLDER = ("msedn_kernel", "neural_grad_kernel", "lambda_grad_kernel", "lambda_fullgrad_kernel", "msed_kernel")


@pytest.mark.skipif(not LIB.exists() or not READELF.exists(), reason="in-tree library or llvm-readelf missing")
def test_full_gradient_kernel_budget(tmp_path):
    meta = _kernel_metadata(tmp_path)
    sweep = {n: m for n, m in meta.items() if "nns_sweep_kernel" in n}
    adjoint = {n: m for n, m in meta.items() if "nns_adjoint_kernel" in n}
    assert len(sweep) == 10 and len(adjoint) == 5, (sorted(sweep), sorted(adjoint))
    assert not any(s in n for n in list(sweep) + list(adjoint) for s in OLDER)
    seen = set()
    for name, m in sorted({**sweep, **adjoint}.items()):
        which, L, st, hb, sc = re.search(r"nns_(sweep|adjoint)_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)E", name).groups()
        print(f"{which} L={L} static={st} hasB={hb} scaled={sc}: vgpr {m['vgpr_count']} agpr {m['agpr_count']} "
              f"scratch {m['private_segment_fixed_size']} spills {m['vgpr_spill_count']}")
        seen.add((which, int(L), st, hb, sc))
        assert m["vgpr_count"] <= 512, (name, m)
        if int(L) == 16:
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        else:
            assert which == "sweep"
            assert m["private_segment_fixed_size"] == L4_SCRATCH[(st, hb, sc)], (name, m)
            assert m["vgpr_spill_count"] <= 4, (name, m)
    assert len(seen) == 15
