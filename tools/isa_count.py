"""Count instructions in a kernel's gfx950 assembly (hipcc --cuda-device-only -S, build_native's flags): the
FP64 work of its largest basic blocks and of the regions between its workgroup barriers, and its resources.

    python tools/isa_count.py <file.s> <symbol-regex> [--blocks K]

Per matching kernel: VGPR / AGPR / scratch / LDS from its descriptor; the K basic blocks with the most FP64
instructions (all instructions, FP64 arithmetic = v_fma/v_mul/v_add/v_max/v_min/v_ldexp/v_rcp/v_div*/…_f64, MFMA,
selects); and, between consecutive s_barrier instructions in program order, the same counts plus the FP64 division
chains (one v_div_fixup_f64 each).  The steady block of fixedz_loglik_kernel<30,3,1,false,true,false> is its
largest block without MFMAs; its setup is the region between the first two barriers."""
import re
import sys
from pathlib import Path


def classify(ins: str) -> str:
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_cndmask"):
        return "select"
    if op.endswith("_f64") or "_f64_" in op:
        return "fp64"
    return "other"


def kernels(path: Path):
    """symbol → (instruction lines with labels, descriptor lines)"""
    out, cur, desc = {}, None, None
    for raw in path.read_text().splitlines():
        if ".amdgpu_metadata" in raw:
            break
        line = raw.split(";")[0].rstrip()
        m = re.match(r"([A-Za-z_$][\w$.]*):", line)
        k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m and not m.group(1).startswith(".L"):
            cur = out.setdefault(m.group(1), ([], []))[0]
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif k:
            desc = out.setdefault(k.group(1), ([], []))[1]
        elif ".end_amdhsa_kernel" in line:
            desc = None
        elif desc is not None:
            desc.append(line.strip())
        elif cur is not None and line.strip():
            cur.append(line.strip())
    return out


def main() -> int:
    args = sys.argv[1:]
    top = 3
    if "--blocks" in args:
        i = args.index("--blocks")
        top = int(args[i + 1])
        del args[i:i + 2]
    path, pat = Path(args[0]), re.compile(args[1])
    for name, (body, desc) in kernels(path).items():
        if not pat.search(name) or not body:
            continue
        d = dict(l.split(None, 1) for l in desc if " " in l)
        print(f"{name}")
        print(f"  vgpr {d.get('.amdhsa_next_free_vgpr')} (accum offset {d.get('.amdhsa_accum_offset')}) sgpr "
              f"{d.get('.amdhsa_next_free_sgpr')} scratch {d.get('.amdhsa_private_segment_fixed_size')} B lds "
              f"{d.get('.amdhsa_group_segment_fixed_size')} B")
        blocks, cur = [], {"label": "entry", "n": 0, "fp64": 0, "mfma": 0, "select": 0, "other": 0}
        regions = [{"n": 0, "fp64": 0, "mfma": 0, "select": 0, "other": 0, "div": 0}]

        def close():
            nonlocal cur
            if cur["n"]:
                blocks.append(cur)

        for ins in body:
            if ins.endswith(":"):
                close()
                cur = {"label": ins[:-1], "n": 0, "fp64": 0, "mfma": 0, "select": 0, "other": 0}
                continue
            if ins.startswith("."):
                continue
            c = classify(ins)
            cur["n"] += 1
            cur[c] += 1
            r = regions[-1]
            r["n"] += 1
            r[c] += 1
            r["div"] += ins.startswith("v_div_fixup_f64")
            if ins.startswith("s_barrier"):
                regions.append({"n": 0, "fp64": 0, "mfma": 0, "select": 0, "other": 0, "div": 0})
            if ins.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
                close()
                cur = {"label": cur["label"] + "+", "n": 0, "fp64": 0, "mfma": 0, "select": 0, "other": 0}
        close()
        for b in sorted(blocks, key=lambda b: -b["fp64"])[:top]:
            print(f"  block {b['label']}: {b['n']} instructions, fp64 {b['fp64']}, mfma {b['mfma']}, selects {b['select']}")
        for i, r in enumerate(regions):
            print(f"  region {i} (barrier {i} → {i + 1}): {r['n']} instructions, fp64 {r['fp64']}, mfma {r['mfma']}, "
                  f"selects {r['select']}, fp64 divisions {r['div']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
