"""Compare the gfx950 device code of this tree with a git revision's, kernel by kernel — the acceptance gate for a
refactor that must not change what the compiler emits.

    python tools/isa_diff.py [--keep <dir>] [<rev>] [<tu> ...]

(rev defaults to HEAD~1; tu = a csrc file stem, e.g. yfm_kernels; default: every csrc/*.hip.)  Each translation
unit of both trees is compiled with build_native's compiler and flags plus --cuda-device-only -S.  Per symbol, the
instruction stream (comments dropped, .LBB<n>_<m> labels renumbered) and the kernel descriptor's .amdhsa_* lines
are compared as text; nothing is looked for inside them.  Exits non-zero on any difference or on a symbol present
on one side only.  yfm_kernels alone takes about two minutes per side.  With --keep, the two streams compared for
each differing symbol are written to <dir>/<tu>/<symbol>.{old,new}.s, for a plain diff to show what moved."""
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))
import build_native as BN  # noqa: E402

CSRC = BN.CSRC.relative_to(ROOT)


def compile_s(root: Path, stem: str, out: Path) -> Path:
    flags = [f"-I{root / 'include'}" if f.startswith("-I") else f for f in BN.FLAGS]
    s = out / f"{stem}.s"
    subprocess.run([BN.HIPCC, *flags, "-w", "--cuda-device-only", "-S", str(root / CSRC / f"{stem}.hip"), "-o", str(s)],
                   check=True)
    return s


def symbols(path: Path) -> dict:
    """symbol → its lines: the body up to .Lfunc_end, then the .amdhsa_* lines of its kernel descriptor."""
    out, cur, desc = {}, None, None
    for line in path.read_text().splitlines():
        if ".amdgpu_metadata" in line:  # the notes after the code restate the descriptors
            break
        line =re.sub(r"(\.L[A-Za-z]+)\d+_", r"\1_", line.split(";")[0]).rstrip()
        m = re.match(r"([A-Za-z_$][\w$.]*):", line)
        k = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if "__hip_cuid_" in line:  # the per-compilation id: its name differs in every build
            cur = None
        elif m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end") or line.lstrip().startswith(".section"):
            cur = None
        elif k:
            desc = out.setdefault(k.group(1), [])
        elif ".end_amdhsa_kernel" in line:
            desc = None
        elif desc is not None:
            desc.append(line.strip())
        elif cur is not None and line.strip():
            cur.append(line)
    return out


def main() -> int:
    args = sys.argv[1:]
    keep = None
    if "--keep" in args:
        i = args.index("--keep")
        if i + 1 >= len(args):
            print("--keep takes a directory", file=sys.stderr)
            return 2
        keep = Path(args[i + 1])
        del args[i:i + 2]
    rev = args.pop(0) if args else "HEAD~1"
    stems = args or sorted(p.stem for p in BN.CSRC.glob("*.hip"))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = Path(tmp) / "old"
        for d in (old, Path(tmp) / "a", Path(tmp) / "b"):
            d.mkdir()
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, str(CSRC), "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", str(old)], input=tar.stdout, check=True)
        # a translation unit the revision does not have is new: nothing to compare it with
        for s in [s for s in stems if not (old / CSRC / f"{s}.hip").exists()]:
            print(f"{s}: new translation unit (not in {rev})")
            stems.remove(s)
        jobs = [(r, s, Path(tmp) / o) for s in stems for r, o in ((old, "a"), (ROOT, "b"))]
        with ThreadPoolExecutor(max_workers=4) as ex:
            files = list(ex.map(lambda j: compile_s(*j), jobs))
        for i, stem in enumerate(stems):
            a, b = symbols(files[2 * i]), symbols(files[2 * i + 1])
            for name in sorted(a.keys() | b.keys()):
                if name not in a or name not in b:
                    verdict = f"only in {rev if name in a else 'the working tree'}"
                elif a[name] == b[name]:
                    verdict = "same"
                else:
                    verdict = f"differs (lines {len(a[name])} → {len(b[name])})"
                    if keep:
                        (keep / stem).mkdir(parents=True, exist_ok=True)
                        for side, lines in (("old", a[name]), ("new", b[name])):
                            (keep / stem / f"{name}.{side}.s").write_text("\n".join(lines) + "\n")
                bad += verdict != "same"
                print(f"{stem} {name}: {verdict}")
    print(f"{bad} differing" if bad else "all same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
