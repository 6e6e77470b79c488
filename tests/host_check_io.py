"""The host check programs (tests/*_check.cpp: stand-alone programs with their own main, never loaded into Python):
how each is compiled, and the text protocol of those that read a case file — [kind] N T B space, N maturities, the N×T
panel column by column, then per candidate T_use and its θ, doubles as C hex floats or "nan" — and lines of hex floats
out.  Shared by the *_host_cpu.py tests and the two tools/*hessian_step_table.py (the TVλ one keeps a compile line of
its own: tests import it as a module)."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]

STD = ("-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas")
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
PLAIN_BUILD = ("-O2", *STD)
SAN_BUILD = ("-O1", "-g", *STD, *SAN)

# program → {sanitize: its flags}.  The table is the record of how each program is built; a build it does not list is
# refused.  (smooth_host_check also takes -DYFM_SMOOTH_M=3 or 5 from its caller.)
HOST_CHECKS = {
    "grad_host_check": {False: PLAIN_BUILD},
    "tvl_grad_host_check": {False: PLAIN_BUILD},
    "nm_tree_check": {False: PLAIN_BUILD},
    "score_host_check": {False: PLAIN_BUILD, True: SAN_BUILD},
    "tvl_score_host_check": {False: PLAIN_BUILD, True: SAN_BUILD},
    "smooth_host_check": {False: PLAIN_BUILD, True: SAN_BUILD},
    "tvl_smooth_host_check": {False: PLAIN_BUILD, True: SAN_BUILD},
    "kalman_map_host_check": {False: PLAIN_BUILD, True: SAN_BUILD},
    "msed_host_check": {True: SAN_BUILD},
    "msed_grad_host_check": {True: SAN_BUILD},
    "msed_fullgrad_host_check": {True: SAN_BUILD},
    "msedn_host_check": {True: SAN_BUILD},
    "msedn_grad_host_check": {True: SAN_BUILD},
    "msedn_fullgrad_host_check": {True: SAN_BUILD},
    "tvl_layout_host_check": {True: ("-O1", "-g", "-std=c++17", "-Wall", "-Werror", *SAN)},
    "fixedz_mean_host_check": {True: (*SAN_BUILD, f"-I{ROOT / 'tools' / 'host_fixedz' / 'stub'}",
                                      f"-I{ROOT / 'yieldfactormodels.jl_amd' / 'csrc'}", "-lquadmath")},
}


def build_host_check(tmp, stem, *, sanitize=False, M=None):
    """Compile tests/<stem>.cpp with its flags of HOST_CHECKS and return the executable.  `tmp` is pytest's
    tmp_path_factory or a directory."""
    d = Path(tmp.mktemp(stem) if hasattr(tmp, "mktemp") else tmp)
    exe = d / (stem + ("_san" if sanitize else "") + (f"_{M}" if M else ""))
    smooth_m = [f"-DYFM_SMOOTH_M={M}"] if M else []
    subprocess.run(["g++", str(ROOT / "tests" / f"{stem}.cpp"), "-o", str(exe), *HOST_CHECKS[stem][sanitize],
                    *smooth_m], check=True)
    return exe


def hexf(v) -> str:
    return "nan" if v != v else float(v).hex()


def run_program(exe, tmp_path, Y, m, Th, tu, space=0, kind=None):
    """The program's output rows (lists of floats), blank lines dropped."""
    N, T = Y.shape
    B = Th.shape[1]
    words = ([] if kind is None else [str(kind)]) + [str(N), str(T), str(B), str(space)]
    words += [hexf(v) for v in m]
    words += [hexf(v) for v in np.asarray(Y).reshape(-1, order="F")]
    for b in range(B):
        words.append(str(int(tu[b])))
        words += [hexf(v) for v in Th[:, b]]
    path = tmp_path / "case.txt"
    path.write_text(" ".join(words))
    out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    return [[float.fromhex(v) if "0x" in v else float(v) for v in line.split()] for line in out if line]


def run_rows(exe, tmp_path, Y, m, Th, tu, space=0, kind=None, width=None):
    """One output line per candidate, as rows[B, width]."""
    rows = np.array(run_program(exe, tmp_path, Y, m, Th, tu, space, kind))
    assert rows.shape[0] == Th.shape[1] and (width is None or rows.shape[1] == width), rows.shape
    return rows


def run_grad_host(exe, tmp_path, Y, m, Th, tu, space=0):
    """(ll[B], g[P, B]) of grad_host_check and tvl_grad_host_check: one line ll g_0 … g_{P−1} per candidate."""
    rows = run_rows(exe, tmp_path, Y, m, Th, tu, space)
    return rows[:, 0], rows[:, 1:].T


def run_score_host(exe, tmp_path, Y, m, Th, tu, space=0):
    """(ll[B], g[P, B], S[P, T−1, B]) of score_host_check: per candidate the gradient line, then T − 1 score columns."""
    T = Y.shape[1]
    P, B = Th.shape
    rows = run_program(exe, tmp_path, Y, m, Th, tu, space)
    assert len(rows) == B * T
    ll, g, Sc = np.empty(B), np.empty((P, B)), np.empty((P, T - 1, B))
    for b in range(B):
        head = rows[b * T]
        ll[b], g[:, b] = head[0], head[1:]
        Sc[:, :, b] = np.array(rows[b * T + 1:(b + 1) * T]).T
    return ll, g, Sc


def run_loss_host(exe, tmp_path, kind, Y, m, Th, tu, space):
    """loss[B] of msed_host_check and msedn_host_check."""
    return run_rows(exe, tmp_path, Y, m, Th, tu, space, kind, width=1)[:, 0]


def run_kind_grad_host(exe, tmp_path, kind, Y, m, Th, tu, space):
    """(loss[B], get_loss[B], grad[12, B]) of msed_grad_host_check and msedn_grad_host_check."""
    rows = run_rows(exe, tmp_path, Y, m, Th, tu, space, kind, width=14)
    return rows[:, 0], rows[:, 1], rows[:, 2:].T


def run_fullgrad_host(exe, tmp_path, kind, Y, m, Th, tu, space):
    """(loss[B], the δ/Φ program's loss[B], unavailable[B], grad[P, B], the δ/Φ gradient [12, B]) of
    msed_fullgrad_host_check and msedn_fullgrad_host_check."""
    P = Th.shape[0]
    rows = run_rows(exe, tmp_path, Y, m, Th, tu, space, kind, width=3 + P + 12)
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:3 + P].T, rows[:, 3 + P:].T


def run_smooth_host(exe, tmp_path, M, Y, m, Th, tu, space=0):
    """(beta_s[M, T, B], V_s[M, M, T, B], C_s[M, M, T − 1, B]) of smooth_host_check (M = 3, 5) and
    tvl_smooth_host_check (M = 4): T lines per candidate."""
    T, B = Y.shape[1], Th.shape[1]
    rows = np.array(run_program(exe, tmp_path, Y, m, Th, tu, space)).reshape(B, T, M + 2 * M * M)
    bs = rows[:, :, :M].transpose(2, 1, 0)
    V = rows[:, :, M:M + M * M].reshape(B, T, M, M).transpose(3, 2, 1, 0)  # column-major M × M per line
    C = rows[:, :, M + M * M:].reshape(B, T, M, M).transpose(3, 2, 1, 0)[:, :, :T - 1]
    return bs, V, C
