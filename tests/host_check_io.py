"""Input and output of the host check programs (tests/grad_host_check.cpp, tests/score_host_check.cpp): one text file
in — N T B space, N maturities, the N×T panel column by column, then per candidate T_use and its θ, doubles as C hex
floats or "nan" — and lines of hex floats out.  Shared by tests/test_score_host_cpu.py and tools/hessian_step_table.py."""
from __future__ import annotations

import subprocess

import numpy as np


def hexf(v) -> str:
    return "nan" if v != v else float(v).hex()


def run_program(exe, tmp_path, Y, m, Th, tu, space=0):
    """The program's output rows (lists of floats), blank lines dropped."""
    N, T = Y.shape
    B = Th.shape[1]
    words = [str(N), str(T), str(B), str(space)]
    words += [hexf(v) for v in m]
    words += [hexf(v) for v in np.asarray(Y).reshape(-1, order="F")]
    for b in range(B):
        words.append(str(int(tu[b])))
        words += [hexf(v) for v in Th[:, b]]
    path = tmp_path / "case.txt"
    path.write_text(" ".join(words))
    out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    return [[float.fromhex(v) if "0x" in v else float(v) for v in line.split()] for line in out if line]


def run_grad_host(exe, tmp_path, Y, m, Th, tu, space=0):
    """(ll[B], g[P, B]) of grad_host_check: one line ll g_0 … g_{P−1} per candidate."""
    rows = np.array(run_program(exe, tmp_path, Y, m, Th, tu, space))
    assert rows.shape[0] == Th.shape[1]
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
