"""CPU test of the neural models' full loss gradient (csrc/yfm_msedn_adj.hpp loss_and_fullgrad — the step routines and
the adjoint step the gfx950 kernels run) compiled for the host (tests/msedn_fullgrad_host_check.cpp,
-ffp-contract=off, -fsanitize=address,undefined, a stand-alone program) against tests/golden/msedn_fullgrad/: central
differences of the 40-digit restatement over the leading rows.  Every fixture candidate, in the spaces stored, passes
max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd over the leading rows; the loss and the last 12 rows are loss_and_grad's bit for
bit; a −Inf loss comes with P NaNs, exactly where the fixture has them."""
from __future__ import annotations

import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(GOLDEN / "msedn_fullgrad"))
import make_msedn_fullgrad as MF  # noqa: E402

REL = 1e-9


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("msedn_fullgrad") / "msedn_fullgrad_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "msedn_fullgrad_host_check.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def cases():
    return MF.load_cases()


def hexf(v) -> str:
    return "nan" if v != v else float(v).hex()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run_host(exe, tmp_path, kind, Y, m, Th, tu, space):
    """(loss[B], loss_and_grad's loss[B], unavailable[B], grad[P, B], loss_and_grad's grad[12, B])."""
    N, T = Y.shape
    P, B = Th.shape
    words = [str(kind), str(N), str(T), str(B), str(space)]
    words += [hexf(v) for v in m]
    words += [hexf(v) for v in np.asarray(Y).reshape(-1, order="F")]
    for b in range(B):
        words.append(str(int(tu[b])))
        words += [hexf(v) for v in Th[:, b]]
    path = tmp_path / "case.txt"
    path.write_text(" ".join(words))
    out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = np.array([[float.fromhex(v) if "0x" in v else float(v) for v in line.split()] for line in out if line])
    assert rows.shape == (B, 3 + P + 12)
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:3 + P].T, rows[:, 3 + P:].T


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


def check_leading(g, g_fd, e_fd, loss, label=""):
    """The fixture rule per candidate over the leading rows; the NaN pattern is the fixture's −Inf pattern."""
    nl = g_fd.shape[0]
    for b in range(g.shape[1]):
        if np.isnan(g_fd[:, b]).any():
            assert np.isneginf(loss[b]) and np.isnan(g[:, b]).all(), (label, b, loss[b], g[:, b])
            continue
        assert np.isfinite(loss[b]) and np.isfinite(g[:, b]).all(), (label, b, loss[b], g[:, b])
        err = np.max(np.abs(g[:nl, b] - g_fd[:, b]))
        bound = REL * np.max(np.abs(g_fd[:, b])) + e_fd[b]
        print(f"{label} b={b}: max|g - g_fd| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (label, b, err, bound)


@pytest.mark.parametrize("name", MF.case_names())
def test_host_full_gradient_matches_truth(harness, cases, tmp_path, name):
    c = cases
    for space in MF.case_spaces(name):
        Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
        loss, loss12, un, g, g12 = run_host(harness, tmp_path, kind_of(name), c[f"{name}_Y"], c[f"{name}_maturities"],
                                            Th, c[f"{name}_T_use"], space)
        assert same_bits(loss, loss12) and not un.any()
        fin = np.isfinite(loss)
        assert same_bits(g[-12:, fin], g12[:, fin]) and np.isnan(g[:, ~fin]).all()
        want = c[f"{name}_loss_s{space}"]
        assert np.array_equal(np.isneginf(loss), np.isneginf(want))
        assert np.all(np.abs(loss[fin] - want[fin]) <= 1e-9 * np.abs(want[fin]))
        check_leading(g, c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


def test_window_without_a_compared_column(harness, cases, tmp_path):
    """T_use = 1: the loss of loss_and_grad and an exactly zero gradient (no trajectory record is touched)."""
    for kind in MF.kinds():
        name = f"k{kind}_n4t8"
        c = cases
        loss, loss12, un, g, _ = run_host(harness, tmp_path, kind, c[f"{name}_Y"], c[f"{name}_maturities"],
                                          c[f"{name}_theta"], [1, 8], 0)
        assert same_bits(loss, loss12) and not un.any()
        assert np.all(g[:, 0] == 0.0) and np.any(g[:, 1] != 0.0)
