"""CPU test of the neural models' δ/Φ loss gradient (csrc/yfm_msedn.hpp loss_and_grad with csrc/yfm_msed.hpp's accum_zv,
grad_accum, grad_finish — the functions the gfx950 gradient kernel runs) compiled for the host
(tests/msedn_grad_host_check.cpp, -ffp-contract=off, -fsanitize=address,undefined, a stand-alone program) against
tests/golden/msedn_grad/: central differences of the 40-digit restatement.  Every fixture candidate, in both parameter
spaces, passes the rule of tests/test_gpu_grad.py, max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd; a −Inf loss comes with 12
NaNs, exactly where the fixture has them."""
from __future__ import annotations

import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(GOLDEN / "msedn_grad"))
import make_msedn_grad as MG  # noqa: E402

REL = 1e-9


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("msedn_grad") / "msedn_grad_host_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "msedn_grad_host_check.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


def hexf(v) -> str:
    return "nan" if v != v else float(v).hex()


def run_host(exe, tmp_path, kind, Y, m, Th, tu, space):
    """(loss[B], get_loss[B], grad[12, B]) from the host build."""
    N, T = Y.shape
    B = Th.shape[1]
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
    assert rows.shape == (B, 14)
    return rows[:, 0], rows[:, 1], rows[:, 2:].T


def check_gradient(g, g_fd, e_fd, loss, label=""):
    """The fixture rule per candidate (column); the NaN pattern must be the fixture's, which is the −Inf pattern.
    Returns the worst error relative to ‖g_fd‖∞."""
    worst = 0.0
    for b in range(g.shape[1]):
        if np.isnan(g_fd[:, b]).any():
            assert np.isneginf(loss[b]) and np.isnan(g[:, b]).all(), (label, b, loss[b], g[:, b])
            continue
        assert np.isfinite(loss[b]) and np.isfinite(g[:, b]).all(), (label, b, loss[b], g[:, b])
        err = np.max(np.abs(g[:, b] - g_fd[:, b]))
        scale = np.max(np.abs(g_fd[:, b]))
        bound = REL * scale + e_fd[b]
        print(f"{label} b={b}: max|g - g_fd| = {err:.3e}, bound {bound:.3e}, |g|inf = {scale:.3e}")
        assert err <= bound, (label, b, err, bound)
        worst = max(worst, err / scale)
    return worst


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


@pytest.mark.parametrize("space", [0, 1])
@pytest.mark.parametrize("name", MG.case_names())
def test_host_gradient_matches_truth(harness, cases, tmp_path, name, space):
    c = cases
    Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
    loss, loss_plain, g = run_host(harness, tmp_path, kind_of(name), c[f"{name}_Y"], c[f"{name}_maturities"], Th,
                                   c[f"{name}_T_use"], space)
    # the loss beside the gradient is get_loss's, sum for sum
    assert np.array_equal(loss, loss_plain), (loss, loss_plain)
    want = c[f"{name}_loss_s{space}"]
    assert np.array_equal(np.isneginf(loss), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.all(np.abs(loss[fin] - want[fin]) <= 1e-9 * np.abs(want[fin]))  # the project's parity bar
    check_gradient(g, c[f"{name}_g_fd_s{space}"], c[f"{name}_e_fd_s{space}"], loss, f"{name} space {space}")


def test_fixture_covers_the_special_cases(cases):
    """The window over the missing column is −Inf with no gradient; the leading NaN column leaves every gradient
    finite; the restatement's own analytic gradient is ten times inside the bar for every stored candidate."""
    for kind in MG.kinds():
        assert np.isnan(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 1:]).all()
        assert np.isfinite(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 0]).all()
        assert np.isnan(cases[f"k{kind}_n4t8nan6_Y"][:, 5]).all()
        for tag in ("n4t8nan0", "n30t8nan0"):
            assert np.isnan(cases[f"k{kind}_{tag}_Y"][:, 0]).all()
            assert np.isfinite(cases[f"k{kind}_{tag}_g_fd_s1"]).all()
    for name in MG.case_names():
        for space in (0, 1):
            g_fd, e_fd, rerr = (cases[f"{name}_{k}_s{space}"] for k in ("g_fd", "e_fd", "rerr"))
            fin = np.isfinite(e_fd)
            assert np.all(rerr[fin] <= MG.SELF_REL * np.max(np.abs(g_fd[:, fin]), axis=0) + e_fd[fin]), (name, space)
    print("worst restatement error relative to |g_fd|inf:", float(cases["worst_restatement_rel"]))
