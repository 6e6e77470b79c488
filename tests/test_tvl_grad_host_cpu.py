"""CPU test of the TVλ gradient's tangent algebra (csrc/yfm_tvl_grad.hpp): the functions the gfx950 kernel runs,
compiled for the host (tests/tvl_grad_host_check.cpp, -ffp-contract=off) and run one candidate at a time on every
case of the fixture (tests/golden/tvl_grad), held to the GPU test's rule:

    max_i |g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]   for every compared candidate, at least 75% compared.

The estimation-length cases of tvl_grad_long_cases.npz (T = 200 and 600, make_tvl_grad_long.py) run through the same
program.
"""
from __future__ import annotations

import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, str(GOLDEN / "tvl_grad"))
import make_tvl_grad as MG  # noqa: E402
import make_tvl_grad_long as ML  # noqa: E402

REL = 1e-9
POS = (0, 1, 3, 6, 10)     # σ² and the diagonal of U: exp
R11 = (15, 20, 25, 30)     # the diagonal of Φ: 2eˣ/(1+eˣ) − 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tvl_grad") / "tvl_grad_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                    str(ROOT / "tests" / "tvl_grad_host_check.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def cases():
    return MG.load_cases()


def hexf(v) -> str:
    return "nan" if v != v else float(v).hex()


def run_host(exe, tmp_path, Y, m, Th, tu, space=0):
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
    rows = np.array([[float.fromhex(v) if "0x" in v else float(v) for v in line.split()] for line in out[:B]])
    return rows[:, 0], rows[:, 1:].T


def check_case(c, ll, g):
    cmp_ = c["compared"]
    assert cmp_.mean() >= 0.75
    gn = np.abs(c["g_fd"]).max(axis=0)
    err = np.abs(g - c["g_fd"]).max(axis=0)
    bound = REL * gn + c["e_fd"]
    live = cmp_ & (gn > 0)
    if live.any():
        print("max err / bound over the compared:", np.max(err[live] / bound[live]),
              "max err / |g|:", np.max(err[live] / gn[live]))
    assert np.all(err[cmp_] <= bound[cmp_]), (err[live] / gn[live]).max()
    zero = c["g_fd"] == 0.0
    assert np.all(g[zero & cmp_[None, :]] == 0.0)
    assert np.all(g[:, c["T_use"] <= 2] == 0.0)
    # the recursion's own FP64 value is not what the library returns (that is the loglik launch's); its distance
    # from the truth is printed only
    fin = np.isfinite(c["loglik_truth"]) & cmp_
    den = np.maximum(np.abs(c["loglik_truth"][fin]), 1.0)
    print("FP64 primal: max |ll − truth| / max(1, |truth|):", np.max(np.abs(ll[fin] - c["loglik_truth"][fin]) / den))


@pytest.mark.parametrize("name", MG.CASE_NAMES)
def test_host_gradient_matches_truth_differences(harness, cases, tmp_path, name):
    c = cases[name]
    ll, g = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], c["T_use"])
    check_case(c, ll, g)


@pytest.mark.parametrize("name", ML.CASE_NAMES)
def test_host_gradient_matches_truth_differences_at_estimation_length(harness, tmp_path, name):
    """The same rule on tvl_grad_long_cases.npz (make_tvl_grad_long.py): T = 200 and 600, windows over a NaN column
    late in the panel."""
    c = ML.load_cases()[name]
    print(f"case {name}: compared {int(c['compared'].sum())}/{c['compared'].size}")
    ll, g = run_host(harness, tmp_path, c["Y"], c["maturities"], c["Theta"], c["T_use"])
    check_case(c, ll, g)


def test_host_chain_rule(harness, cases, tmp_path):
    """grad(space 0, θ) = grad(space 1, θ_c) · dθ_c/dθ: θ_c for the exp entries, (1 − θ_c²)/2 for the Φ diagonal."""
    from yfm_amd import KIND_TVL
    from yfm_amd.params import transform_params
    c = cases["C"]
    Th = c["Theta"]
    Tc = np.stack([transform_params(KIND_TVL, Th[:, b]) for b in range(Th.shape[1])], axis=1)
    _, g0 = run_host(harness, tmp_path, c["Y"], c["maturities"], Th, c["T_use"], 0)
    _, g1 = run_host(harness, tmp_path, c["Y"], c["maturities"], Tc, c["T_use"], 1)
    f = np.ones_like(Tc)
    for i in POS:
        f[i] = Tc[i]
    for i in R11:
        f[i] = (1.0 - Tc[i] ** 2) / 2.0
    assert np.all(np.abs(g0 - g1 * f).max(axis=0) <= REL * np.abs(g0).max(axis=0))
