"""CPU test of the λ models' algebra (csrc/yfm_msed.hpp): the functions the gfx950 kernel runs — loadings and their
γ-derivative, the 3×3 Cholesky with the ridge retry, the score, the EWMA, one step — compiled for the host
(tests/msed_host_check.cpp, -ffp-contract=off, -fsanitize=address,undefined, a stand-alone program) and run as
one full filter per kind on N = 4, T = 8 against the values the Float64 restatement (tests/msed_reference.py)
wrote to tests/golden/msed/, at 1e-12 relative; −Inf must agree exactly."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from host_check_io import build_host_check, run_loss_host as run_host

sys.path.insert(0, str(GOLDEN / "msed"))
import make_msed as MM  # noqa: E402

REL = 1e-12
KINDS = (3, 4, 5, 6, 8)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "msed_host_check", sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return MM.load_cases()


def check(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (got, want)
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print("max rel", rel.max() if rel.size else 0.0)
    assert np.all(rel <= REL), rel


@pytest.mark.parametrize("kind", KINDS)
def test_host_filter_matches_restatement(harness, cases, tmp_path, kind):
    """Windows of 5 and 8 columns on a panel whose column 6 misses its first maturity: the short window is finite,
    the long ones −Inf; both parameter spaces."""
    c = cases
    got = run_host(harness, tmp_path, kind, c["Y"], c["maturities"], c[f"theta_{kind}"], c[f"T_use_{kind}"], 0)
    check(got, c[f"loss_{kind}"])
    assert np.isfinite(got[0]) and np.isneginf(got[1])
    got_c = run_host(harness, tmp_path, kind, c["Y"], c["maturities"], c[f"theta_c_{kind}"], c[f"T_use_{kind}"], 1)
    check(got_c, c[f"loss_c_{kind}"])


@pytest.mark.parametrize("kind", KINDS)
def test_host_filter_full_panel(harness, cases, tmp_path, kind):
    """The same candidates on the panel without the missing entry: three finite values per kind."""
    from yfm_amd import synthetic as S
    c = cases
    Y = S.simulate_panel(kind, 8, maturities=c["maturities"], seed=7)
    got = run_host(harness, tmp_path, kind, Y, c["maturities"], c[f"theta_{kind}"], [8, 8, 8], 0)
    assert np.all(np.isfinite(got))
    check(got, c[f"loss_full_{kind}"])


def test_host_ridge_branch(harness, cases, tmp_path):
    """NS with γ = 800: λ = Inf, Z₂ = Z₃ = 0 exactly, the second pivot is exactly zero, the ridge retry runs and
    the loss is finite and the restatement's."""
    import msed_reference as R
    c = cases
    Y = c["Y"].copy()
    Y[0, 5] = 4.0
    th = c["theta_c_3"][:, :1].copy()
    th[0, 0] = 800.0
    got = run_host(harness, tmp_path, 3, Y, c["maturities"], th, [8], 1)
    want = np.array([R.get_loss(3, c["maturities"], Y, th[:, 0], 1, R.FLOAT)])
    assert np.isfinite(want[0])
    check(got, want)


@pytest.mark.parametrize("kind", [6, 8])
def test_host_scaled_score_at_square_loadings(harness, tmp_path, kind):
    """N = 3: OLS interpolates and the exact score is 0, so γ never moves (the 40-digit truth), while a Float64
    score is rounding noise that the scaled update turns into steps of ±A — the restatement ends 1e-3 from the
    truth.  The scaled kinds' refined score (residual with its errors carried, one correction of β) keeps the host
    build of the kernel's algebra within 1e-9 of the truth."""
    import msed_reference as R
    from yfm_amd import synthetic as S
    mats = np.array([3.0, 12.0, 60.0])
    Y = S.simulate_panel(kind, 8, maturities=mats)
    Th = S.theta_batch(kind, 6, scale=0.1, seed=500 + kind, bad_frac=0.0)
    got = run_host(harness, tmp_path, kind, Y, mats, Th, [8] * 6, 0)
    truth = np.array([R.get_loss(kind, mats, Y, Th[:, b], 0, R.TRUTH) for b in range(6)])
    ref = np.array([R.get_loss(kind, mats, Y, Th[:, b], 0, R.FLOAT) for b in range(6)])
    print("host vs truth", np.max(np.abs(got - truth) / np.abs(truth)), "float64 restatement vs truth",
          np.max(np.abs(ref - truth) / np.abs(truth)))
    assert np.all(np.abs(got - truth) <= 1e-9 * np.abs(truth))

