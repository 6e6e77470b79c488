"""CPU test of the neural models' algebra (csrc/yfm_msedn.hpp): the functions the gfx950 kernel runs — decode with
the duplicator, the networks and transforms with their group-wide scalars, the back-propagated score, the EWMA, one
step — compiled for the host (tests/msedn_host_check.cpp, -ffp-contract=off, -fsanitize=address,undefined, a
stand-alone program) and run as full filters against the losses the Float64 restatement (tests/msedn_reference.py)
wrote to tests/golden/msedn/, at 1e-12 relative — the λ host check's bar.

Cases: 2 static and 8 score-driven switch combinations (random walk × scaled × anchored, the duplicator form
cycling scalar / block_diag / diag) × N ∈ {4, 5, 30, 33} × a panel with a NaN column mid-window and one whose
first column is NaN × both parameter spaces, three candidates each (T = 10)."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from host_check_io import build_host_check, run_loss_host as run_host

sys.path.insert(0, str(GOLDEN / "msedn"))
import make_msedn as MM  # noqa: E402
from yfm_amd import params as P  # noqa: E402

REL = 1e-12


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_host_check(tmp_path_factory, "msedn_host_check", sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return MM.load_cases()


def test_the_cases_cover_every_switch():
    kinds = MM.HOST_KINDS
    assert len(kinds) == 10 and sum(P.neural_is_static(k) for k in kinds) == 2
    sd = [k for k in kinds if not P.neural_is_static(k)]
    assert {(P.neural_has_b(k), P.neural_scaled(k), P.neural_anchored(k)) for k in sd} == {
        (a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    assert {k & 3 for k in sd} == {0, 1, 2}


@pytest.mark.parametrize("N", MM.HOST_N)
@pytest.mark.parametrize("kind", MM.HOST_KINDS)
def test_host_filter_matches_restatement(harness, cases, tmp_path, kind, N):
    mats = MM.mats_for(N)
    Th = MM.host_theta(kind)
    worst = 0.0
    for which, Y in enumerate(MM.host_panels(N)):
        for space in (0, 1):
            th = Th if space == 0 else P.transform_params(kind, Th)
            got = run_host(harness, tmp_path, kind, Y, mats, th, [MM.HOST_T] * 3, space)
            want = cases[f"host_{kind}_{N}_{which}_{space}"]
            # a NaN column inside the window is compared (−Inf); a NaN first column only makes step 1 prediction-only
            assert np.all(np.isneginf(want)) if which == 0 else np.all(np.isfinite(want))
            assert np.array_equal(np.isneginf(got), np.isneginf(want)) and not np.isnan(got).any(), (got, want)
            fin = np.isfinite(want)
            if fin.any():
                rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
                worst = max(worst, float(rel.max()))
                assert np.all(rel <= REL), (which, space, got, want)
    print("kind", kind, "N", N, "worst rel", worst)


@pytest.mark.parametrize("kind", MM.HOST_KINDS)
def test_host_window_before_the_nan_column(harness, tmp_path, kind):
    """The mid-panel NaN column (column 5) is not reached by a window of 4 columns: finite, and the restatement's."""
    import msedn_reference as R
    N = 5
    mats, Y = MM.mats_for(N), MM.host_panels(N)[0]
    Th = MM.host_theta(kind)
    got = run_host(harness, tmp_path, kind, Y, mats, Th, [4, 4, 1], 0)
    want = np.array([R.get_loss(kind, mats, Y, Th[:, b], 0, R.FLOAT, tu) for b, tu in enumerate((4, 4, 1))])
    assert np.all(np.isfinite(want)) and want[2] == 0.0 and got[2] == 0.0
    assert np.all(np.abs(got[:2] - want[:2]) <= REL * np.abs(want[:2])), (got, want)
