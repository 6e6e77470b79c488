"""The committed fixture tests/golden/info/info_cases.npz is what make_info.py describes: the shapes of the issue's
cases, every stored candidate compared (finite truth, e_fd ≤ 1e-9 of the largest entry), a positive plain-FP64
reference error per Hessian candidate, and score truths that telescope to the whole window's difference gradient."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN / "info"))
import make_info as MI  # noqa: E402

REL = 1e-9
SHAPES = {"H-E": (4, 8, 2), "H-nan": (6, 12, 2), "S-E": (4, 8, 2), "S-nan": (30, 40, 3), "S-n64": (64, 12, 2)}


@pytest.fixture(scope="module")
def cases():
    return MI.load_cases()


def test_file_is_small_and_complete(cases):
    assert MI.FILE.stat().st_size < 256 * 1024
    assert set(cases) == set(MI.HESS_CASES) | set(MI.SCORE_CASES) == set(SHAPES)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_and_inputs(cases, name):
    c = cases[name]
    N, T, B = SHAPES[name]
    assert c["Y"].shape == (N, T) and c["maturities"].shape == (N,) and c["Theta"].shape == (20, B)
    Y, m, pool, keep = MI.case_inputs(name)
    np.testing.assert_array_equal(c["Y"], Y)
    np.testing.assert_array_equal(c["maturities"], m)
    assert keep == B and all(any(np.array_equal(c["Theta"][:, b], pool[:, k]) for k in range(pool.shape[1]))
                             for b in range(B))
    assert np.isfinite(c["loglik_truth"]).all() and int(c["replaced"]) >= 0
    nan_cols = np.flatnonzero(np.isnan(c["Y"]).all(axis=0)).tolist()
    nan_any = np.flatnonzero(np.isnan(c["Y"]).any(axis=0)).tolist()
    if name == "H-nan":
        assert nan_cols == [5] and nan_any == [5, 9]
    elif name == "S-nan":
        assert nan_cols == [6] and nan_any == [5, 6, 20, 39]
    else:
        assert nan_any == []


@pytest.mark.parametrize("name", MI.HESS_CASES)
def test_every_hessian_candidate_is_compared(cases, name):
    c = cases[name]
    H = c["H_truth"]
    B = c["Theta"].shape[1]
    assert H.shape == (20, 20, B) and np.isfinite(H).all()
    np.testing.assert_array_equal(H, H.transpose(1, 0, 2))
    scale = np.abs(H).max(axis=(0, 1))
    assert np.all(c["e_fd"] <= REL * scale) and np.all(c["e_fd"] >= 0)
    assert c["ref_err"].shape == (B,) and np.all(c["ref_err"] > 0) and np.isfinite(c["ref_err"]).all()
    assert all(s in MI.REF_STEPS for s in c["ref_step"])
    # the plain FP64 reference is a usable Hessian, just a coarser one
    assert np.all(c["ref_err"] <= 1e-3 * scale)


@pytest.mark.parametrize("name", MI.SCORE_CASES)
def test_every_score_candidate_is_compared_and_telescopes(cases, name):
    c = cases[name]
    N, T, B = SHAPES[name]
    s = c["s_truth"]
    assert s.shape == (20, T - 1, B) and np.isfinite(s).all() and np.all(s[:, 0, :] == 0.0)
    gn = np.abs(c["g_fd"]).max(axis=0)
    assert np.all(c["e_fd"] <= REL * gn) and np.all(gn > 0)
    # Σ_k s_k = g_fd(T) − g_fd(2) = g_fd(T): a telescoping sum of float64 differences
    gap = np.abs(s.sum(axis=1) - c["g_fd"])
    assert np.all(gap <= 4 * T * 2.0 ** -53 * np.abs(s).sum(axis=1) + 1e-300)
