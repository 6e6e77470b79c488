"""The NumPy half of yfm_amd.smoothing against the checker's arrays (tests/smoother_reference.py), and the fixture's own
consistency: smoothed_yields is Zβ̂_t with the oracle's loadings, em_moments the explicit sums over the window, and
the stored truth is within 1e-10 of the stored checker for every ordinary candidate."""
import numpy as np
import pytest

import smooth_fixture as SF
import smoother_reference as SR
from yfm_amd import smoothing
from yfm_amd.models import create_model


def model_for(c):
    dns = c["kind"] == 0
    return create_model("1C" if dns else "GNS5", c["maturities"], len(c["maturities"]), 3 if dns else 5)[0]


@pytest.mark.parametrize("name", ("S-E", "G-E"))
def test_smoothed_yields_are_Z_beta(name):
    c = SF.cases()[name]
    n = c["Y"].shape[1]
    bs = c["windows"][n]["beta_chk"][..., 0]
    got = smoothing.smoothed_yields(model_for(c), c["Theta_c"][:, 0], bs)
    ref = SR.smoothed_yields_ref(c["kind"], c["maturities"], c["Theta_c"][:, 0], bs, space=1)
    assert got.shape == c["Y"].shape
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name,n", (("S-E", 8), ("S-n30", 3), ("S-n30", 70), ("G-E", 12)))
def test_em_moments_are_the_window_sums(name, n):
    c = SF.cases()[name]
    w = c["windows"][n]
    T = c["Y"].shape[1]
    M = w["beta_chk"].shape[0]
    # the arrays as the device returns them: T slots, NaN past the window
    bs = np.full((M, T), np.nan)
    Vs = np.full((M, M, T), np.nan)
    Cs = np.full((M, M, T - 1), np.nan)
    bs[:, :n], Vs[:, :, :n], Cs[:, :, :n - 1] = w["beta_chk"][..., 0], w["V_chk"][..., 0], w["C_chk"][..., 0]
    got = smoothing.em_moments(bs, Vs, Cs, n)
    S00, S11, S10 = SR.em_moments_ref(bs[:, :n], Vs[:, :, :n], Cs[:, :, :n - 1])
    for key, ref in (("S00", S00), ("S11", S11), ("S10", S10)):
        assert got[key].shape == (M, M) and np.isfinite(got[key]).all()
        np.testing.assert_allclose(got[key], ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    np.testing.assert_array_equal(got["S00"], got["S00"].T)


def test_em_moments_of_a_one_column_window_are_zero():
    c = SF.cases()["S-n30"]
    w = c["windows"][1]
    got = smoothing.em_moments(w["beta_chk"][..., 0], w["V_chk"][..., 0], w["C_chk"][..., 0], 1)
    for key in ("S00", "S11", "S10"):
        assert np.array_equal(got[key], np.zeros((3, 3)))


def test_fixture_is_small_and_consistent():
    assert SF.MS.FILE.stat().st_size < 256 * 1024
    cs = SF.cases()
    assert set(cs) == set(SF.CASES)
    assert sorted(cs["S-n30"]["windows"]) == sorted(SF.MS.WINDOWS_N30)
    assert cs["S-n30"]["unit_root"] >= 0
    Y = cs["S-nan"]["Y"]
    nan_cols = np.isnan(Y).any(axis=0).nonzero()[0].tolist()
    assert nan_cols == [0, 4, 8, Y.shape[1] - 1] and np.isnan(Y[:, 8]).sum() == 1
    for name, c in cs.items():
        for n, w in c["windows"].items():
            for b in range(c["Theta"].shape[1]):
                if b == c["unit_root"]:
                    continue
                for what in ("beta", "V", "C"):
                    e = SR.traj_err(w[what + "_chk"][..., b], w[what + "_tru"][..., b], w[what + "_tru"][..., b])
                    assert e <= 1e-10, (name, n, b, what, e)


def test_near_unit_root_candidate_has_the_eigenvalue():
    c = SF.cases()["S-n30"]
    Phi = SR.model_fp64(c["kind"], c["maturities"], c["Theta"][:, c["unit_root"]])[4]
    assert np.abs(np.linalg.eigvals(Phi) - 0.999).min() < 1e-12
