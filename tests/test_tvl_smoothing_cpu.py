"""The NumPy half of the TVλ smoother's host mirror (yfm_amd.smoothing) on the checker's arrays: λ̂_t and its delta-method
standard deviation, the fitted curves Z(λ̂_t)[:, 1:3]·β̂_t[1:3] against an explicit loop over the oracle's loadings, and
em_moments at M = 4 against the explicit sums."""
import numpy as np
import pytest

import tvl_smooth_fixture as TF
import tvl_smoother_reference as TR
from yfm_amd import smoothing
from yfm_amd.models import create_model


def model_for(c):
    return create_model("TVλ", c["maturities"], len(c["maturities"]), 3)[0]


def device_like(c, n, b=0):
    """One candidate's arrays as the device returns them: T slots, NaN past the window."""
    w = c["windows"][n]
    T = c["Y"].shape[1]
    bs, Vs, Cs = np.full((4, T), np.nan), np.full((4, 4, T), np.nan), np.full((4, 4, T - 1), np.nan)
    bs[:, :n], Vs[:, :, :n], Cs[:, :, :n - 1] = w["beta_chk"][..., b], w["V_chk"][..., b], w["C_chk"][..., b]
    return bs, Vs, Cs


def test_lambda_path_and_its_standard_deviation():
    c = TF.cases()["T-n30"]
    bs, Vs, _ = device_like(c, 64)
    lam, sd = smoothing.lambda_path(bs, Vs)
    assert lam.shape == sd.shape == (70,)
    for t in range(64):
        assert lam[t] == pytest.approx(0.01 + np.exp(bs[3, t]), rel=1e-15)
        assert sd[t] == pytest.approx((lam[t] - 0.01) * np.sqrt(Vs[3, 3, t]), rel=1e-14)
    assert np.all(lam[:64] > 0.01) and np.all(sd[:64] > 0)
    assert np.isnan(lam[64:]).all() and np.isnan(sd[64:]).all()
    # batched arrays keep the batch axis
    w = c["windows"][70]
    lam2, sd2 = smoothing.lambda_path(w["beta_chk"], w["V_chk"])
    assert lam2.shape == sd2.shape == (70, 2)
    np.testing.assert_array_equal(lam2[:, 0], smoothing.lambda_path(w["beta_chk"][..., 0], w["V_chk"][..., 0])[0])


@pytest.mark.parametrize("name,n", (("T-E", 8), ("T-n30", 65)))
def test_smoothed_yields_use_the_smoothed_lambda(name, n):
    c = TF.cases()[name]
    bs = device_like(c, n)[0]
    got = smoothing.tvl_smoothed_yields(model_for(c), bs)
    ref = TR.smoothed_yields_ref(c["maturities"], bs)
    assert got.shape == c["Y"].shape
    np.testing.assert_allclose(got[:, :n], ref[:, :n], rtol=1e-13, atol=0)
    assert np.isnan(got[:, n:]).all()


def test_smoothed_yields_refuse_the_fixed_loading_models():
    dns = create_model("1C", np.array([3.0, 12.0, 60.0]), 3, 3)[0]
    with pytest.raises(NotImplementedError, match="smooth_batch"):
        smoothing.tvl_smoothed_yields(dns, np.zeros((4, 2)))
    with pytest.raises(NotImplementedError, match="smooth_batch"):
        smoothing.tvl_smooth_batch(dns, None, None)


@pytest.mark.parametrize("name,n", (("T-E", 8), ("T-n30", 3), ("T-n30", 70)))
def test_em_moments_at_four_states(name, n):
    c = TF.cases()[name]
    bs, Vs, Cs = device_like(c, n)
    got = smoothing.em_moments(bs, Vs, Cs, n)
    S00, S11, S10 = TR.em_moments_ref(bs[:, :n], Vs[:, :, :n], Cs[:, :, :n - 1])
    for key, ref in (("S00", S00), ("S11", S11), ("S10", S10)):
        assert got[key].shape == (4, 4) and np.isfinite(got[key]).all()
        np.testing.assert_allclose(got[key], ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    np.testing.assert_array_equal(got["S00"], got["S00"].T)
