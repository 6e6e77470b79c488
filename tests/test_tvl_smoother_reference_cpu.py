"""The TVλ smoother's three checkers against each other (tests/tvl_smoother_reference.py) on an N = 3, T = 5 case with a
missing column: the dense FP64 EKF with the RTS pass (a), the same in 40-digit mpmath (b) and the joint Gaussian
conditional of the linearised time-varying model (c), which uses no backward recursion at all.  This pins the definitions
of include/yfm.h yfm_tvl_smooth_batch, C_t's index convention included.  The committed fixture regenerates: its smallest
case is rebuilt from the generator and compared with the stored arrays."""
import multiprocessing as mproc

import numpy as np
import pytest

import tvl_smooth_fixture as TF
import tvl_smoother_reference as TR
from yfm_amd import KIND_TVL
from yfm_amd import synthetic as S


@pytest.fixture(scope="module")
def case():
    m = np.array([6.0, 24.0, 120.0])
    Y = S.simulate_panel(KIND_TVL, 5, m, 77).copy()
    Y[1, 2] = np.nan  # one NaN entry makes column 3 a missing column
    Th = S.theta_batch(KIND_TVL, 2, 0.02, 78, bad_frac=0)
    return m, Y, Th


@pytest.mark.parametrize("b", (0, 1))
def test_dense_mp_and_joint_agree(case, b):
    m, Y, Th = case
    d = TR.smooth_dense(m, Y, Th[:, b])
    t = TR.smooth_mp(m, Y, Th[:, b])
    j = TR.smooth_joint(m, Y, Th[:, b])
    for what, xd, xt, xj in zip(("beta", "V", "C"), d, t, j):
        assert xd.shape == xt.shape == xj.shape
        e_dt, e_jt = TR.traj_err(xd, xt, xt), TR.traj_err(xj, xt, xt)
        print(what, "dense vs mp", e_dt, "joint vs mp", e_jt)
        assert e_dt <= 1e-10 and e_jt <= 1e-9, (what, e_dt, e_jt)
    assert d[0].shape == (4, 5) and d[1].shape == (4, 4, 5) and d[2].shape == (4, 4, 4)


def test_lag_one_index_convention(case):
    """C[:, :, t − 1] is Cov(β_{t+1}, β_t | y): the block below the diagonal of the joint conditional covariance."""
    m, Y, Th = case
    C = TR.smooth_dense(m, Y, Th[:, 0])[2]
    Cj = TR.smooth_joint(m, Y, Th[:, 0])[2]
    Ct = np.transpose(C, (1, 0, 2))
    assert TR.traj_err(C, Cj, Cj) <= 1e-9
    assert TR.traj_err(Ct, Cj, Cj) > 1e-3


def test_windows_and_space(case):
    """A window of n columns is the panel cut to n columns; n = 1 has one update and no C; the constrained space takes
    the transformed θ; smooth_mp_windows is smooth_mp per window."""
    from yfm_amd.params import transform_params
    m, Y, Th = case
    for n in (1, 3):
        a = TR.smooth_dense(m, Y, Th[:, 0], n=n)
        c = TR.smooth_dense(m, Y[:, :n], Th[:, 0])
        for x, y in zip(a, c):
            np.testing.assert_array_equal(x, y)
        assert a[2].shape == (4, 4, n - 1)
    a = TR.smooth_dense(m, Y, Th[:, 0])
    c = TR.smooth_dense(m, Y, transform_params(KIND_TVL, Th[:, 0]), space=1)
    for x, y in zip(a, c):
        assert TR.traj_err(x, y, y) <= 1e-10
    w = TR.smooth_mp_windows(m, Y, Th[:, 0], 0, (2, 5))
    for got, n in zip(w, (2, 5)):
        for x, y in zip(got, TR.smooth_mp(m, Y, Th[:, 0], 0, n)):
            np.testing.assert_array_equal(x, y)


def test_linearisation_is_at_the_predicted_state(case):
    """Z_t of the forward pass is the oracle's loadings at a_t with the Jacobian column of filter.jl:43-46 as written:
    the step the oracle's own filter_step_tvl takes from (a_t, P_t) lands on the forward pass's a_{t+1}, P_{t+1}."""
    from oracle import kalman_oracle as O
    m, Y, Th = case
    f = TR.forward_dense(m, Y, Th[:, 0])
    s = TR.model_fp64(m, Th[:, 0])
    for t in (0, 1, 3):
        s.beta, s.P = f["ap"][t].copy(), f["Pp"][t].copy()
        assert O.filter_step_tvl(s, Y[:, t])
        np.testing.assert_allclose(s.beta, f["ap"][t + 1], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(s.P, f["Pp"][t + 1], rtol=1e-8, atol=1e-12)


def test_fixture_regenerates():
    """The generator's smallest case, rebuilt, equals the stored arrays bit for bit; the file is small; the stored truth
    is within 1e-10 of the stored checker for every ordinary candidate."""
    MT = TF.MT
    assert MT.FILE.stat().st_size < 512 * 1024
    with mproc.Pool(4) as pool:
        fresh = MT.make_case(pool, "T-E")
    with np.load(MT.FILE, allow_pickle=False) as z:
        for k, v in fresh.items():
            np.testing.assert_array_equal(z["T-E/" + k], v, err_msg=k)
    cs = TF.cases()
    assert set(cs) == set(TF.CASES)
    assert sorted(cs["T-n30"]["windows"]) == sorted(MT.WINDOWS_N30) and cs["T-n30"]["unit_root"] == 1
    Y = cs["T-nan"]["Y"]
    nan_cols = np.isnan(Y).any(axis=0).nonzero()[0].tolist()
    assert nan_cols == [0, 4, 8, Y.shape[1] - 1] and np.isnan(Y[:, 8]).sum() == 1
    for name, c in cs.items():
        assert c["Y"].shape == MT.SHAPES[name][:2]
        for n, w in c["windows"].items():
            for b in range(c["Theta"].shape[1]):
                if b == c["unit_root"]:
                    continue
                for what in ("beta", "V", "C"):
                    e = TR.traj_err(w[what + "_chk"][..., b], w[what + "_tru"][..., b], w[what + "_tru"][..., b])
                    assert e <= 1e-10, (name, n, b, what, e)
    Phi = TR.model_fp64(cs["T-n30"]["maturities"], cs["T-n30"]["Theta"][:, 1]).Phi
    assert np.abs(np.linalg.eigvals(Phi) - 0.999).min() < 1e-12
