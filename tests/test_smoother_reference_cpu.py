"""The smoother's three checkers against each other (tests/smoother_reference.py) on a 3-state, N = 2, T = 5 case with a
missing column: the dense FP64 RTS smoother (a), the same in 40-digit mpmath (b) and the joint Gaussian conditional
formed from the stacked covariance of (β_1 … β_5, y_obs) (c), which uses no recursion at all.  This pins the
definitions of include/yfm.h yfm_smooth_batch, C_t's index convention included: slot t − 1 holds Cov(β_{t+1}, β_t | y),
not its transpose."""
import numpy as np
import pytest

import smoother_reference as SR
from yfm_amd import KIND_DNS
from yfm_amd import synthetic as S


@pytest.fixture(scope="module")
def case():
    m = np.array([6.0, 60.0])
    Y = S.simulate_panel(KIND_DNS, 5, m, 77).copy()
    Y[1, 2] = np.nan  # one NaN entry makes column 3 a missing column
    Th = S.theta_batch(KIND_DNS, 2, 0.02, 78, bad_frac=0)
    return m, Y, Th


@pytest.mark.parametrize("b", (0, 1))
def test_dense_mp_and_joint_agree(case, b):
    m, Y, Th = case
    d = SR.smooth_dense(KIND_DNS, m, Y, Th[:, b])
    t = SR.smooth_mp(KIND_DNS, m, Y, Th[:, b])
    j = SR.smooth_joint(KIND_DNS, m, Y, Th[:, b])
    for what, xd, xt, xj in zip(("beta", "V", "C"), d, t, j):
        assert xd.shape == xt.shape == xj.shape
        e_dt, e_jt = SR.traj_err(xd, xt, xt), SR.traj_err(xj, xt, xt)
        print(what, "dense vs mp", e_dt, "joint vs mp", e_jt)
        assert e_dt <= 1e-12 and e_jt <= 1e-11, (what, e_dt, e_jt)
    assert d[0].shape == (3, 5) and d[1].shape == (3, 3, 5) and d[2].shape == (3, 3, 4)


def test_lag_one_index_convention(case):
    """C[:, :, t − 1] is Cov(β_{t+1}, β_t | y): the block below the diagonal of the joint conditional covariance.  The
    transposed convention is far outside the agreement above (C_t is not symmetric)."""
    m, Y, Th = case
    C = SR.smooth_dense(KIND_DNS, m, Y, Th[:, 0])[2]
    Cj = SR.smooth_joint(KIND_DNS, m, Y, Th[:, 0])[2]
    Ct = np.transpose(C, (1, 0, 2))
    assert SR.traj_err(C, Cj, Cj) <= 1e-11
    assert SR.traj_err(Ct, Cj, Cj) > 1e-3


def test_windows_and_space(case):
    """A window of n columns is the panel cut to n columns; n = 1 has one update and no C; the constrained space takes
    the transformed θ."""
    from yfm_amd.params import transform_params
    m, Y, Th = case
    for n in (1, 3):
        a = SR.smooth_dense(KIND_DNS, m, Y, Th[:, 0], n=n)
        c = SR.smooth_dense(KIND_DNS, m, Y[:, :n], Th[:, 0])
        for x, y in zip(a, c):
            np.testing.assert_array_equal(x, y)
        assert a[2].shape == (3, 3, n - 1)
    a = SR.smooth_dense(KIND_DNS, m, Y, Th[:, 0])
    c = SR.smooth_dense(KIND_DNS, m, Y, transform_params(KIND_DNS, Th[:, 0]), space=1)
    for x, y in zip(a, c):
        assert SR.traj_err(x, y, y) <= 1e-12
