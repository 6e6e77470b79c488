"""GPU tests of yfm_nm_block (csrc/yfm_estimate.hip): one Optim.NelderMead run per chain on a block of coordinates,
all chains' trial points in one launch per round.

The λ kinds' loss is bitwise independent of the batch, so a chain must equal, bit for bit, the sequential restatement
of Optim's NelderMead (oracle/optim_nm.py) run on x ↦ −engine.loglik(kind, embed(x), T_use = w): the same objective
values give the same simplices.  For DNS, whose value is not batch-independent in general, the whole-θ block is held
against yfm_estimate's first group pass, which runs the same rounds."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import optim_nm as NM
from yfm_amd import params as P
from yfm_amd import synthetic as S

pytestmark = pytest.mark.gpu

MATS4 = np.array([3.0, 12.0, 60.0, 120.0])
WINDOWS = np.array([40, 24, 12], dtype=np.int32)


@pytest.mark.parametrize("kind", [P.KIND_SD_NS, P.KIND_NS])
def test_block_equals_sequential_nelder_mead(engine, kind):
    """N = 4, T = 40, three chains on windows 40, 24 and 12, the leading parameters as the block, 60 iterations."""
    Y = S.simulate_panel(kind, 40, maturities=MATS4, seed=7)
    engine.set_panel(Y, MATS4)
    n_lead = P.n_params(kind) - 12
    idx = np.arange(n_lead)
    p0 = S.theta_batch(kind, 3, scale=0.1, seed=11 + kind, bad_frac=0.0)
    X, f, n_evals = engine.nm_block(kind, p0, idx, T_use=WINDOWS, iterations=60, g_tol=1e-6)
    assert n_evals > 0
    np.testing.assert_array_equal(X[n_lead:], p0[n_lead:])  # the rest is held
    calls = 0
    for r in range(3):
        def objective(x, r=r):
            th = p0[:, r].copy()
            th[idx] = x
            return -float(engine.loglik(kind, th, space=0, T_use=[int(WINDOWS[r])])[0])
        want = NM.nelder_mead(objective, p0[idx, r], iterations=60, g_tol=1e-6)
        calls += want.f_calls
        np.testing.assert_array_equal(X[idx, r], want.x)
        assert f[r] == want.f
        assert f[r] == objective(X[idx, r])
        assert f[r] <= objective(p0[idx, r])
    print("n_evals", n_evals, "sequential f_calls", calls)


def test_block_of_a_scattered_index_set(engine):
    """A block that is neither leading nor contiguous (rows 1, 7, 4 in that order), SSD-NS: still the sequential run."""
    kind = P.KIND_SSD_NS
    Y = S.simulate_panel(kind, 40, maturities=MATS4, seed=7)
    engine.set_panel(Y, MATS4)
    idx = np.array([1, 7, 4])
    p0 = S.theta_batch(kind, 2, scale=0.1, seed=3, bad_frac=0.0)
    X, f, _ = engine.nm_block(kind, p0, idx, T_use=[40, 17], iterations=25)
    for r, w in enumerate((40, 17)):
        def objective(x, r=r, w=w):
            th = p0[:, r].copy()
            th[idx] = x
            return -float(engine.loglik(kind, th, space=0, T_use=[w])[0])
        want = NM.nelder_mead(objective, p0[idx, r], iterations=25, g_tol=1e-6)
        np.testing.assert_array_equal(X[idx, r], want.x)
        assert f[r] == want.f
    keep = np.setdiff1d(np.arange(15), idx)
    np.testing.assert_array_equal(X[keep], p0[keep])


def test_whole_theta_block_equals_estimate_first_pass(engine):
    """DNS with idx = every coordinate: the chain is yfm_estimate's first group pass (max_group_iters = 1) from the
    same start, which needs no sanitising or rescaling — same rounds, same batch slots, same bits."""
    kind = P.KIND_DNS
    mats = S.maturities_30()
    Y = S.simulate_panel(kind, 40, maturities=mats)
    engine.set_panel(Y, mats)
    p0 = S.theta_batch(kind, 3, scale=0.05, seed=5, bad_frac=0.0)
    est = engine.estimate(kind, p0, space=0, T_use=WINDOWS, iterations=60, g_tol=1e-6, max_group_iters=1)
    assert np.all(est["status"] == 0)
    # the start was used as it came (the library's own transform: a few ulp from NumPy's)
    np.testing.assert_allclose(est["init_c"], P.transform_params(kind, p0), rtol=1e-14)
    X, f, n_evals = engine.nm_block(kind, p0, np.arange(20), T_use=WINDOWS, iterations=60, g_tol=1e-6)
    np.testing.assert_array_equal(X, est["p"])
    np.testing.assert_array_equal(f, -est["ll"])
    assert n_evals == est["n_evals"] - 3  # the estimate also validated each start once


def test_bad_requests(engine):
    from yfm_amd import _lib
    kind = P.KIND_SD_NS
    engine.set_panel(S.simulate_panel(kind, 12, maturities=MATS4, seed=7), MATS4)
    p0 = S.theta_batch(kind, 1, scale=0.1, bad_frac=0.0)
    for idx in ([0, 0], [15], [-1], []):
        with pytest.raises(_lib.YFMError) as e:
            engine.nm_block(kind, p0, idx, iterations=5)
        assert e.value.code == -1, str(e.value)
