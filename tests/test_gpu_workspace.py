"""The context's own launch workspace across an estimation (yfm_capi.hip: launch; yfm_estimate.hip).

A context embeds one workspace (counter banks, scratch, deferral list); yfm_estimate with R >= 32 chains runs
two chain groups side by side, group 0 on that workspace through its own stream and group 1 on an extra one.
The batches before and after such an estimation go through the same workspace on the context's stream, so
their counters (yfm_last_batch_flags) must be their own and their logliks those of a context that never ran
an estimation.

Batches: 300 candidates of synthetic.theta_batch(bad_frac=0.1), whose non-stationary columns give −Inf.  No
seed of theta_batch gives a NaN lane (initialize_filter throws only for an exactly singular I − Φ, which a
random draw never is; the CPU oracle counts 0 NaN for seeds 71..76), so three columns get the unconstrained
Φ diagonal 40, which decodes to exactly Φ = I (as tests/test_gpu_estimate.py does).  With oracle/kalman_oracle.py
the two batches then hold 3 NaN and 18 / 20 −Inf lanes, so both counts compare non-zero numbers."""
from __future__ import annotations

import numpy as np
import pytest

from yfm_amd import KIND_DNS
from yfm_amd import synthetic as S
from yfm_amd.params import param_layout

pytestmark = pytest.mark.gpu

SEEDS = (71, 72)
NAN_COLS = (5, 150, 299)


def make_panel():
    mats = S.maturities_30()[:8].copy()
    return S.simulate_panel(KIND_DNS, 40, maturities=mats), mats


def make_batch(seed):
    Th = S.theta_batch(KIND_DNS, 300, seed=seed, bad_frac=0.1)
    lay = param_layout(KIND_DNS)
    for b in NAN_COLS:  # Φ = I exactly: initialize_filter throws, the lane is NaN
        Th[lay.phi_offset:lay.phi_offset + 9, b] = np.eye(3).reshape(-1) * 40.0
    return Th


def make_starts():
    return S.theta_batch(KIND_DNS, 32, seed=73, bad_frac=0.0, scale=0.05)


def check_flags(engine, ll):
    n_nan, n_neg = int(np.isnan(ll).sum()), int(np.isneginf(ll).sum())
    assert n_nan >= 1 and n_neg >= 1, (n_nan, n_neg)
    assert engine.last_flags() == (n_nan, n_neg)


def test_own_workspace_across_two_group_estimate(engine):
    from yfm_amd.engine import Engine

    Y, mats = make_panel()
    engine.set_panel(Y, mats)
    check_flags(engine, engine.loglik(KIND_DNS, make_batch(SEEDS[0])))
    # R = 32 is the smallest chain count with two groups: group 0 launches on the context's own workspace
    got = engine.estimate(KIND_DNS, make_starts(), space=0, iterations=3, max_group_iters=1)
    assert got["ll"].shape == (32,) and (got["status"] == 0).all()
    Th = make_batch(SEEDS[1])
    ll = engine.loglik(KIND_DNS, Th)
    check_flags(engine, ll)
    fresh = Engine(engine.device)
    try:
        fresh.set_panel(Y, mats)
        ref = fresh.loglik(KIND_DNS, Th)
    finally:
        fresh.close()
    np.testing.assert_array_equal(ll, ref)
