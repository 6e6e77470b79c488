"""The shared checkers can fail: tests/grad_rule.py and the bit comparison of tests/gpu_scenarios.py on synthetic arrays
(no fixture, no compiler, no GPU)."""
from __future__ import annotations

import numpy as np
import pytest

from gpu_scenarios import assert_same_bits, same_bits
from grad_rule import REL, assert_candidate_rule, assert_gradient_rule, chain_factor
from yfm_amd import KIND_DNS, KIND_TVL
from yfm_amd.params import n_params, state_dim, transform_params

P, B = 4, 100


def case():
    """‖g_fd‖∞ = 4 for every candidate, row 2 exactly zero, everything compared; g = g_fd passes."""
    g_fd = np.tile(np.array([4.0, 1.0, 0.0, -2.0])[:, None], (1, B))
    return {"g_fd": g_fd, "e_fd": np.full(B, 1e-12), "compared": np.ones(B, dtype=bool),
            "T_use": np.full(B, 10), "loglik_truth": np.full(B, -3.0), "ref_err": np.full(B, 1.0)}


def test_rule_holds_at_the_bound_and_fails_one_ulp_above():
    c = case()
    bound = REL * 4.0 + c["e_fd"][7]
    g = c["g_fd"].copy()
    c["g_fd"][1, 7], g[1, 7] = bound, 0.0  # |g − g_fd| is the bound to the bit
    assert_gradient_rule(g, c)
    c["g_fd"][1, 7] = np.nextafter(bound, np.inf)
    assert abs(g[1, 7] - c["g_fd"][1, 7]) > bound
    with pytest.raises(AssertionError):
        assert_gradient_rule(g, c)


def test_rule_needs_three_quarters_compared():
    c = case()
    c["compared"][75:] = False
    assert_gradient_rule(c["g_fd"].copy(), c)
    c["compared"][74] = False
    with pytest.raises(AssertionError):
        assert_gradient_rule(c["g_fd"].copy(), c)


def test_rule_wants_exact_zeros():
    c = case()
    g = c["g_fd"].copy()
    g[2, 3] = 1e-300  # far inside the bound, but g_fd is 0.0 there
    with pytest.raises(AssertionError):
        assert_gradient_rule(g, c)
    c["compared"][3] = False
    assert_gradient_rule(g, c)


def test_rule_checks_the_selection_it_is_given():
    c = case()
    g = c["g_fd"].copy()
    g[0, 5] += 1.0
    c["compared"][5] = False  # not compared: not checked …
    assert_gradient_rule(g, c)
    with pytest.raises(AssertionError):  # … unless the selection says so
        assert_gradient_rule(g, c, sel=np.ones(B, dtype=bool))
    c["compared"][5] = True
    with pytest.raises(AssertionError):
        assert_gradient_rule(g, c)
    assert_gradient_rule(g, c, sel=np.arange(B) != 5)
    hard = np.arange(B) == 5
    assert_gradient_rule(g, c, second_clause=hard)  # err = 1 ≤ ref_err = 1
    c["ref_err"][5] = 0.5
    with pytest.raises(AssertionError):
        assert_gradient_rule(g, c, second_clause=hard)


def test_rule_extras_are_asserted_only_where_passed():
    c = case()
    c["T_use"][9], c["compared"][9] = 2, False
    g = c["g_fd"].copy()
    assert_gradient_rule(g, c)
    with pytest.raises(AssertionError):
        assert_gradient_rule(g, c, short_windows_zero=True)
    ll = c["loglik_truth"] * (1 + 2e-9)
    assert_gradient_rule(g, c, primal=ll, primal_asserted=False)
    assert_gradient_rule(g, c, primal=c["loglik_truth"] * (1 + 5e-10))
    with pytest.raises(AssertionError):
        assert_gradient_rule(g, c, primal=ll)
    ll = c["loglik_truth"].copy()
    ll[9] = 0.0
    assert_gradient_rule(g, c, primal=ll, primal_mask=c["compared"])


def test_candidate_rule_wants_the_fixtures_nan_pattern():
    g_fd = np.array([[4.0, np.nan], [1.0, np.nan]])
    e_fd = np.array([1e-12, np.nan])
    loss = np.array([2.0, -np.inf])
    g = np.array([[4.0, np.nan], [1.0, np.nan], [9.0, np.nan]])  # a row past the fixture's leading ones
    assert assert_candidate_rule(g, g_fd, e_fd, loss) == 0.0
    bad = g.copy()
    bad[:, 1] = 0.5  # a finite gradient where the fixture has NaN
    with pytest.raises(AssertionError):
        assert_candidate_rule(bad, g_fd, e_fd, loss)
    bad = g.copy()
    bad[2, 0] = np.nan  # NaN where the fixture is finite
    with pytest.raises(AssertionError):
        assert_candidate_rule(bad, g_fd, e_fd, loss)
    with pytest.raises(AssertionError):
        assert_candidate_rule(g, g_fd, e_fd, np.array([2.0, 2.0]))
    bad = g.copy()
    bad[1, 0] += 1e-8
    with pytest.raises(AssertionError):
        assert_candidate_rule(bad, g_fd, e_fd, loss)


@pytest.mark.parametrize("kind", [KIND_DNS, KIND_TVL])
def test_chain_factor_is_the_transforms_derivative(kind):
    """The index tables against central differences of transform_params at a random θ: its Jacobian is diagonal and
    the diagonal is chain_factor."""
    n = n_params(kind)
    th = np.random.default_rng(kind).normal(scale=0.5, size=n)
    h = 1e-5
    J = np.empty((n, n))
    for i in range(n):
        up, dn = th.copy(), th.copy()
        up[i] += h
        dn[i] -= h
        J[:, i] = (transform_params(kind, up) - transform_params(kind, dn)) / (up[i] - dn[i])
    f = chain_factor(kind, transform_params(kind, th))
    assert np.all(np.abs(J - np.diag(f)) <= 1e-6 * np.abs(f).max())
    assert np.all(np.abs(np.diag(J) - f) <= 1e-6 * np.abs(f))


def test_bit_comparison():
    nan1 = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)
    nan2 = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    assert np.isnan(nan1).all() and np.isnan(nan2).all()
    assert same_bits(nan1, nan1.copy()) and not same_bits(nan1, nan2)
    assert same_bits([0.0, 1.5], [0.0, 1.5]) and not same_bits([0.0], [-0.0])
    assert not same_bits(np.zeros(2), np.zeros((2, 1)))
    for a, b in ((nan1, nan2), ([0.0], [-0.0])):
        assert_same_bits(a, b, nan_payloads=False)
        with pytest.raises(AssertionError):
            assert_same_bits(a, b)
    with pytest.raises(AssertionError):
        assert_same_bits([1.0], [2.0], nan_payloads=False)


# ---- tests/call_steps.py: the comparer of the call sequences, and the table's constructed flags -----------------------
def _result():
    nan = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
    out = {"ll": np.array([-3.5, nan, -np.inf, 0.0]), "grad": np.arange(8.0).reshape(2, 4)}
    cnt = {"flags": (1, 1), "deferred": 2, "unavailable": 3, "steady": 0}
    return out, cnt


def _copy(r):
    return {k: v.copy() for k, v in r[0].items()}, dict(r[1])


def test_sequence_comparer_accepts_equal_runs_and_fails_on_one_counter_one_bit_or_one_key():
    import call_steps as CS
    ref = _result()
    CS.assert_same_result(_copy(ref), ref)
    for key, value in (("flags", (1, 2)), ("flags", (0, 1)), ("deferred", 3), ("unavailable", 2), ("steady", 1)):
        got = _copy(ref)
        got[1][key] = value  # one flipped counter
        with pytest.raises(AssertionError):
            CS.assert_same_result(got, ref)
    got = _copy(ref)
    got[0]["grad"][1, 2] = np.nextafter(got[0]["grad"][1, 2], np.inf)  # one differing bit
    with pytest.raises(AssertionError):
        CS.assert_same_result(got, ref)
    got = _copy(ref)
    got[0]["ll"][1] = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]  # … in a NaN's payload
    with pytest.raises(AssertionError):
        CS.assert_same_result(got, ref)
    got = _copy(ref)
    got[0]["ll"][3] = -0.0
    with pytest.raises(AssertionError):
        CS.assert_same_result(got, ref)
    got = _copy(ref)
    del got[0]["grad"]  # a missing output
    with pytest.raises(AssertionError):
        CS.assert_same_result(got, ref)
    got = _copy(ref)
    got[0]["extra"] = np.zeros(1)
    with pytest.raises(AssertionError):
        CS.assert_same_result(got, ref)
    with pytest.raises(AssertionError):  # counters where the reference defines none
        CS.assert_same_result(_copy(ref), (ref[0], None))


def test_sequence_constructed_counters_can_fail():
    import call_steps as CS
    step = CS.Step("s", lambda: None, lambda e: {}, flags=(1, 1), deferred=2, unavailable=3, value="ll")
    ref = _result()
    CS.assert_constructed(step, ref)
    for key, value in (("flags", (1, 0)), ("deferred", 0), ("unavailable", 0), ("steady", 128)):
        got = _copy(ref)
        got[1][key] = value
        with pytest.raises(AssertionError):
            CS.assert_constructed(step, got)
    got = _copy(ref)
    got[0]["ll"][0] = -np.inf  # the values' own −Inf count no longer is the flag
    with pytest.raises(AssertionError):
        CS.assert_constructed(step, got)
    free = CS.Step("d", lambda: None, lambda e: {}, flags=(1, 1), deferred=2, unavailable=3, steady=None, value="ll")
    got = _copy(ref)
    got[1]["steady"] = 128  # not constructible: any number passes, the other counters still count
    CS.assert_constructed(free, got)
    got[1]["deferred"] = 0
    with pytest.raises(AssertionError):
        CS.assert_constructed(free, got)
    silent = CS.Step("r", lambda: None, lambda e: {}, flags=None)
    CS.assert_constructed(silent, ({}, None))
    with pytest.raises(AssertionError):
        CS.assert_constructed(silent, ref)


def test_sequence_table_flags_are_the_c_oracles_counts():
    """Every Kalman-kind batch of the table, the dirtier and the victim: the NaN and −Inf counts the table constructs
    are those of the dense FP64 restatement of the reference (oracle/yfm_oracle.c), and the steps' names, the pair
    representatives and the batch sizes are what the sequences assume."""
    import call_steps as CS
    from oracle import kalman_oracle as O
    from oracle.truth import loglik_oracle
    table = CS.build_table()
    assert set(CS.PAIR_STEPS) <= set(table) and len(CS.PAIR_STEPS) == 13
    shapes = {table[n].panel()[0].shape for n in CS.PAIR_STEPS}
    assert {s[0] for s in shapes} >= {4, 30, 64, 65, 67} and {s[1] for s in shapes} >= {8, 12, 16, 40}
    steps = list(table.values()) + [CS.dirtier(), CS.victim()]
    checked = 0
    for s in steps:
        if s.batch is None:
            continue
        Y, mats = s.panel()
        Th = s.batch()
        assert Th.shape[1] <= 16 or s.name == "D", s.name
        ll = loglik_oracle(s.kind, Y, mats, Th, space=s.space)
        if s.name.endswith("loss_array"):  # its −Inf count is of its own rows, which σ² = 0 leaves finite
            Tc = Th if s.space == 1 else transform_params(s.kind, Th)
            for b in np.flatnonzero(~np.isnan(ll)):
                st = O.KalmanState.fresh(s.kind, mats, state_dim(s.kind))
                O.set_params(st, Tc[:, b])
                assert np.isfinite(O.get_loss_array(st, Y)).all(), (s.name, b)
            assert tuple(s.flags) == (int(np.isnan(ll).sum()), 0), s.name
            checked += 1
            continue
        assert (int(np.isnan(ll).sum()), int(np.isneginf(ll).sum())) == tuple(s.flags), (s.name, ll)
        assert len({Th[:, b].tobytes() for b in range(Th.shape[1])}) == Th.shape[1], s.name  # no two candidates equal
        checked += 1
    assert checked >= 30
