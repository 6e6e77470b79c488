"""What the estimation-length smoother tests share, on the CPU and the GPU, for the fixed-loading models ("fixed": DNS and
GNS5, tests/golden/smooth_long/smooth_long_cases.npz) and TVλ ("tvl", tests/golden/tvl_smooth_long/
tvl_smooth_long_cases.npz): the cases (loaded once, never modified), the dense FP64 checker of a candidate on a window
(computed here once: the files do not store it) and the rule.

The rule, per array (β̂, V, C), with a step's error measured normwise against the reference's magnitude at that step
(smoother_reference.traj_err):

  ordinary candidate   within 1e-9 of the checker.  No truth is stored for it; the generator asserted that its checker
                       is within 1e-10 of the truth, so the scale is the checker's.
  hard candidate       smoother_reference.assert_rule unchanged: within 1e-9 of the checker, or at least as close to the
                       stored 40-digit truth as the checker is; the scale is the truth's.

and for every candidate: NaN past the window, V symmetric to the bit.

A hard (candidate, array) is a test case of its own (hard_params), so that a miss names the array; the parity tests
hold the hard candidates to everything but the rule and print their three errors.
"""
from __future__ import annotations

import functools
import sys

import numpy as np
import pytest

import smoother_reference as SR
import tvl_smoother_reference as TR
from conftest import GOLDEN

for d in ("smooth", "smooth_long", "tvl_smooth_long"):
    sys.path.insert(0, str(GOLDEN / d))
import make_smooth_long as ML  # noqa: E402
import make_tvl_smooth_long as MTL  # noqa: E402

MODELS = ("fixed", "tvl")
GENERATORS = {"fixed": ML, "tvl": MTL}
MIXED_WINDOWS = (1, 64, 65, 128, 129, 192, 193, 200)
CUT_WINDOWS = (128, 129, 193)
ARRAYS = ("beta", "V", "C")
# the hard candidates of the committed files (tests/test_smooth_long_fixture_cpu.py holds this table to them)
HARD = {"fixed": {"SL-hard": (0, 1)}, "tvl": {"TL-n90": (1,)}}


@functools.lru_cache(maxsize=None)
def cases(model) -> dict:
    return GENERATORS[model].load_cases()


def case_windows(model):
    """(case, window) pairs of a model, from the generator's tables: no file is read at collection."""
    gen = GENERATORS[model]
    return [(name, n) for name in gen.CASES
            for n in (ML.WINDOWS_CHUNK if name.endswith("-chunk") else (gen.SHAPES[name][1],))]


@functools.lru_cache(maxsize=None)
def _tvl_forward(name, b):
    c = cases("tvl")[name]
    return TR.forward_dense(c["maturities"], c["Y"], c["Theta"][:, b], 0, c["Y"].shape[1])


@functools.lru_cache(maxsize=None)
def checker(model, name, n, b):
    """(β̂, V, C) of the dense FP64 checker for candidate b on the window of n columns (any n, not only the stored ones)."""
    c = cases(model)[name]
    if model == "fixed":
        return SR.smooth_dense(c["kind"], c["maturities"], c["Y"], c["Theta"][:, b], 0, n)
    return TR.backward_dense(_tvl_forward(name, b), n)


def candidate_errors(model, name, n, b, got):
    """Per array: (got − checker,) for an ordinary candidate, (got − checker, got − truth, checker − truth) for a hard one."""
    c = cases(model)[name]
    chk = checker(model, name, n, b)
    if not c["hard"][b]:
        return {what: (SR.traj_err(g, k, k),) for what, g, k in zip(ARRAYS, got, chk)}
    tru = c["truth"][(n, b)]
    return {what: SR.rule_errors(g, k, t) for what, g, k, t in zip(ARRAYS, got, chk, tru)}


def hard_params(model):
    """pytest params (case, window, candidate, array) of the hard candidates."""
    return [pytest.param(name, n, b, what, id=f"{name}-{n}-b{b}-{what}") for name, n in case_windows(model)
            for b in HARD[model].get(name, ()) for what in ARRAYS]


def assert_hard_array(model, name, n, b, what, beta_s, V_s, C_s):
    """smoother_reference.assert_rule on one array of a hard candidate."""
    assert cases(model)[name]["hard"][b]
    k = ARRAYS.index(what)
    got = (beta_s[:, :n], V_s[:, :, :n], C_s[:, :, :n - 1])[k]
    return SR.assert_rule(got, checker(model, name, n, b)[k], cases(model)[name]["truth"][(n, b)][k],
                          (model, name, n, b, what))


def assert_candidate(model, name, n, b, beta_s, V_s, C_s):
    """beta_s M × T, V_s M × M × T, C_s M × M × (T − 1) of one candidate: finite inside the window, NaN past it, V
    symmetric to the bit, and for an ordinary candidate the rule (a hard one's arrays are held to it one by one, by
    assert_hard_array; its errors are printed here).  Returns the errors per array."""
    got = (beta_s[:, :n], V_s[:, :, :n], C_s[:, :, :n - 1])
    errs = candidate_errors(model, name, n, b, got)
    hard = bool(cases(model)[name]["hard"][b])
    for what, g in zip(ARRAYS, got):
        print((model, name, n, b, what, "hard" if hard else "ordinary"), " ".join(f"{v:.3e}" for v in errs[what]))
        assert np.isfinite(g).all(), (name, n, b, what)
    assert np.isnan(beta_s[:, n:]).all() and np.isnan(V_s[:, :, n:]).all() and np.isnan(C_s[:, :, n - 1:]).all()
    np.testing.assert_array_equal(V_s[:, :, :n], np.transpose(V_s[:, :, :n], (1, 0, 2)))
    if not hard:
        missed = {what: e for what, e in errs.items() if not e[0] <= SR.REL}
        assert not missed, (name, n, b, missed)
    return errs
