"""What the TVλ smoother's CPU and GPU tests share: the cases of tests/golden/tvl_smooth/tvl_smooth_cases.npz (loaded
once, never modified) and the comparison of a candidate's three arrays under the rule of tests/smoother_reference.py."""
from __future__ import annotations

import functools
import sys

import numpy as np

import tvl_smoother_reference as TR
from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN / "tvl_smooth"))
import make_tvl_smooth as MT  # noqa: E402

CASES = MT.CASES
# (case, window) pairs: every case on its whole panel, T-n30 also on its shorter windows
CASE_WINDOWS = [(name, n) for name in CASES for n in (MT.WINDOWS_N30 if name == "T-n30" else (None,))]


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    return MT.load_cases()


def window_of(c, n):
    return c["Y"].shape[1] if n is None else n


@functools.lru_cache(maxsize=None)
def checker_constrained(name, n, b):
    """The dense FP64 checker at the stored constrained θ (cheap, so not stored)."""
    c = cases()[name]
    return TR.smooth_dense(c["maturities"], c["Y"], c["Theta_c"][:, b], 1, n)


def references(name, n, b, space):
    """((β, V, C) of the checker, (β, V, C) of the truth) of candidate b on a window of n columns."""
    w = cases()[name]["windows"][n]
    if space == 0:
        chk = (w["beta_chk"][..., b], w["V_chk"][..., b], w["C_chk"][..., b])
        tru = (w["beta_tru"][..., b], w["V_tru"][..., b], w["C_tru"][..., b])
    else:
        chk = checker_constrained(name, n, b)
        tru = (w["beta_tru1"][..., b], w["V_tru1"][..., b], w["C_tru1"][..., b])
    return chk, tru


def assert_candidate(name, n, b, space, beta_s, V_s, C_s):
    """beta_s 4 × T, V_s 4 × 4 × T, C_s 4 × 4 × (T − 1) of one candidate: the rule inside the window, NaN past it."""
    chk, tru = references(name, n, b, space)
    got = (beta_s[:, :n], V_s[:, :, :n], C_s[:, :, :n - 1])
    worst = {}
    for what, g, c, t in zip(("beta", "V", "C"), got, chk, tru):
        worst[what] = TR.assert_rule(g, c, t, (name, n, b, space, what))
    assert np.isnan(beta_s[:, n:]).all() and np.isnan(V_s[:, :, n:]).all() and np.isnan(C_s[:, :, n - 1:]).all()
    np.testing.assert_array_equal(V_s[:, :, :n], np.transpose(V_s[:, :, :n], (1, 0, 2)))
    return worst
