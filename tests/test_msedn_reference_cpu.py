"""The neural models' checker against itself (tests/msedn_reference.py): its Float64 run against its 40-digit run
on parity inputs, and its written-out score against central differences of the 40-digit loss.

Bounds, and where they come from:
* FLOAT against TRUTH ≤ 1e-9 relative — the parity rule's first clause.  With Float64 emulated at 53 bits, T = 40,
  N ∈ {4, 5, 30}, plain and scaled, both transforms, the worst gap measured was 1.4e-15; on the values recorded in
  tests/golden/msedn/ (T = 40, all 26 kinds at N ∈ {4, 30}, six kinds at N ∈ {5, 33, 90}) it is 3.8e-14.
* score against central differences (h = 1e-12 and 3e-12) ≤ 1e-12·‖g‖∞ — at 200 bits the formulas agree with
  central differences to 1.1e-26; at 40 digits the difference quotient's own error is O(h²) ≈ 1e-24 relative.
"""
from __future__ import annotations

import sys

import mpmath as mp
import numpy as np
import pytest

from conftest import GOLDEN

import msedn_reference as R

sys.path.insert(0, str(GOLDEN / "msedn"))
import make_msedn as MM  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return MM.load_cases()


def test_float_against_truth_on_recorded_parity_inputs(cases):
    worst, n = 0.0, 0
    for key, truth in cases.items():
        if not key.startswith("truth_"):
            continue
        ref = cases["float_" + key[6:]][:len(truth)]
        assert np.all(np.isfinite(truth)) and np.all(np.isfinite(ref))
        worst = max(worst, float(np.max(np.abs(ref - truth) / np.abs(truth))))
        n += len(truth)
    print("recorded truths", n, "worst FLOAT-to-TRUTH gap", worst)
    assert n >= 2 * (26 * 2 + 6 * 3)
    assert worst <= 1e-9


@pytest.mark.parametrize("kind,N", [(R.KIND_NNS, 4), (R.sd_kind(0), 5), (R.sd_kind(2, False, True, True), 4),
                                    (R.sd_kind(1, True), 30)])
def test_recorded_values_are_the_restatement_s(cases, kind, N):
    """The file is the restatement's output for the seeded inputs: candidate 0 recomputed in both arithmetics (T = 8
    keeps the 40-digit run short; the T = 40 truth is compared as recorded)."""
    T = 8 if kind in MM.REP_KINDS else 40
    for space in (0, 1):
        th = MM.theta_for(kind, space)[:, 0]
        got = R.get_loss(kind, MM.mats_for(N), MM.panel_for(N, T), th, space, R.FLOAT)
        assert got == cases[f"float_{kind}_{N}_{T}_{space}"][0]
    if T == 8:
        truth = R.get_loss(kind, MM.mats_for(N), MM.panel_for(N, 8), MM.theta_for(kind, 0)[:, 0], 0, R.TRUTH)
        assert abs(cases[f"float_{kind}_{N}_8_0"][0] - truth) <= 1e-9 * abs(truth)


def test_every_parity_reference_is_finite(cases):
    for (kind, N, T, space), n in MM.parity_cases().items():
        v = cases[f"float_{kind}_{N}_{T}_{space}"]
        assert v.shape == (n,) and np.all(np.isfinite(v)) and np.all(v < 0.0)


@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("N", MM.SCORE_N)
def test_score_against_central_differences(cases, N, anchored):
    kind = R.sd_kind(2, anchored=anchored)
    mats = MM.mats_for(N)
    tag = f"{N}_{int(anchored)}"
    gam, beta, y, g_rec = (cases[f"score_{k}_{tag}"] for k in ("gamma", "beta", "y", "g"))
    with mp.workdps(R.TRUTH.digits):
        ar = R.TRUTH
        m = R.Model()
        m.ar, m.anchored, m.kind = ar, anchored, kind
        m.maturities = ar.vec(mats)
        m.N = N
        gm, bm, ym = ar.vec(gam), ar.vec(beta), ar.vec(y)
        g = R.score(m, gm, bm, ym)
        scale = max(abs(v) for v in g)
        assert scale > 0
        for h in (mp.mpf("1e-12"), mp.mpf("3e-12")):
            for k in range(R.G):
                up, dn = gm.copy(), gm.copy()
                up[k] += h
                dn[k] -= h
                fd = (R.loss_at_gamma(kind, mats, up, bm, ym) - R.loss_at_gamma(kind, mats, dn, bm, ym)) / (2 * h)
                assert abs(fd - g[k]) <= mp.mpf("1e-12") * scale, (k, float(h), float(fd), float(g[k]))
        # the recorded score was taken at the 40-digit β, this one at β rounded to Float64: the residual v = y − Zβ
        # moves by 1e-16·‖y‖, up to 1e-13 of itself, and the score with it
        assert np.max(np.abs(ar.to_float(g) - g_rec)) <= 1e-12 * float(scale)
    # and the Float64 run of the same text
    mf = R.Model()
    mf.ar, mf.anchored, mf.kind, mf.maturities, mf.N = R.FLOAT, anchored, kind, mats, N
    gf = R.score(mf, gam, beta, y)
    assert np.max(np.abs(gf - g_rec)) <= 1e-9 * np.max(np.abs(g_rec))
