"""GPU test of the DNS log-likelihood gradient (csrc/yfm_grad.hip) at estimation length: windows of up to T = 600
columns, the bench batch's own candidates, the NaN-column branch late in the panel and the band of κ₁(Z'Z) below the
deferral threshold (tests/golden/grad/grad_long_cases.npz, make_grad_long.py).

The rule is tests/test_gpu_grad.py's: per case and compared candidate (at least 75% of a case)

    max_i |g_gpu − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd[b]

with two additions that read the fixture only.  L-hard: a candidate on which the dense FP64 oracle's own loglik is
more than 1e-9 from the truth (`hard`: exactly bench columns 10283, 1679, 5390, 22413) may instead be at least as close
to the truth as a plain FP64 gradient of the same operation, err ≤ ref_err[b] — the second clause of the project's
parity rule.  L-band: a candidate with κ₁ ≤ 5e5 must have a gradient that passes the rule, one with κ₁ ≥ 2e6 must be
unavailable (NaN rows, engine.loglik's value, counted), in between either — and a gradient that is produced passes.

Observed on MI355X: DESIGN.md §3.5.
"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import assert_batch_independent
from grad_rule import assert_gradient_rule
from test_gpu_parity import assert_parity
from yfm_amd import KIND_DNS

sys.path.insert(0, str(GOLDEN / "grad"))
import make_grad_long as ML  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return ML.load_cases()


@pytest.mark.parametrize("name", ["L", "L-windows", "L-n64"])
def test_gradient_matches_truth_differences(engine, cases, name):
    c = cases[name]
    engine.set_panel(c["Y"], c["maturities"])
    ll, g = engine.loglik_grad(KIND_DNS, c["Theta"], space=0, T_use=c["T_use"])
    assert_gradient_rule(g, c, label=f"case {name}")
    assert_parity(ll, c["loglik_oracle"], c["loglik_truth"])
    assert engine.last_grad_unavailable() == 0


def test_hard_candidates(engine, cases):
    """The four hard bench columns and two benign ones: the set of hard candidates is asserted, and only they may
    use the second clause."""
    c = cases["L-hard"]
    assert c["hard"].tolist() == [True, True, True, True, False, False]
    assert c["compared"].mean() >= 0.75 and np.isfinite(c["ref_err"][c["hard"]]).all()
    engine.set_panel(c["Y"], c["maturities"])
    ll, g = engine.loglik_grad(KIND_DNS, c["Theta"], space=0, T_use=c["T_use"])
    assert_gradient_rule(g, c, label="case L-hard", second_clause=c["hard"])
    assert_parity(ll, c["loglik_oracle"], c["loglik_truth"])
    assert engine.last_grad_unavailable() == 0


def test_band_below_the_deferral_threshold(engine, cases):
    c = cases["L-band"]
    k1 = c["kappa1"]
    assert c["compared"].mean() >= 0.75
    engine.set_panel(c["Y"], c["maturities"])
    ll, g = engine.loglik_grad(KIND_DNS, c["Theta"], space=0, T_use=c["T_use"])
    have = np.isfinite(g).all(axis=0)
    print("case L-band: κ₁", " ".join(f"{k:.2e}" for k in k1), "gradient produced:", have.astype(int).tolist())
    assert np.all(have | np.isnan(g).all(axis=0))
    assert np.all(have[k1 <= 5e5]) and not np.any(have[k1 >= 2e6])
    assert (k1 <= 5e5).sum() >= 3 and (k1 >= 2e6).sum() >= 2
    assert engine.last_grad_unavailable() == int((~have).sum()) == engine.last_deferred()
    np.testing.assert_array_equal(ll, engine.loglik(KIND_DNS, c["Theta"], space=0, T_use=c["T_use"]))
    assert np.all(c["compared"][k1 <= 5e5])
    assert_gradient_rule(g, c, label="case L-band", sel=c["compared"] & have)
    assert_parity(ll, c["loglik_oracle"], c["loglik_truth"])


def test_outputs_do_not_depend_on_the_batch(engine, cases):
    """Candidate 47 of L alone, inside the batch of 48 and with the batch reversed: the same bits."""
    c = cases["L"]
    engine.set_panel(c["Y"], c["maturities"])
    Th = c["Theta"]
    ll, g = assert_batch_independent(lambda X: engine.loglik_grad(KIND_DNS, X), Th, [47])
    assert np.isfinite(g[:, 47]).all()
