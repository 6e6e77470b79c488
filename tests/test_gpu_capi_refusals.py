"""Every batched entry point of include/yfm.h refuses a bad call with the return code and the yfm_last_error() text
recorded in tests/golden/capi_refusals/refusals.json — written by make_capi_refusals.py from the library as it was
before the entry points were folded into one path per call family.  The matrix (one kind of each class × no panel,
wrong P, B = −1, unknown param_space, null θ, T_use outside [1, T], a kind or an N the entry point refuses, lags = −1,
both matrices null, horizon = 0, K = 0; a 30 × 4 and a 65 × 2 panel) is the generator's: every case is refused by the
checks at the top of its entry point, so no kernel runs here except yfm_set_panel's."""
from __future__ import annotations

import importlib.util

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DIR = GOLDEN / "capi_refusals"


def _generator():
    spec = importlib.util.spec_from_file_location("make_capi_refusals", DIR / "make_capi_refusals.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refusals_match_the_recorded_codes_and_texts(engine):
    gen = _generator()
    want = gen.load()
    got = gen.run_matrix(engine.lib)
    assert got.keys() == want.keys(), sorted(got.keys() ^ want.keys())[:10]
    assert all(rc != 0 for rc, _ in want.values())
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, (len(wrong), list(wrong.items())[:5])
