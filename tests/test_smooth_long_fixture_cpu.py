"""The estimation-length smoother fixtures themselves (tests/golden/smooth_long/smooth_long_cases.npz and
tests/golden/tvl_smooth_long/tvl_smooth_long_cases.npz; no GPU): their size, that the generators' case_inputs regenerate
the stored inputs bit for bit, which candidates are hard, and that the dense FP64 checker the tests compute here is the
one the generators measured — a BLAS that moved it would show in the hard candidates' distance from the truth."""
from __future__ import annotations

import numpy as np
import pytest

import smooth_long_fixture as LF
from gpu_scenarios import same_bits

FIXED_CASES = LF.ML.CASES
TVL_CASES = LF.MTL.CASES
ALL_CASES = [("fixed", name) for name in FIXED_CASES] + [("tvl", name) for name in TVL_CASES]


@pytest.mark.parametrize("model", LF.MODELS)
def test_file_stays_under_512_KiB(model):
    gen = LF.GENERATORS[model]
    assert gen.FILE.stat().st_size < gen.MAX_BYTES == 512 * 1024


@pytest.mark.parametrize("model,name", ALL_CASES)
def test_case_inputs_regenerate_the_stored_inputs_bit_for_bit(model, name):
    c = LF.cases(model)[name]
    inp = LF.GENERATORS[model].case_inputs(name)
    if model == "fixed":
        kind, Y, m, Th, windows, unit = inp
        assert kind == c["kind"]
    else:
        Y, m, Th, windows, unit, k = inp
        assert k == c["seed_step"]
    for got, stored in ((Y, c["Y"]), (m, c["maturities"]), (Th, c["Theta"])):
        assert same_bits(np.asarray(got, dtype=np.float64), stored)
    assert tuple(windows) == c["windows"] and unit == c["unit_root"]
    assert [(name, n) for n in windows] == [cw for cw in LF.case_windows(model) if cw[0] == name]
    N, T, B = LF.GENERATORS[model].SHAPES[name]
    assert c["Y"].shape == (N, T) and c["Theta"].shape[1] == B
    assert c["e_ct"].shape == (B, len(windows), 3) and c["hard"].shape == (B,)


def test_missing_columns_sit_on_the_chunk_boundaries():
    """1-based: column 64 whole, one entry of 65, columns 128 and 129 whole, one entry of 200; SL-n64 one entry of 65."""
    for model, name in (("fixed", "SL-chunk"), ("fixed", "GL-chunk"), ("tvl", "TL-chunk")):
        nan = np.isnan(LF.cases(model)[name]["Y"])
        assert np.flatnonzero(nan.any(axis=0)).tolist() == [63, 64, 127, 128, 199]
        assert nan.sum(axis=0)[[63, 64, 127, 128, 199]].tolist() == [nan.shape[0], 1, nan.shape[0], nan.shape[0], 1]
    nan = np.isnan(LF.cases("fixed")["SL-n64"]["Y"])
    assert nan.sum() == 1 and nan[:, 64].sum() == 1
    for model, name in (("fixed", "SL-hard"), ("fixed", "GL-n30"), ("tvl", "TL-n90"), ("tvl", "TL-600")):
        assert not np.isnan(LF.cases(model)[name]["Y"]).any()


def test_the_hard_sets():
    """SL-hard: bench columns 10283 and 1679 are hard, 0 and 1 are not.  A truth is stored for exactly the hard candidates,
    on every window.  DNS and TVλ each have a hard candidate; no GNS5 candidate of these cases is one (the worst
    checker of GL-chunk and GL-n30 is 2.2e-13 from the truth), so GNS5 is held to the checker alone."""
    fixed, tvl = LF.cases("fixed"), LF.cases("tvl")
    assert fixed["SL-hard"]["hard"].tolist() == [True, True, False, False]
    for cs in (fixed, tvl):
        for name, c in cs.items():
            want = {(n, b) for b in np.flatnonzero(c["hard"]) for n in c["windows"]}
            assert set(c["truth"]) == want, name
    assert any(c["hard"].any() for c in fixed.values() if c["kind"] == LF.ML.KIND_DNS)
    assert any(c["hard"].any() for c in tvl.values())
    assert not any(c["hard"].any() for c in fixed.values() if c["kind"] == LF.ML.KIND_GNS)


@pytest.mark.parametrize("model,name", ALL_CASES)
def test_ordinary_candidates_have_a_checker_within_1e_10_of_the_truth(model, name):
    c = LF.cases(model)[name]
    assert LF.GENERATORS[model].GEN_REL == 1e-10
    assert (c["e_ct"][~c["hard"]] <= 1e-10).all()
    assert (c["e_ct"][c["hard"]].max(axis=(1, 2)) > 1e-10).all()


@pytest.mark.parametrize("model,name", ALL_CASES)
def test_checker_recomputed_here_reproduces_the_stored_distance_of_the_hard_candidates(model, name):
    """Within a factor of 2 per window and array: the checker of this machine's BLAS is the one the generator measured."""
    c = LF.cases(model)[name]
    for b in np.flatnonzero(c["hard"]):
        for wi, n in enumerate(c["windows"]):
            chk = LF.checker(model, name, n, int(b))
            tru = c["truth"][(n, int(b))]
            for k, what in enumerate(LF.ARRAYS):
                e = LF.SR.traj_err(chk[k], tru[k], tru[k])
                print(name, n, b, what, f"{e:.3e} stored {c['e_ct'][b, wi, k]:.3e}")
                assert 0.5 * c["e_ct"][b, wi, k] <= e <= 2.0 * c["e_ct"][b, wi, k], (name, n, b, what)


def test_gns5_cases_are_below_the_deferral_threshold():
    for name in ("GL-chunk", "GL-n30"):
        assert (LF.cases("fixed")[name]["kappa1"] <= LF.ML.KAPPA_MAX).all()
