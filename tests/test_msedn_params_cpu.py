"""Host mirror of the neural Nelson–Siegel models: the 26 codes and strings (create_neural_model) of
model_dictionary.jl:20-112, parameter counts, layouts, the duplicator, the transforms and the trial grid of
get_new_initial_params' multi-unique branch (msedriven/paramteroperations.jl:161-184)."""
from __future__ import annotations

import numpy as np
import pytest

import msedn_reference as R
from yfm_amd import models as M
from yfm_amd import params as P
from yfm_amd import synthetic as S

# model_dictionary.jl:20-112: string, numeric code, (dynamics, random_walk, scale_grad, transform_bool)
SD = []
for anchored, first in ((False, 8), (True, 21)):
    code = first
    for scaled in (False, True):
        for d, dyn in enumerate(("scalar", "block_diag", "diag")):
            for rw in (False, True):
                name = f"{d + 1}{'S' if scaled else ''}{'RW' if rw else ''}SD-NNS{'-Anchored' if anchored else ''}"
                SD.append((name, str(code), dyn, rw, scaled, not anchored))
                code += 1


def test_the_table_above_is_the_reference_s():
    assert len(SD) == 24
    assert SD[0][:2] == ("1SD-NNS", "8") and SD[5][:2] == ("3RWSD-NNS", "13") and SD[6][:2] == ("1SSD-NNS", "14")
    assert SD[11][:2] == ("3SRWSD-NNS", "19") and SD[12][:2] == ("1SD-NNS-Anchored", "21")
    assert SD[17][:2] == ("3RWSD-NNS-Anchored", "26") and SD[23][:2] == ("3SRWSD-NNS-Anchored", "32")


@pytest.mark.parametrize("name,code,dyn,rw,scaled,transform", SD)
def test_score_driven_codes(name, code, dyn, rw, scaled, transform):
    mats = S.maturities_30()
    for key in (name, code):
        m, std = M.create_neural_model(key, mats, 30, 3)
        assert std == name and isinstance(m, M.MSEDNeuralModel)
        assert (m.dynamics, m.random_walk, m.scale_grad, m.transform_bool) == (dyn, rw, scaled, transform)
        assert m.base.M == 3 and m.base.L == 18 and m.base.model_string == key
        assert m.kind == P.neural_kind(dyn, rw, scaled, transform) == R.sd_kind(P.NEURAL_DYNAMICS.index(dyn), rw, scaled,
                                                                             not transform)
        assert P.KIND_NAMES[m.kind] == name
    nu = {"scalar": 2, "block_diag": 6, "diag": 18}[dyn]
    want = nu * (1 if rw else 2) + 30
    assert P.n_params(m.kind) == want == R.n_params(m.kind) == len(M.get_params(m))
    assert want == {("scalar", False): 34, ("scalar", True): 32, ("block_diag", False): 42, ("block_diag", True): 36,
                    ("diag", False): 66, ("diag", True): 48}[(dyn, rw)]
    assert P.gamma_dim(m.kind) == 18 and P.state_dim(m.kind) == 3 and P.is_neural_kind(m.kind)
    assert m.A_guesses == (1e-6, 1e-5, 1e-4, 1e-3) and m.B_guesses == (0.97, 0.98, 0.99, 0.999)
    assert m.forget_factor == 0.9
    groups = M.get_param_groups(m)
    assert groups == ["1"] * (want - 12) + ["2"] * 12  # msebasemodel.jl:153-162
    assert M.get_param_groups(m, ["7"] * want) == ["7"] * want


def test_static_codes():
    mats = S.maturities_30()
    for keys, std_want, kind, transform in ((("NNS", "3"), "NNS", P.KIND_NNS, True),
                                            (("NNS-Anchored", "20"), "NNS-Anchored", P.KIND_NNS_ANCHORED, False)):
        for key in keys:
            m, std = M.create_neural_model(key, mats, 30, 3)
            assert std == std_want and isinstance(m, M.StaticNeuralModel) and m.kind == kind
            assert m.transform_bool is transform and m.base.L == 18
        assert P.n_params(kind) == 30 == R.n_params(kind)
        assert list(P.transform_codes(kind)) == [P.ID] * 21 + [P.R11, 0, 0, 0, P.R11, 0, 0, 0, P.R11]
    assert len(P.NEURAL_KINDS) == 26 == len(set(P.NEURAL_KINDS)) and set(P.NEURAL_KINDS) == set(R.all_kinds())
    assert not any(P.is_lambda_kind(k) or k in (P.KIND_DNS, P.KIND_TVL, P.KIND_GNS) for k in P.NEURAL_KINDS)
    with pytest.raises(ValueError):
        M.create_neural_model("RW", mats, 30, 3)  # out of scope, like "pC" and "vanillaNN"
    for code in ("SD-NS", "1C", "33", "7"):  # the other tables' codes are not this one's
        with pytest.raises(ValueError):
            M.create_neural_model(code, mats, 30, 3)
    assert len(M._NEURAL_CODES) == 52 and not set(M._NEURAL_CODES) & set(M._CODES)
    with pytest.raises(ValueError) as e:  # create_model refuses the neural codes and names the way in
        M.create_model("1SD-NNS", mats, 30, 3)
    assert "create_neural_model" in str(e.value)
    with pytest.raises(ValueError):
        P.neural_kind("full")


def test_duplicator_expansion():
    """mseneural.jl:33-48: scalar 9 + 9, block_diag 3 each, diag one each."""
    assert list(P.neural_duplicator(P.neural_kind("scalar"))) == [0] * 9 + [1] * 9
    assert list(P.neural_duplicator(P.neural_kind("block_diag"))) == [k // 3 for k in range(18)]
    assert list(P.neural_duplicator(P.neural_kind("diag"))) == list(range(18))
    np.testing.assert_array_equal(P.expand_unique(P.neural_kind("block_diag"), np.arange(6) * 10.0),
                                  np.repeat(np.arange(6) * 10.0, 3))
    m, _ = M.create_neural_model("2SD-NNS", S.maturities_30(), 30, 3)
    assert list(m.duplicator) == [k // 3 + 1 for k in range(18)]  # 1-based, as the reference's
    # the restatement's model holds the expanded vectors
    kind = P.neural_kind("block_diag")
    th = P.transform_params(kind, S.theta_batch(kind, 1, bad_frac=0.0)[:, 0])
    mod = R.set_params(kind, th, S.maturities_30())
    np.testing.assert_array_equal(mod.A, np.repeat(th[:6], 3))
    np.testing.assert_array_equal(mod.B, np.repeat(th[6:12], 3))
    np.testing.assert_array_equal(mod.nu, (1 - mod.B) * th[12:30])


@pytest.mark.parametrize("kind", P.NEURAL_KINDS)
def test_transform_round_trip(kind):
    Th = S.theta_batch(kind, 16, seed=7, bad_frac=0.0)
    lay = P.neural_layout(kind)
    assert Th.shape == (lay.P, 16) and lay.phi_offset + 9 == lay.P and lay.delta_offset == lay.gamma_offset + 18
    codes = P.transform_codes(kind)
    nu = lay.n_unique
    assert list(codes[:nu]) == [P.POS] * nu
    assert list(codes[nu:lay.n_lead]) == ([P.U01] * nu if P.neural_has_b(kind) else [])
    assert list(codes[lay.n_lead:lay.phi_offset]) == [P.ID] * 21
    Tc = P.transform_params(kind, Th)
    for b in range(3):  # the restatement's transform, entry by entry
        np.testing.assert_allclose(Tc[:, b], R.transform_params(kind, Th[:, b]), rtol=1e-15)
    np.testing.assert_allclose(P.untransform_params(kind, Tc), Th, rtol=1e-11, atol=1e-13)
    assert np.all(Tc[:nu] >= 1e-4 * (1 - 1e-12)) and np.all(Tc[:nu] <= 1e-3 * (1 + 1e-12))  # A over 1e-4 … 1e-3
    if P.neural_has_b(kind):
        assert np.all(np.abs(Tc[nu:2 * nu] - 0.98) < 0.02)
    g = Th[lay.gamma_offset:lay.gamma_offset + 18]
    assert np.all(g[3:6] == 0.0) and np.all(g[12:15] == 0.0) and 0.05 < g[[0, 1, 2, 6, 7, 8]].std() < 0.2
    assert S.theta0(kind).shape == (lay.P,)


def test_existing_draws_are_unchanged():
    """theta_batch of a kind from before the neural models: the same numbers as a plain θ₀ + scale·N(0, I)."""
    for kind in (P.KIND_DNS, P.KIND_SD_NS):
        rng = np.random.Generator(np.random.PCG64(5))
        want = S.theta0(kind)[:, None] + 0.1 * rng.standard_normal((P.n_params(kind), 4))
        np.testing.assert_array_equal(S.theta_batch(kind, 4, seed=5, bad_frac=0.0), want)


def test_trial_grid_by_hand():
    """Trial k (1-based): A₁ = (k−1) ÷ 64, A₂ = ((k−1) mod 64) ÷ 16, B₁ = ((k−1) mod 16) ÷ 4, B₂ = (k−1) mod 4;
    random walk: A₁ = (k−1) ÷ 4, A₂ = (k−1) mod 4."""
    A, Bg = (1e-6, 1e-5, 1e-4, 1e-3), (0.97, 0.98, 0.99, 0.999)
    m, _ = M.create_neural_model("2SD-NNS", S.maturities_30(), 30, 3)  # 6 unique values: halves of 3
    grid = M._trial_grid(m)
    assert grid.shape == (12, 256)
    np.testing.assert_array_equal(grid[:, 0], [A[0]] * 6 + [Bg[0]] * 6)                       # trial 1
    np.testing.assert_array_equal(grid[:, 255], [A[3]] * 6 + [Bg[3]] * 6)                     # trial 256
    # trial 100: 99 = 1·64 + 35, 35 = 2·16 + 3, 3 = 0·4 + 3
    np.testing.assert_array_equal(grid[:, 99], [A[1]] * 3 + [A[2]] * 3 + [Bg[0]] * 3 + [Bg[3]] * 3)
    np.testing.assert_array_equal(grid[:, 1], [A[0]] * 6 + [Bg[0]] * 3 + [Bg[1]] * 3)         # B₂ cycles fastest
    rw, _ = M.create_neural_model("3RWSD-NNS", S.maturities_30(), 30, 3)
    g2 = M._trial_grid(rw)
    assert g2.shape == (18, 16)
    np.testing.assert_array_equal(g2[:, 0], [A[0]] * 18)
    np.testing.assert_array_equal(g2[:, 15], [A[3]] * 18)
    np.testing.assert_array_equal(g2[:, 6], [A[1]] * 9 + [A[2]] * 9)                          # trial 7: 6 = 1·4 + 2
    # and the restatement's walk produces the same leading rows, trial by trial
    for model, kind in ((m, m.kind), (rw, rw.kind)):
        grid = M._trial_grid(model)
        p = S.theta0_constrained(kind)
        for k in range(1, grid.shape[1] + 1):
            p = R.trial_params(kind, p, k)
            np.testing.assert_array_equal(p[:grid.shape[0]], grid[:, k - 1])
        assert R.trial_params(kind, p, grid.shape[1] + 1) is None


def test_what_is_not_built_says_so():
    mats = S.maturities_30()
    Y = np.zeros((30, 8))
    m, _ = M.create_neural_model("1SD-NNS", mats, 30, 3)
    th = S.theta0_constrained(m.kind)
    from yfm_amd import driver as D
    for call in (lambda: M.estimate_steps_(m, Y, th[:, None]), lambda: M.estimate_(m, Y, th[:, None]),
                 lambda: M.estimate_batch(m, Y, th[:, None]), lambda: M.estimate_steps_batch(m, Y, th[:, None]),
                 lambda: M.compute_loss_grad_block(m, Y, th[:, None]),
                 lambda: D.run_estimation_(m, Y, 8, th[:, None], ["1"] * len(th), 1, 1e-8)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "neural" in str(e.value)
    s, _ = M.create_neural_model("NNS", mats, 30, 3)
    for call in (lambda: M.try_initializations(S.theta0_constrained(s.kind), s, Y),
                 lambda: M.try_initializations_batch(S.theta0_constrained(s.kind)[:, None], s, Y)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "Julia" in str(e.value)
