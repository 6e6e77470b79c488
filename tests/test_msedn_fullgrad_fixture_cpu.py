"""CPU checks of the neural full gradient's fixtures (tests/golden/msedn_fullgrad/): the truth file's self-consistency —
the stored autograd gradient ten times inside the tests' bar on every candidate, the differences converged, every
leading row of every kind above the screen in some candidate, the special cases where they should be — the torch
checker (tests/msedn_fullgrad_torch.py) rerun on a subset against the stored truth, and the long file's anchor."""
from __future__ import annotations

import importlib.util
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN / "msedn_fullgrad"))
import make_msedn_fullgrad as MF  # noqa: E402
import make_msedn_fullgrad_long as ML  # noqa: E402
import msedn_fullgrad_torch as TQ  # noqa: E402
import msedn_reference as R  # noqa: E402

# the λ models' generator has the same file name (tests/golden/msed_fullgrad/): this one is loaded under a name of its own
_spec = importlib.util.spec_from_file_location("make_neural_estimate_full",
                                               GOLDEN / "msedn_fullgrad" / "make_estimate_full.py")
ME = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ME)


@pytest.fixture(scope="module")
def cases():
    return MF.load_cases()


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


def test_truth_file_is_self_consistent(cases):
    c = cases
    covered = {}
    for name in MF.case_names():
        kind = kind_of(name)
        nl = R.n_params(kind) - 12
        for space in MF.case_spaces(name):
            g_fd, e_fd, g_ad = (c[f"{name}_{k}_s{space}"] for k in ("g_fd", "e_fd", "g_ad"))
            Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
            assert g_fd.shape == (nl, Th.shape[1]) and g_ad.shape == Th.shape
            for b in range(Th.shape[1]):
                if np.isnan(g_fd[:, b]).any():
                    assert np.isneginf(c[f"{name}_loss_s{space}"][b]) and np.isnan(g_ad[:, b]).all()
                    continue
                top = np.max(np.abs(g_fd[:, b]))
                assert e_fd[b] <= 1e-9 * top, (name, space, b)
                assert np.max(np.abs(g_ad[:nl, b] - g_fd[:, b])) <= MF.SELF_REL * top + e_fd[b], (name, space, b)
                cov = covered.setdefault(kind, np.zeros(nl, dtype=bool))
                cov |= np.abs(g_fd[:, b]) >= MF.SCREEN * top
    assert sorted(covered) == sorted(MF.kinds())
    for kind, cov in covered.items():
        assert cov.all(), (kind, np.where(~cov)[0])  # no leading row goes unchecked
    print("worst autograd error relative to |g_fd|inf:", float(c["worst_checker_rel"]))
    assert float(c["worst_checker_rel"]) <= MF.SELF_REL


def test_special_cases_are_where_they_should_be(cases):
    for kind in MF.kinds():
        assert np.isnan(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 1:]).all()
        assert np.isfinite(cases[f"k{kind}_n4t8nan6_g_fd_s0"][:, 0]).all()
        assert np.isnan(cases[f"k{kind}_n4t8nan6_Y"][:, 5]).all()
        assert list(cases[f"k{kind}_n4t8nan6_T_use"]) == [5, 8, 8]
        assert np.isnan(cases[f"k{kind}_n4t8nan0_Y"][:, 0]).all()
        assert np.isfinite(cases[f"k{kind}_n4t8nan0_g_fd_s0"]).all()
        assert f"k{kind}_n4t8_theta_c" in cases and f"k{kind}_n33t8_theta_c" not in cases


@pytest.mark.parametrize("kind", MF.kinds())
def test_torch_checker_reproduces_the_stored_gradient(cases, kind):
    """N = 4, T = 8 in both spaces and the prediction-only first step: the checker run here gives the stored g_ad (to
    rounding) and so stands inside the bar against the stored truth."""
    c = cases
    for name, spaces in ((f"k{kind}_n4t8", (0, 1)), (f"k{kind}_n4t8nan0", (0,))):
        for space in spaces:
            Th = c[f"{name}_theta"] if space == 0 else c[f"{name}_theta_c"]
            for b in range(Th.shape[1]):
                loss, g = TQ.loss_and_grad(kind, c[f"{name}_maturities"], c[f"{name}_Y"], Th[:, b], space,
                                           int(c[f"{name}_T_use"][b]))
                want = c[f"{name}_loss_s{space}"][b]
                assert abs(loss - want) <= 1e-12 * abs(want)
                g_fd, e_fd = c[f"{name}_g_fd_s{space}"][:, b], c[f"{name}_e_fd_s{space}"][b]
                top = np.max(np.abs(g_fd))
                assert np.max(np.abs(g - c[f"{name}_g_ad_s{space}"][:, b])) <= 1e-11 * np.max(np.abs(g))
                assert np.max(np.abs(g[:len(g_fd)] - g_fd)) <= MF.SELF_REL * top + e_fd


def test_long_file_and_its_anchor():
    c = ML.load_cases()
    for name in ML.long_names():
        kind = kind_of(name)
        assert c[f"{name}_Y"].shape == (30, 600) and c[f"{name}_g_ad"].shape == (R.n_params(kind), 2)
    nan = "k32_n30t600nan450"
    assert np.isnan(c[f"{nan}_Y"][:, 450]).all() and list(c[f"{nan}_T_use"]) == [300, 600]
    assert np.isfinite(c[f"{nan}_g_ad"][:, 0]).all() and np.isnan(c[f"{nan}_g_ad"][:, 1]).all()
    assert np.isneginf(c[f"{nan}_loss"][1])
    a = ML.anchor_name()
    g_fd, e_fd, g_ad = c[f"{a}_g_fd"][:, 0], float(c[f"{a}_e_fd"][0]), c[f"{a}_g_ad"][:, 0]
    assert c[f"{a}_Y"].shape == (5, 600) and len(g_fd) == 22
    top = np.max(np.abs(g_fd))
    assert e_fd <= 1e-9 * top and np.max(np.abs(g_ad[:22] - g_fd)) <= MF.SELF_REL * top + e_fd


def test_estimate_reference_follows_its_recipe():
    c = ME.load()
    assert c["Y"].shape == (4, 40) and list(c["windows"]) == list(ME.WINDOWS)
    for kind in ME.KINDS:
        assert len(c[f"k{kind}_start_c"]) == R.n_params(kind)
        for w in ME.WINDOWS:
            pre = f"k{kind}_w{w}"
            runs = c[f"{pre}_ll_runs"]
            assert float(c[f"{pre}_ll_ref"]) == runs.max()
            assert float(c[f"{pre}_G"]) == max(1e-6, 10.0 * abs(runs[0] - runs[1]))
            assert runs.min() > float(c[f"{pre}_ll_start"])  # both reference runs improved on the start
