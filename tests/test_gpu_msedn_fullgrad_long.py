"""GPU test of the neural models' full gradient at estimation length (tests/golden/msedn_fullgrad/
msedn_fullgrad_long.npz): T = 600, N = 30, NNS, 1SD-NNS, 3SSD-NNS and 1SRWSD-NNS, against the torch checker's gradient
(tests/msedn_fullgrad_torch.py, reverse-mode autograd of the restated filter) under the project's bar,
max|g − g_ad| ≤ 1e-9·‖g_ad‖∞ over all P rows, and against the 40-digit central differences of the N = 5 anchor under the
truth rule, max|g − g_fd| ≤ 1e-9·‖g_fd‖∞ + e_fd over its leading rows — under both lane counts.  Prints err / ‖g‖∞ per
kind (DESIGN.md §3.10 quotes them)."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_scenarios import same_bits

sys.path.insert(0, str(GOLDEN / "msedn_fullgrad"))
import make_msedn_fullgrad_long as ML  # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-9


@pytest.fixture(scope="module")
def cases():
    return ML.load_cases()


@pytest.fixture
def lanes_env():
    old = os.environ.pop("YFM_MSED_LANES", None)
    yield
    os.environ.pop("YFM_MSED_LANES", None)
    if old is not None:
        os.environ["YFM_MSED_LANES"] = old


def kind_of(name: str) -> int:
    return int(name[1:name.index("_")])


@pytest.mark.parametrize("lanes", ["4", "16"])
@pytest.mark.parametrize("name", ML.long_names())
def test_long_gradient_matches_the_checker(engine, cases, lanes_env, name, lanes):
    c, kind = cases, kind_of(name)
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    os.environ["YFM_MSED_LANES"] = lanes
    Th, tu, g_ad = c[f"{name}_theta"], c[f"{name}_T_use"], c[f"{name}_g_ad"]
    loss, g = engine.neural_loss_full_grad(kind, Th, space=0, T_use=tu)
    assert engine.last_flags() == (0, int(np.isnan(g_ad).any(axis=0).sum())) and engine.last_grad_unavailable() == 0
    assert same_bits(loss, engine.loglik(kind, Th, space=0, T_use=tu))
    _, g12 = engine.neural_loss_grad(kind, Th, space=0, T_use=tu)
    fin = np.isfinite(loss)
    assert same_bits(g[-12:, fin], g12[:, fin])
    for b in range(Th.shape[1]):
        if np.isnan(g_ad[:, b]).any():
            assert np.isneginf(loss[b]) and np.isnan(g[:, b]).all()
            continue
        want = c[f"{name}_loss"][b]
        assert abs(loss[b] - want) <= REL * abs(want)
        top = np.max(np.abs(g_ad[:, b]))
        err = np.max(np.abs(g[:, b] - g_ad[:, b]))
        print(f"{name} L={lanes} b={b}: err / |g|inf = {err / top:.3e} (|g|inf {top:.3e})")
        assert err <= REL * top, (name, b, err, top)


@pytest.mark.parametrize("lanes", ["4", "16"])
def test_long_anchor_matches_the_truth(engine, cases, lanes_env, lanes):
    c, name = cases, ML.anchor_name()
    kind = kind_of(name)
    engine.set_panel(c[f"{name}_Y"], c[f"{name}_maturities"])
    os.environ["YFM_MSED_LANES"] = lanes
    loss, g = engine.neural_loss_full_grad(kind, c[f"{name}_theta"], space=0, T_use=c[f"{name}_T_use"])
    g_fd, e_fd = c[f"{name}_g_fd"][:, 0], float(c[f"{name}_e_fd"][0])
    assert np.isfinite(loss[0]) and np.isfinite(g).all() and engine.last_grad_unavailable() == 0
    err, top = np.max(np.abs(g[:len(g_fd), 0] - g_fd)), np.max(np.abs(g_fd))
    print(f"{name} L={lanes}: max|g - g_fd| / |g_fd|inf = {err / top:.3e}, e_fd {e_fd:.3e}")
    assert err <= REL * top + e_fd
