"""CPU-side checks of ABI version 5: the neural kinds' values, parameter counts and dimensions as the library, the
header and the host mirror state them (no compute calls: no GPU here; the refused entry points need a context and
are checked in tests/test_gpu_msedn.py)."""
from __future__ import annotations

import re

import pytest

from conftest import ROOT, PKG
from yfm_amd import _lib, params as P


def test_abi_version_is_5():
    lib = _lib.load()
    assert lib.yfm_abi_version() == 5 == _lib.ABI_VERSION
    txt = (ROOT / "include" / "yfm.h").read_text()
    assert re.search(r"#define YFM_ABI_VERSION 5\b", txt)


def test_header_values_are_the_mirror_s():
    txt = (ROOT / "include" / "yfm.h").read_text()
    val = {k: int(v) for k, v in re.findall(r"\b(YFM_(?:MODEL_\w+|NNS_\w+))\s*=\s*(\d+)", txt)}
    assert val["YFM_MODEL_NNS"] == P.KIND_NNS == 16 and val["YFM_MODEL_NNS_ANCHORED"] == P.KIND_NNS_ANCHORED == 17
    assert val["YFM_MODEL_SD_NNS"] == P.NEURAL_SD_BASE == 32
    assert (val["YFM_NNS_RW"], val["YFM_NNS_SCALED"], val["YFM_NNS_ANCHORED"]) == (4, 8, 16)
    assert P.neural_kind("diag", True, True, False) == 32 | 2 | 4 | 8 | 16
    # the existing values stay
    assert [val[f"YFM_MODEL_{n}"] for n in ("DNS", "TVL", "GNS5", "NS", "SD_NS", "RWSD_NS", "SSD_NS", "SRWSD_NS")] == [
        0, 1, 2, 3, 4, 5, 6, 8]
    jl = (PKG / "julia" / "YFMAMD.jl").read_text()
    assert "YFM_MODEL_NNS, YFM_MODEL_NNS_ANCHORED, YFM_MODEL_SD_NNS = Cint(16), Cint(17), Cint(32)" in jl
    assert "YFM_NNS_RW, YFM_NNS_SCALED, YFM_NNS_ANCHORED = Cint(4), Cint(8), Cint(16)" in jl


@pytest.mark.parametrize("kind", P.NEURAL_KINDS)
def test_counts_and_dims(kind):
    lib = _lib.load()
    assert lib.yfm_param_count(kind) == P.n_params(kind)
    assert lib.yfm_state_dim(kind) == 3 == P.state_dim(kind)
    assert lib.yfm_gamma_dim(kind) == 18 == P.gamma_dim(kind)


def test_values_that_are_not_kinds():
    lib = _lib.load()
    for kind in (7, 9, 15, 18, 31, 35, 39, 43, 47, 51, 55, 59, 63, 64, -1):
        assert lib.yfm_param_count(kind) == -1 and lib.yfm_state_dim(kind) == -1 and lib.yfm_gamma_dim(kind) == -1, kind
        assert not P.is_neural_kind(kind)
