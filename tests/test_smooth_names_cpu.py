"""The smoother's public names: include/yfm.h declares the two entry points, says that they are an extension and carries
the definitions; yfm_amd._lib binds them with matching argument lists; the ABI version stays 5 (the change is additive);
the library exports them; the package exports the host mirror; the Julia wrapper calls them."""
import ctypes
import re
import subprocess

import pytest

import yfm_amd
from conftest import ROOT
from yfm_amd import _lib, engine, smoothing

NAMES = ("yfm_smooth_batch", "yfm_smooth_batch_device")


def header():
    return (ROOT / "include" / "yfm.h").read_text()


def test_header_declares_the_entry_points():
    h = header()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    doc = h[h.index("The fixed-interval Kalman smoother"):h.index("int yfm_smooth_batch(")]
    assert "EXTENSION" in doc and "no counterpart" in doc
    for word in ("B_t = σ²I + G P_t", "s_t = B_t⁻¹(Z'y_t − G a_t)", "W_t = B_t⁻¹G", "L_t = Φ(I − P_t W_t)",
                 "r_{t−1} = s_t + L_t' r_t", "N_{t−1} = W_t + L_t' N_t L_t", "β̂_t = a_t + P_t r_{t−1}",
                 "V_t = P_t − P_t N_{t−1} P_t", "(I − P_{t+1} N_t) L_t P_t", "any(isnan.(y))", "n = 1 is valid",
                 "symmetric to the bit", "may be NULL", "deferral list", "yfm_last_batch_grad_unavailable",
                 "bitwise independent", "128 MiB", "YFM_EUNSUPPORTED", "B = 0 succeeds"):
        assert word in doc, word


def test_lib_binds_them():
    t = _lib.SIGNATURES
    res, args = t["yfm_smooth_batch"]
    assert res is ctypes.c_int and args == t["yfm_filter_states"][1]
    res, args = t["yfm_smooth_batch_device"]
    assert res is ctypes.c_int and len(args) == 11
    assert _lib.ABI_VERSION == 5
    for n in NAMES:
        decl = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\);", header()).group(1)
        assert len(decl.split(",")) == len(t[n][1]), n


def test_library_exports_them():
    if not _lib.LIB_PATH.exists():
        pytest.skip("in-tree library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True,
                         text=True).stdout
    for n in NAMES:
        assert re.search(r"\bT " + n + r"$", out, re.M), n


def test_package_exports_the_host_mirror():
    for n in ("smooth", "smooth_device"):
        assert hasattr(engine.Engine, n), n
    for n in ("smoothing", "smooth_batch", "smooth_", "smoothed_yields", "em_moments"):
        assert n in yfm_amd.__all__ and hasattr(yfm_amd, n), n
    assert yfm_amd.smooth_batch is smoothing.smooth_batch


def test_refused_models_name_the_gap():
    """The kinds the entry point refuses raise NotImplementedError before any device call, naming what is missing."""
    class M:
        def __init__(self, kind):
            self.kind = kind
    for kind, word in ((yfm_amd.KIND_TVL, "extended smoother"), (yfm_amd.KIND_SD_NS, "not Kalman filters"),
                       (yfm_amd.KIND_NNS, "not Kalman filters")):
        with pytest.raises(NotImplementedError, match=word):
            smoothing.smooth_batch(M(kind), None, None)
        with pytest.raises(NotImplementedError, match=word):
            engine.Engine._smooth_kinds(kind, "smooth")


def test_julia_wrapper_and_documents_name_them():
    jl = (ROOT / "yieldfactormodels.jl_amd" / "julia" / "YFMAMD.jl").read_text()
    assert "LIB.yfm_smooth_batch(" in jl and "function smooth(" in jl
    assert "yfm_smooth_batch" in (ROOT / "INTEGRATION.md").read_text()
    design = (ROOT / "DESIGN.md").read_text()
    assert "### 3.12" in design and "yfm_smooth_batch" in design
    assert "smooth" in (ROOT / "README.md").read_text()
