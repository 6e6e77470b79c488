"""The TVλ smoother's public names: include/yfm.h declares the two entry points, says that they are an extension and
carries the definitions; yfm_amd._lib binds them with the argument lists of yfm_smooth_batch(_device); the ABI version
stays 5 (the change is additive); the library exports them; the package exports the host mirror; the Julia wrapper
calls them; the documents name them."""
import ctypes
import re
import subprocess

import pytest

import yfm_amd
from conftest import ROOT
from yfm_amd import _lib, engine, smoothing

NAMES = ("yfm_tvl_smooth_batch", "yfm_tvl_smooth_batch_device")


def header():
    return (ROOT / "include" / "yfm.h").read_text()


def test_header_declares_the_entry_points():
    h = header()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    doc = h[h.index("The extended Kalman smoother of the TVλ model"):h.index("int yfm_tvl_smooth_batch(")]
    assert "EXTENSION" in doc and "no counterpart" in doc
    for word in ("linearised once", "nothing is re-linearised", "λ_t = 0.01 + exp(a_{4,t})", "filter.jl:38-46",
                 "quirk kept", "v_t = y_t − Z_t[:,1:3]·a_t[1:3]", "G_t = Z_t'Z_t", "u_t = Z_t'v_t",
                 "B_t = σ²I + G_t P_t", "s_t = B_t⁻¹u_t", "W_t = B_t⁻¹G_t", "L_t = Φ(I − P_t W_t)",
                 "r_{t−1} = s_t + L_t' r_t", "N_{t−1} = W_t + L_t' N_t L_t", "β̂_t = a_t + P_t r_{t−1}",
                 "V_t = P_t − P_t N_{t−1} P_t", "(I − P_{t+1} N_t) L_t P_t", "missing column", "n = 1 is valid",
                 "symmetric to the bit", "may be NULL", "no deferral list", "yfm_last_batch_grad_unavailable",
                 "det(σ²I + P_t G_t)", "128 MiB", "lane count", "only the parity rule is promised", "YFM_EUNSUPPORTED",
                 "B = 0 succeeds", "λ̂_t = 0.01 + exp("):
        assert word in doc, word


def test_lib_binds_them():
    t = _lib.SIGNATURES
    for n, twin in zip(NAMES, ("yfm_smooth_batch", "yfm_smooth_batch_device")):
        res, args = t[n]
        assert res is ctypes.c_int and args == t[twin][1], n
        decl = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\);", header()).group(1)
        twin_decl = re.search(r"\bint\s+" + twin + r"\s*\(([^;]*)\);", header()).group(1)
        assert len(decl.split(",")) == len(args), n
        assert re.sub(r"\s+", " ", decl) == re.sub(r"\s+", " ", twin_decl), n
    assert _lib.ABI_VERSION == 5


def test_library_exports_them():
    if not _lib.LIB_PATH.exists():
        pytest.skip("in-tree library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True,
                         text=True).stdout
    for n in NAMES:
        assert re.search(r"\bT " + n + r"$", out, re.M), n


def test_package_exports_the_host_mirror():
    for n in ("tvl_smooth", "tvl_smooth_device"):
        assert hasattr(engine.Engine, n), n
    for n in ("tvl_smooth_batch", "tvl_smooth_", "tvl_smoothed_yields"):
        assert n in yfm_amd.__all__ and hasattr(yfm_amd, n), n
    assert yfm_amd.tvl_smooth_batch is smoothing.tvl_smooth_batch


def test_refused_models_say_where_to_go():
    """The kinds the entry point refuses raise NotImplementedError before any device call; the fixed-loading smoother
    keeps refusing TVλ with the words "extended smoother"."""
    class M:
        def __init__(self, kind):
            self.kind = kind
    for kind, word in ((yfm_amd.KIND_DNS, "smooth"), (yfm_amd.KIND_GNS, "smooth"),
                       (yfm_amd.KIND_SD_NS, "nothing to smooth"), (yfm_amd.KIND_NNS, "nothing to smooth")):
        with pytest.raises(NotImplementedError, match=word):
            smoothing.tvl_smooth_batch(M(kind), None, None)
        with pytest.raises(NotImplementedError, match=word):
            engine.Engine._tvl_smooth_kinds(kind, "tvl_smooth")
    engine.Engine._tvl_smooth_kinds(yfm_amd.KIND_TVL, "tvl_smooth")
    with pytest.raises(NotImplementedError, match="extended smoother"):
        smoothing.smooth_batch(M(yfm_amd.KIND_TVL), None, None)
    with pytest.raises(NotImplementedError, match="extended smoother"):
        engine.Engine._smooth_kinds(yfm_amd.KIND_TVL, "smooth")


def test_julia_wrapper_and_documents_name_them():
    jl = (ROOT / "yieldfactormodels.jl_amd" / "julia" / "YFMAMD.jl").read_text()
    assert "LIB.yfm_tvl_smooth_batch(" in jl and "function tvl_smooth(" in jl
    assert "yfm_tvl_smooth_batch" in (ROOT / "INTEGRATION.md").read_text()
    design = (ROOT / "DESIGN.md").read_text()
    assert "### 3.13" in design and "yfm_tvl_smooth_batch" in design and "tvl_smooth_kernel" in design
    assert "tvl_smooth" in (ROOT / "README.md").read_text()
    assert (ROOT / "tools" / "bench_tvl_smooth.py").exists()
