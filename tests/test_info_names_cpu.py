"""The score and information entry points' public names: include/yfm.h declares the three entry points and the default
step and says that they are an extension, yfm_amd._lib binds them with matching argument lists, the ABI version stays 5
(the change is additive), the library exports them, and the package exports the host mirror."""
import ctypes
import re
import subprocess

import pytest

import yfm_amd
from conftest import ROOT
from yfm_amd import _lib, engine, inference

NAMES = ("yfm_loglik_scores_batch", "yfm_loglik_scores_batch_device", "yfm_loglik_info_batch")


def header():
    return (ROOT / "include" / "yfm.h").read_text()


def test_header_declares_the_entry_points():
    h = header()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    doc = h[h.index("Score series, information matrices"):h.index("int yfm_loglik_scores_batch(")]
    # an extension, said so instead of citing a reference line for the feature; the definitions of the issue
    assert "EXTENSION" in doc and "no counterpart" in doc
    for word in ("Bartlett", "fourth-order central differences", "realised steps", "yfm_last_batch_grad_unavailable",
                 "YFM_EUNSUPPORTED", "deferral list", "128 MiB", "exactly 0.0"):
        assert word in doc, word


def test_default_step_agrees_between_header_binding_and_design():
    m = re.search(r"#define\s+YFM_INFO_DEFAULT_STEP\s+(\S+)", header())
    assert m and float(m.group(1)) == _lib.INFO_DEFAULT_STEP
    design = (ROOT / "DESIGN.md").read_text()
    sec = design[design.index("### 3.11"):]
    assert f"h = {_lib.INFO_DEFAULT_STEP:g}" in sec


def test_lib_binds_them():
    t = _lib.SIGNATURES
    assert t["yfm_loglik_scores_batch"] == t["yfm_loglik_grad_batch"]
    assert t["yfm_loglik_scores_batch_device"] == t["yfm_loglik_grad_batch_device"]
    res, args = t["yfm_loglik_info_batch"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[7] is ctypes.c_int and args[8] is ctypes.c_double  # lags, step
    assert _lib.ABI_VERSION == 5
    # the header's argument counts
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
    for n in ("loglik_scores", "loglik_scores_device", "loglik_info"):
        assert hasattr(engine.Engine, n), n
    for n in ("covariance", "standard_errors_batch", "standard_errors_", "inference"):
        assert n in yfm_amd.__all__ and hasattr(yfm_amd, n), n
    assert yfm_amd.covariance is inference.covariance
    assert inference.COV_KINDS == ("hessian", "opg", "sandwich")
