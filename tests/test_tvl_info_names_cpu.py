"""The TVλ score and information entry points' public names: include/yfm.h declares the three entry points and their
default step and says that they are an extension, yfm_amd._lib binds them with their DNS namesakes' argument lists, the
ABI version stays 5 (the change is additive), the library exports them, the package exports the host mirror, and the
DNS names keep refusing TVλ."""
import re
import subprocess

import numpy as np
import pytest

import yfm_amd
from conftest import ROOT
from yfm_amd import KIND_DNS, KIND_TVL, _lib, engine, inference, models
from yfm_amd import synthetic as S

NAMES = ("yfm_tvl_loglik_scores_batch", "yfm_tvl_loglik_scores_batch_device", "yfm_tvl_loglik_info_batch")
DNS_NAMES = ("yfm_loglik_scores_batch", "yfm_loglik_scores_batch_device", "yfm_loglik_info_batch")


def header():
    return (ROOT / "include" / "yfm.h").read_text()


def test_header_declares_the_entry_points():
    h = header()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    doc = h[h.index("The same three calls for the TVλ model"):h.index("int yfm_tvl_loglik_scores_batch(")]
    assert "EXTENSION" in doc and "extension" in h
    for word in ("Bartlett", "realised", "yfm_last_batch_grad_unavailable", "YFM_EUNSUPPORTED", "128 MiB",
                 "exactly 0.0", "124", "YFM_ABI_VERSION stays 5", "YFM_TVL_INFO_DEFAULT_STEP"):
        assert word in doc, word


def test_default_step_agrees_between_header_binding_and_design():
    m = re.search(r"#define\s+YFM_TVL_INFO_DEFAULT_STEP\s+(\S+)", header())
    assert m and float(m.group(1)) == _lib.TVL_INFO_DEFAULT_STEP
    design = (ROOT / "DESIGN.md").read_text()
    sec = design[design.index("### 3.15"):]
    assert f"h = {_lib.TVL_INFO_DEFAULT_STEP:g}" in sec


def test_lib_binds_them_with_the_dns_argument_lists():
    t = _lib.SIGNATURES
    for n, d in zip(NAMES, DNS_NAMES):
        assert t[n] == t[d], n
        decl = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\);", header()).group(1)
        assert len(decl.split(",")) == len(t[n][1]), n
    assert _lib.ABI_VERSION == 5


def test_library_exports_them():
    if not _lib.LIB_PATH.exists():
        pytest.skip("in-tree library not built")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True,
                         text=True).stdout
    for n in NAMES:
        assert re.search(r"\bT " + n + r"$", out, re.M), n


def test_package_exports_the_host_mirror():
    for n in ("tvl_loglik_scores", "tvl_loglik_scores_device", "tvl_loglik_info"):
        assert hasattr(engine.Engine, n), n
    for n in ("tvl_standard_errors_batch", "tvl_standard_errors_"):
        assert n in yfm_amd.__all__ and hasattr(yfm_amd, n) and hasattr(inference, n), n


def test_the_old_names_still_refuse_tvl(monkeypatch):
    monkeypatch.setattr(models, "_engine", lambda model, data: pytest.fail("no launch for a refused kind"))
    tvl, _ = models.create_model("TVλ", S.maturities_30(), 30, 3)
    assert tvl.kind == KIND_TVL
    with pytest.raises(NotImplementedError, match="DNS"):
        inference.standard_errors_batch(tvl, np.zeros((30, 8)), S.theta0(KIND_TVL))
    eng = object.__new__(engine.Engine)  # no context: the refusal comes before any call into the library
    for call in (eng.loglik_scores, eng.loglik_info):
        with pytest.raises(NotImplementedError, match="DNS"):
            call(KIND_TVL, S.theta0(KIND_TVL))
    with pytest.raises(NotImplementedError, match="DNS"):
        eng.loglik_scores_device(KIND_TVL, 0, 1, 1, 0, 0)
    # … and the new ones refuse DNS the same way
    for call in (eng.tvl_loglik_scores, eng.tvl_loglik_info):
        with pytest.raises(NotImplementedError, match="TVλ"):
            call(KIND_DNS, S.theta0(KIND_DNS))
