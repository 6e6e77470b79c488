"""The TVλ gradient's public names: include/yfm.h declares the two entry points, yfm_amd._lib binds them with the
argument lists of the DNS pair, and the ABI version stays 5 (the change is additive)."""
import re

from conftest import ROOT
from yfm_amd import _lib

NAMES = ("yfm_tvl_loglik_grad_batch", "yfm_tvl_loglik_grad_batch_device")


def test_header_declares_the_entry_points():
    h = (ROOT / "include" / "yfm.h").read_text()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
    assert re.search(r"#define\s+YFM_ABI_VERSION\s+5\b", h)
    for ref in ("optimization.jl:367", "optimization.jl:10-23", "filter.jl:12-80"):
        assert ref in h[h.index("The TVλ log-likelihood WITH its gradient"):h.index("int yfm_tvl_loglik_grad_batch(")]


def test_lib_binds_them_like_the_dns_pair():
    sig = _lib._SIGNATURES if hasattr(_lib, "_SIGNATURES") else None
    table = sig if sig is not None else next(v for v in vars(_lib).values()
                                             if isinstance(v, dict) and "yfm_loglik_grad_batch" in v)
    assert table["yfm_tvl_loglik_grad_batch"] == table["yfm_loglik_grad_batch"]
    assert table["yfm_tvl_loglik_grad_batch_device"] == table["yfm_loglik_grad_batch_device"]
    assert _lib.ABI_VERSION == 5


def test_engine_and_models_expose_the_feature():
    import inspect

    from yfm_amd import engine, models
    assert hasattr(engine.Engine, "tvl_loglik_grad") and hasattr(engine.Engine, "tvl_loglik_grad_device")
    assert "T_use" in inspect.signature(models.estimate_lbfgs_batch).parameters
