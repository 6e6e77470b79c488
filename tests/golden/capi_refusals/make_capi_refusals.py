"""The refusals of libyfm_hip.so's batched entry points: the matrix of bad calls, and the generator of refusals.json.

    YFM_LIB=<the library to record> python tests/golden/capi_refusals/make_capi_refusals.py

Every host-pointer and device-pointer entry point of include/yfm.h that opens with (ctx, model_kind, param_space,
theta, P, B, T_use) is called through ctypes with one bad argument at a time, for one kind of each class and on a
context without a panel, with a 30 × 4 panel and with a 65 × 2 panel (above the 64 maturities of the DNS tangent kernel
and of the smoother).  Each call is one the library refuses in the checks at the top of the entry point, before it
enqueues anything: apart from the bad argument every call is valid (B = 1, θ = 0 in real buffers), and a call that the
entry point would serve is never made.  `run_matrix` returns {case id: (return code, yfm_last_error() text)};
tests/test_gpu_capi_refusals.py runs it on the tree's library and compares with the recorded file, which was written
from the library of the commit before the entry points were folded into one path per call family.
"""
from __future__ import annotations

import ctypes
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
FIXTURE = HERE / "refusals.json"

_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int)

# one kind of each class (include/yfm.h): DNS, TVλ, GNS5, SD-NS, NNS, the scalar score-driven NNS
KINDS = {"dns": 0, "tvl": 1, "gns5": 2, "sd_ns": 4, "nns": 16, "sd_nns": 32}
KALMAN, LAMBDA, NEURAL = {"dns", "tvl", "gns5"}, {"sd_ns"}, {"nns", "sd_nns"}
EVERY = KALMAN | LAMBDA | NEURAL

# family → (output arrays after the prefix, the kinds it serves); each has a `_device` twin that ends with the stream
FAMILIES = {
    "yfm_loglik_batch": (1, EVERY),
    "yfm_loglik_grad_batch": (2, {"dns"}),
    "yfm_tvl_loglik_grad_batch": (2, {"tvl"}),
    "yfm_loglik_scores_batch": (2, {"dns"}),
    "yfm_lambda_loss_grad_batch": (2, LAMBDA),
    "yfm_lambda_loss_fullgrad_batch": (2, LAMBDA),
    "yfm_neural_loss_grad_batch": (2, NEURAL),
    "yfm_neural_loss_fullgrad_batch": (2, NEURAL),
    "yfm_smooth_batch": (3, {"dns", "gns5"}),
    "yfm_tvl_smooth_batch": (3, {"tvl"}),
}
# host-pointer entry points without a twin → the kinds they serve
HOST_ONLY = {
    "yfm_filter_states": KALMAN,
    "yfm_predict": EVERY,
    "yfm_forecast": EVERY,
    "yfm_loss_array": EVERY,
    "yfm_loglik_info_batch": {"dns"},
    "yfm_estimate": KALMAN,
}
# the entry points that refuse a panel of more than 64 maturities for a kind they serve
N_LIMITED = ("yfm_loglik_grad_batch", "yfm_loglik_scores_batch", "yfm_loglik_info_batch", "yfm_smooth_batch")
PANELS = {"N30_T4": (30, 4), "N65_T2": (65, 2)}
BUF = 16384  # doubles per buffer: more than any output of a B = 1 call on these panels


def entries():
    for name, (_, serves) in FAMILIES.items():
        yield name, serves
        yield name + "_device", serves
    yield from HOST_ONLY.items()


class Buffers:
    """Real memory behind every pointer argument, so that a call the library failed to refuse would still be a valid
    one: zeroed host arrays, and zeroed device arrays for the `_device` entry points."""

    def __init__(self):
        import torch
        self.host = [np.zeros(BUF) for _ in range(7)]
        self.host_int = np.zeros(BUF, dtype=np.int32)
        self.tuse = np.ones(1, dtype=np.int32)
        self.dev = [torch.zeros(BUF, dtype=torch.float64, device="cuda") for _ in range(5)]
        torch.cuda.synchronize()


def call(lib, ctx, buf, name, kind, P, *, space=0, B=1, null_theta=False, T_use=None, horizon=1, K=1, lags=0,
         matrices=True):
    """One call of the entry point `name`; returns (return code, error text)."""
    if name.endswith("_device"):
        n = FAMILIES[name[:-len("_device")]][0]
        ptr = [ctypes.c_void_p(t.data_ptr()) for t in buf.dev]
        args = [ctx, kind, space, None if null_theta else ptr[0], P, B, None] + ptr[1:1 + n] + [None]
    else:
        h = [a.ctypes.data_as(_D) for a in buf.host]
        tu = None
        if T_use is not None:
            buf.tuse[0] = T_use
            tu = buf.tuse.ctypes.data_as(_I)
        args = [ctx, kind, space, None if null_theta else h[0], P, B, tu]
        if name in FAMILIES:
            args += h[1:1 + FAMILIES[name][0]]
        elif name == "yfm_filter_states":
            args += h[1:4]
        elif name == "yfm_predict":
            args += [horizon] + h[1:6]
        elif name == "yfm_forecast":
            args += [horizon, h[1]]
        elif name == "yfm_loss_array":
            args += [K, h[1]]
        elif name == "yfm_loglik_info_batch":
            args += [lags, 0.0, h[1], h[2], h[3] if matrices else None, h[4] if matrices else None]
        elif name == "yfm_estimate":
            args += [1, 1e-6, 1, 1e-8] + h[1:5] + [buf.host_int.ctypes.data_as(_I), ctypes.byref(ctypes.c_longlong(0))]
        else:
            raise KeyError(name)
    rc = getattr(lib, name)(*args)
    return int(rc), lib.yfm_last_error().decode("utf-8") if rc != 0 else ""


def bad_calls(name, serves, kname, panel):
    """(case, keyword arguments of `call`) for the entry point and kind on `panel` (None: no panel set)."""
    if panel is None:
        yield "no_panel", {}
        return
    T = PANELS[panel][1]
    yield "wrong_P", {"dP": 1}
    yield "B_negative", {"B": -1}
    yield "unknown_param_space", {"space": 7}
    yield "null_theta", {"null_theta": True}
    if not name.endswith("_device"):
        yield "T_use_zero", {"T_use": 0}
        yield "T_use_past_T", {"T_use": T + 1}
    if kname not in serves:
        yield "kind_refused", {}
    elif PANELS[panel][0] > 64 and name.replace("_device", "") in N_LIMITED:
        yield "N_above_limit", {}
    if name in ("yfm_predict", "yfm_forecast"):
        yield "horizon_zero", {"horizon": 0}
    if name == "yfm_loss_array":
        yield "K_zero", {"K": 0}
    if name == "yfm_loglik_info_batch":
        yield "lags_negative", {"lags": -1}
        yield "both_matrices_null", {"matrices": False}


def run_matrix(lib) -> dict:
    """{"<panel>/<entry point>/<kind>/<case>": (return code, error text)} on a context of its own."""
    buf = Buffers()
    ctx = ctypes.c_void_p(lib.yfm_create(0))
    assert ctx, lib.yfm_last_error()
    out = {}
    try:
        for panel in (None, *PANELS):
            if panel is not None:
                N, T = PANELS[panel]
                Y = np.asfortranarray(0.05 + 0.001 * np.arange(N * T, dtype=np.float64).reshape(N, T))
                mats = np.arange(1.0, N + 1.0)
                rc = lib.yfm_set_panel(ctx, Y.ctypes.data_as(_D), N, T, mats.ctypes.data_as(_D))
                assert rc == 0, lib.yfm_last_error()
            for name, serves in entries():
                for kname, kind in KINDS.items():
                    P = lib.yfm_param_count(kind)
                    for case, kw in bad_calls(name, serves, kname, panel):
                        kw = dict(kw)
                        dP = kw.pop("dP", 0)
                        out[f"{panel or 'no_panel'}/{name}/{kname}/{case}"] = call(lib, ctx, buf, name, kind, P + dP,
                                                                                  **kw)
    finally:
        lib.yfm_destroy(ctx)
    return out


def main() -> int:
    root = HERE.parents[2]
    sys.path.insert(0, str(root / "yieldfactormodels.jl_amd"))
    import torch  # noqa: F401  (the HIP runtime the library binds to)
    from yfm_amd import _lib
    got = run_matrix(_lib.load())
    served = [k for k, (rc, _) in got.items() if rc == 0]
    if served:
        print("not refused:", *served, sep="\n  ", file=sys.stderr)
        return 1
    FIXTURE.write_text(dumps(got), encoding="utf-8")
    assert load() == got
    print(f"{len(got)} refusals -> {FIXTURE}")
    return 0


def dumps(got: dict) -> str:
    """The file's text: the distinct texts once, then one line per panel and entry point holding, per case, the
    (return code, index of the text) of each kind in KINDS' order (null: the case is not made for that kind)."""
    texts = sorted({t for _, t in got.values()})
    rows = {}
    for key, (rc, t) in got.items():
        panel, name, kname, case = key.split("/")
        row = rows.setdefault(f"{panel}/{name}", {}).setdefault(case, [None] * len(KINDS))
        row[list(KINDS).index(kname)] = [rc, texts.index(t)]
    js = lambda o: json.dumps(o, ensure_ascii=False, separators=(",", ":"))  # noqa: E731
    return ('{"texts":[\n' + ",\n".join(js(t) for t in texts) + '\n],"cases":{\n'
            + ",\n".join(f"{js(k)}:{js(v)}" for k, v in rows.items()) + "\n}}\n")


def load() -> dict:
    """The recorded file in run_matrix's form."""
    rec = json.loads(FIXTURE.read_text(encoding="utf-8"))
    return {f"{key}/{kname}/{case}": (pair[0], rec["texts"][pair[1]])
            for key, cases in rec["cases"].items() for case, row in cases.items()
            for kname, pair in zip(KINDS, row) if pair is not None}


if __name__ == "__main__":
    sys.exit(main())
