"""Cost of the TVλ extended smoother's backward sweep beside its forward launch.

    python tools/bench_tvl_smooth.py [--N 30 360] [--B 240 1400] [--T 600] [--reps 7] [--warmup 2]

At T columns, for every N (30: the 30-maturity grid; 360: months 1 … 360), every B (240 and one full chunk: 1,400
candidates at T = 600) and both precisions of the forward pass, three legs on one stream (HIP events, `warmup` untimed
rounds, the median of `reps` with min–max, the legs alternating):
    forward  the TVλ forward trajectory launch alone: yfm_tvl_smooth_batch_device with YFM_SMOOTH_SWEEP=0 in the
             environment (a measurement switch: the sweep is left out, nothing is written)
    smooth   yfm_tvl_smooth_batch_device — the trajectory launch and tvl_smooth_kernel
    value    yfm_loglik_batch_device — the value-only loglik launch
and sweep_ms = smooth − forward, smooth_over_forward = smooth / forward.  Prints one JSON line.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

from yfm_amd import KIND_TVL, Engine, _lib, n_params  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def timed(run, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def measure(eng, N, B, T, mode, reps, warmup):
    mats = S.maturities_30() if N == 30 else S.maturities_360()[:N]
    eng.set_panel(S.simulate_panel(KIND_TVL, T, maturities=mats), mats)
    eng.precision = mode
    P, M = n_params(KIND_TVL), 4
    stream = torch.cuda.current_stream()
    Th = S.theta_batch(KIND_TVL, B, scale=0.02, seed=41, bad_frac=0.0)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_b = torch.empty(B * T * M, dtype=torch.float64, device="cuda")
    d_V = torch.empty(B * T * M * M, dtype=torch.float64, device="cuda")
    d_C = torch.empty(B * (T - 1) * M * M, dtype=torch.float64, device="cuda")

    def smooth():
        eng.tvl_smooth_device(KIND_TVL, d_th.data_ptr(), P, B, d_b.data_ptr(), d_V.data_ptr(), d_C.data_ptr(),
                              stream=stream.cuda_stream)

    def forward():
        os.environ["YFM_SMOOTH_SWEEP"] = "0"
        try:
            smooth()
        finally:
            del os.environ["YFM_SMOOTH_SWEEP"]

    legs = {
        "forward": forward,
        "smooth": smooth,
        "value": lambda: eng.loglik_device(KIND_TVL, d_th.data_ptr(), P, B, d_ll.data_ptr(),
                                           stream=stream.cuda_stream),
    }
    for _ in range(warmup):
        for run in legs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, run in legs.items():
            t[k].append(timed(run, stream))
    torch.cuda.synchronize()
    res = {"N": len(mats), "B": B, "T": T, "precision": "certified" if mode == _lib.PREC_CERTIFIED else "fp64",
           **{k: summary(v) for k, v in t.items()}}
    res["sweep_ms"] = res["smooth"]["median_ms"] - res["forward"]["median_ms"]
    res["smooth_over_forward"] = res["smooth"]["median_ms"] / res["forward"]["median_ms"]
    smooth()
    torch.cuda.synchronize()
    res["unavailable"] = eng.last_grad_unavailable()
    res["finite_candidates"] = int(torch.isfinite(d_b.view(B, -1)[:, 0]).sum().item())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[30, 360])
    ap.add_argument("--B", type=int, nargs="+", default=[240, 1400])
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    old = eng.precision
    out = []
    try:
        for N in args.N:
            for B in args.B:
                for mode in (_lib.PREC_CERTIFIED, _lib.PREC_FP64):
                    out.append(measure(eng, N, B, args.T, mode, args.reps, args.warmup))
    finally:
        eng.precision = old
    print(json.dumps({"tvl_smooth": out}), flush=True)


if __name__ == "__main__":
    main()
