"""Cost of the DNS score series, OPG matrix and Hessian beside the gradient launch.

    python tools/bench_info.py [--B 240 4080] [--T 600] [--reps 7] [--warmup 2] [--lags 0]

At T columns and N = 30, per batch size B:
  launches (HIP events on one stream, `warmup` untimed rounds, the median of `reps` with min–max, alternating):
    grad    yfm_loglik_grad_batch_device   — the loglik launch and dns_grad_kernel
    scores  yfm_loglik_scores_batch_device — the loglik launch and dns_score_kernel
    value   yfm_loglik_batch_device        — the loglik launch alone
  host-pointer calls (synchronous; wall clock, the same warm-ups and repetitions, alternating):
    grad_call   yfm_loglik_grad_batch
    info_call   yfm_loglik_info_batch with both halves (4P perturbed points per candidate, chunked), and with the
                OPG half alone (opg_call) and the Hessian half alone (hess_call)
and the ratios to the gradient's.  The C ABI has no entry that runs opg_kernel alone, so the OPG half's own cost is
derived: opg_extra = opg_call − grad_call − (scores − value), i.e. what the call adds to a gradient call and a score
kernel — opg_kernel per chunk, the chunking and J's copy to the host.  Prints one JSON line.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

from yfm_amd import KIND_DNS, Engine, n_params  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def timed(run, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(run):
    t0 = time.perf_counter()
    run()
    return 1e3 * (time.perf_counter() - t0)


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def measure(eng, B, T, reps, warmup, lags):
    mats = S.maturities_30()
    eng.set_panel(S.simulate_panel(KIND_DNS, T, maturities=mats), mats)
    P = n_params(KIND_DNS)
    stream = torch.cuda.current_stream()
    Th = S.theta_batch(KIND_DNS, B, seed=41, bad_frac=0.0)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, P), dtype=torch.float64, device="cuda")
    d_s = torch.empty((B, T - 1, P), dtype=torch.float64, device="cuda")
    launches = {
        "grad": lambda: eng.loglik_grad_device(KIND_DNS, d_th.data_ptr(), P, B, d_ll.data_ptr(), d_g.data_ptr(),
                                               stream=stream.cuda_stream),
        "scores": lambda: eng.loglik_scores_device(KIND_DNS, d_th.data_ptr(), P, B, d_ll.data_ptr(), d_s.data_ptr(),
                                                   stream=stream.cuda_stream),
        "value": lambda: eng.loglik_device(KIND_DNS, d_th.data_ptr(), P, B, d_ll.data_ptr(),
                                           stream=stream.cuda_stream),
    }
    calls = {
        "grad_call": lambda: eng.loglik_grad(KIND_DNS, Th),
        "opg_call": lambda: eng.loglik_info(KIND_DNS, Th, lags=lags, hessian=False),
        "hess_call": lambda: eng.loglik_info(KIND_DNS, Th, opg=False),
        "info_call": lambda: eng.loglik_info(KIND_DNS, Th, lags=lags),
    }
    for _ in range(warmup):
        for run in launches.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in (*launches, *calls)}
    for _ in range(reps):
        for k, run in launches.items():
            t[k].append(timed(run, stream))
    torch.cuda.synchronize()
    for _ in range(warmup):
        for run in calls.values():
            run()
    for _ in range(reps):
        for k, run in calls.items():
            t[k].append(wall(run))
    res = {"B": B, "T": T, "N": len(mats), "lags": lags, **{k: summary(v) for k, v in t.items()}}
    g, gc = res["grad"]["median_ms"], res["grad_call"]["median_ms"]
    res["scores_over_grad"] = res["scores"]["median_ms"] / g
    res["opg_extra_ms"] = (res["opg_call"]["median_ms"] - gc
                           - (res["scores"]["median_ms"] - res["value"]["median_ms"]))
    res["opg_extra_over_grad"] = res["opg_extra_ms"] / g
    for k in ("opg_call", "hess_call", "info_call"):
        res[f"{k}_over_grad_call"] = res[k]["median_ms"] / gc
    r = eng.loglik_info(KIND_DNS, Th, lags=lags)
    res["finite_hessians"] = int(np.isfinite(r["hess"]).all(axis=(0, 1)).sum())
    res["finite_opg"] = int(np.isfinite(r["opg"]).all(axis=(0, 1)).sum())
    res["unavailable"] = eng.last_grad_unavailable()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[240, 4080])
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lags", type=int, default=0)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    print(json.dumps({"info": [measure(eng, B, args.T, args.reps, args.warmup, args.lags) for B in args.B]}),
          flush=True)


if __name__ == "__main__":
    main()
