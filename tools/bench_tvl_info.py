"""Cost of the TVλ score series, OPG matrix and Hessian beside the TVλ gradient launch (tools/bench_info.py's method).

    python tools/bench_tvl_info.py [--B 240 4080] [--N 30 360] [--T 600] [--reps 7] [--warmup 2] [--lags 0]
                                   [--hess-max-B 4080] [--hess-reps 7] [--hess-warmup 2]

At T columns, per maturity count N and batch size B:
  launches (HIP events on one stream, `warmup` untimed rounds, the median of `reps` with min–max, alternating):
    grad    yfm_tvl_loglik_grad_batch_device   — the loglik launch and tvl_grad_kernel (the baseline)
    scores  yfm_tvl_loglik_scores_batch_device — the loglik launch and tvl_score_kernel
    value   yfm_loglik_batch_device            — the loglik launch alone
  host-pointer calls (synchronous; wall clock, the same warm-ups and repetitions, alternating):
    grad_call   yfm_tvl_loglik_grad_batch
    opg_call    yfm_tvl_loglik_info_batch with the OPG half alone
    hess_call   … with the Hessian half alone (124 perturbed points per candidate, chunked)
    info_call   … with both halves
and the ratios to the gradient's.  The Hessian half evaluates 124·B candidates: batches above --hess-max-B skip
hess_call and info_call (reported as null), and those two take their own --hess-reps / --hess-warmup.
Prints one JSON line per (N, B).  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from bench_info import summary, timed, wall  # noqa: E402
from yfm_amd import KIND_TVL, Engine, n_params  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def measure(eng, N, B, T, args):
    mats = S.maturities_30() if N == 30 else (S.maturities_360() if N == 360 else np.linspace(3.0, 360.0, N))
    eng.set_panel(S.simulate_panel(KIND_TVL, T, maturities=mats), mats)
    P = n_params(KIND_TVL)
    stream = torch.cuda.current_stream()
    Th = S.theta_batch(KIND_TVL, B, 0.02, seed=41, bad_frac=0.0)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, P), dtype=torch.float64, device="cuda")
    d_s = torch.empty((B, T - 1, P), dtype=torch.float64, device="cuda")
    launches = {
        "grad": lambda: eng.tvl_loglik_grad_device(KIND_TVL, d_th.data_ptr(), P, B, d_ll.data_ptr(), d_g.data_ptr(),
                                                   stream=stream.cuda_stream),
        "scores": lambda: eng.tvl_loglik_scores_device(KIND_TVL, d_th.data_ptr(), P, B, d_ll.data_ptr(),
                                                       d_s.data_ptr(), stream=stream.cuda_stream),
        "value": lambda: eng.loglik_device(KIND_TVL, d_th.data_ptr(), P, B, d_ll.data_ptr(),
                                           stream=stream.cuda_stream),
    }
    calls = {
        "grad_call": lambda: eng.tvl_loglik_grad(KIND_TVL, Th),
        "opg_call": lambda: eng.tvl_loglik_info(KIND_TVL, Th, lags=args.lags, hessian=False),
    }
    hess = {} if B > args.hess_max_B else {
        "hess_call": lambda: eng.tvl_loglik_info(KIND_TVL, Th, opg=False),
        "info_call": lambda: eng.tvl_loglik_info(KIND_TVL, Th, lags=args.lags),
    }
    for _ in range(args.warmup):
        for run in launches.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in (*launches, *calls, *hess)}
    for _ in range(args.reps):
        for k, run in launches.items():
            t[k].append(timed(run, stream))
    torch.cuda.synchronize()
    for group, warmup, reps in ((calls, args.warmup, args.reps), (hess, args.hess_warmup, args.hess_reps)):
        for _ in range(warmup):
            for run in group.values():
                run()
        for _ in range(reps):
            for k, run in group.items():
                t[k].append(wall(run))
    res = {"B": B, "T": T, "N": len(mats), "lags": args.lags, "precision": int(eng.lib.yfm_get_precision(eng.ctx)),
           **{k: summary(v) for k, v in t.items()}}
    g, gc = res["grad"]["median_ms"], res["grad_call"]["median_ms"]
    res["scores_over_grad"] = res["scores"]["median_ms"] / g
    res["score_kernel_over_grad_kernel"] = ((res["scores"]["median_ms"] - res["value"]["median_ms"])
                                            / (g - res["value"]["median_ms"]))
    for k in ("opg_call", "hess_call", "info_call"):
        res[f"{k}_over_grad_call"] = res[k]["median_ms"] / gc if k in res else None
    r = eng.tvl_loglik_info(KIND_TVL, Th, lags=args.lags, hessian=False)
    res["finite_opg"] = int(np.isfinite(r["opg"]).all(axis=(0, 1)).sum())
    res["unavailable"] = eng.last_grad_unavailable()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[240, 4080])
    ap.add_argument("--N", type=int, nargs="+", default=[30, 360])
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lags", type=int, default=0)
    ap.add_argument("--hess-max-B", type=int, default=4080)
    ap.add_argument("--hess-reps", type=int, default=7)
    ap.add_argument("--hess-warmup", type=int, default=2)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    for N in args.N:
        for B in args.B:
            print(json.dumps({"tvl_info": measure(eng, N, B, args.T, args)}), flush=True)


if __name__ == "__main__":
    main()
