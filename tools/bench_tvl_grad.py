"""Cost of the TVλ tangent gradient against the FP64 loglik launches that central differences would need.

    python tools/bench_tvl_grad.py [--B 16384] [--T 600] [--N 360] [--reps 7] [--warmup 2] [--out FILE]

Three legs, all under YFM_PREC_FP64 so that the value launch inside leg (a) is the same kernel as (b) and (c):
  (a) one yfm_tvl_loglik_grad_batch_device launch of B candidates (the value launch and the tangent kernel),
  (b) one yfm_loglik_batch_device launch of the same B candidates,
  (c) one yfm_loglik_batch_device launch of the 2P·B = 62·B candidates central differences cost — the yardstick:
      that kernel is not touched by the gradient work.
HIP events around each launch, `warmup` untimed launches, the median of `reps`, the legs alternating.  N = 360 is
the config-3 shape (maturities 1..360), N = 30 the estimator's (maturities_30).

Prints one JSON line (and writes it to --out).  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
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


def speed(eng, B, T, N, reps, warmup):
    mats = S.maturities_360() if N == 360 else S.maturities_30() if N == 30 else np.linspace(3, 360, N)
    eng.set_panel(S.simulate_panel(KIND_TVL, T, maturities=mats), mats)
    P = n_params(KIND_TVL)
    stream = torch.cuda.current_stream()
    Th = S.theta_batch(KIND_TVL, B, 0.02, seed=41, bad_frac=0.0)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, P), dtype=torch.float64, device="cuda")
    # the 2P points per candidate of central differences: the same θ repeated (the kernel's time does not depend on h)
    d_fd = d_th.repeat(2 * P, 1).contiguous()
    d_fd_out = torch.empty(d_fd.shape[0], dtype=torch.float64, device="cuda")
    grad = lambda: eng.tvl_loglik_grad_device(KIND_TVL, d_th.data_ptr(), P, B, d_ll.data_ptr(), d_g.data_ptr(),
                                              stream=stream.cuda_stream)
    fd = lambda: eng.loglik_device(KIND_TVL, d_fd.data_ptr(), P, d_fd.shape[0], d_fd_out.data_ptr(),
                                   stream=stream.cuda_stream)
    value = lambda: eng.loglik_device(KIND_TVL, d_th.data_ptr(), P, B, d_ll.data_ptr(), stream=stream.cuda_stream)
    for _ in range(warmup):
        grad(), value(), fd()
    torch.cuda.synchronize()
    t = {"grad": [], "fd": [], "value": []}
    for _ in range(reps):
        t["grad"].append(timed(grad, stream))
        t["value"].append(timed(value, stream))
        t["fd"].append(timed(fd, stream))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"B": B, "T": T, "N": len(mats), "grad_launch_ms": med["grad"], "loglik_B_launch_ms": med["value"],
            "loglik_62B_launch_ms": med["fd"], "grad_over_loglik_B": med["grad"] / med["value"],
            "grad_over_62B": med["grad"] / med["fd"], "grad_ms_spread": [min(t["grad"]), max(t["grad"])],
            "loglik_62B_ms_spread": [min(t["fd"]), max(t["fd"])],
            "finite_gradients": int(np.isfinite(d_g.cpu().numpy()).all(axis=1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--N", type=int, default=360)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    eng.precision = _lib.PREC_FP64
    res = {"speed": speed(eng, args.B, args.T, args.N, args.reps, args.warmup)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
