"""The SD-NS estimator on both paths, from the same start: the 240-window rolling re-estimation of
tools/bench_msed.py case (e) (the T = 600, N = 30 panel, expanding windows, every window started from θ₀) run once with
estimate_steps!'s default parameter groups (models.estimate_steps_batch: Nelder–Mead on A, B, ω and L-BFGS on δ, Φ) and
once with the L-BFGS estimate! on the full gradient (models.estimate_lbfgs_batch with T_use: one chain per window, in
lockstep, one yfm_lambda_loss_fullgrad_batch launch per round).

    python tools/bench_lambda_estimate.py [--windows 240] [--lbfgs-iterations 1000] [--out FILE]

Per path: wall seconds, loss reached (median, mean, and the number of windows where that path ends higher by more than
1e-6), objective evaluations and, for L-BFGS, rounds (launches) and status counts.  Prints one JSON line.  Not part of
bench.py.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))

from yfm_amd import KIND_SD_NS, create_model, estimate_lbfgs_batch, estimate_steps_batch, get_engine  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=240)
    ap.add_argument("--max-group-iters", type=int, default=10)
    ap.add_argument("--lbfgs-iterations", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mats = S.maturities_30()
    Y = S.simulate_panel(KIND_SD_NS, 600, maturities=mats)
    th0 = S.theta0_constrained(KIND_SD_NS)
    wins = np.arange(601 - args.windows, 601, dtype=np.int32)
    Th0 = np.asfortranarray(np.repeat(th0[:, None], len(wins), axis=1))
    torch.cuda.set_device(0)
    eng = get_engine(0)
    model, _ = create_model("SD-NS", mats, len(mats), 3)
    eng.set_panel(Y, mats)
    # warm up both paths
    estimate_steps_batch(model, Y, Th0[:, :2], T_use=wins[:2], max_group_iters=1, iterations=5)
    estimate_lbfgs_batch(model, Y, Th0[:, :2], space=1, T_use=wins[:2], iterations=2)
    t0 = time.perf_counter()
    gr = estimate_steps_batch(model, Y, Th0, T_use=wins, max_group_iters=args.max_group_iters)
    gr_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    lb = estimate_lbfgs_batch(model, Y, Th0, space=1, T_use=wins, iterations=args.lbfgs_iterations)
    lb_s = time.perf_counter() - t0
    ok = np.isfinite(gr["ll"]) & np.isfinite(lb["ll"])
    d = lb["ll"][ok] - gr["ll"][ok]
    out = {"metric": "SD-NS rolling re-estimation from θ₀, T ≤ 600, N = 30: estimate_steps! (default groups) against "
                     "estimate! (L-BFGS on the full gradient)",
           "windows": int(len(wins)),
           "groups": {"seconds": gr_s, "n_evals": int(gr["n_evals"]),
                      "evals_by_group": {k: int(v) for k, v in gr["evals_by_group"].items()},
                      "rounds_by_group": {k: int(v) for k, v in gr["rounds_by_group"].items()},
                      "ll_median": float(np.median(gr["ll"])), "ll_mean": float(np.mean(gr["ll"][ok])),
                      "max_group_iters": args.max_group_iters,
                      "status_counts": np.bincount(gr["status"], minlength=3).tolist()},
           "lbfgs": {"seconds": lb_s, "n_evals": int(lb["n_evals"]), "rounds": int(lb["rounds"]),
                     "ll_median": float(np.median(lb["ll"])), "ll_mean": float(np.mean(lb["ll"][ok])),
                     "iterations_limit": args.lbfgs_iterations, "iterations_median": float(np.median(lb["iterations"])),
                     "status_counts": np.bincount(lb["status"], minlength=4).tolist()},
           "windows_both_finite": int(ok.sum()),
           "lbfgs_higher_by_1e-6": int((d > 1e-6).sum()), "groups_higher_by_1e-6": int((d < -1e-6).sum()),
           "ll_difference_lbfgs_minus_groups": {"min": float(d.min()), "median": float(np.median(d)),
                                                "max": float(d.max())}}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
