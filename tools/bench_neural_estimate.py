"""The 1SD-NNS estimator on both paths, from the same start: the 240-window rolling re-estimation of
tools/bench_msedn.py case (f) (the T = 600, N = 30 panel, expanding windows, every window started from θ₀) run with the
L-BFGS estimate! on the full gradient (models.estimate_neural_lbfgs_batch with T_use: one chain per window, in
lockstep, one yfm_neural_loss_fullgrad_batch launch per round) and — unless --skip-groups — once with estimate_steps!'s
default parameter groups (models.estimate_neural_steps_batch: Nelder–Mead on A, B, ω and L-BFGS on δ, Φ; about 205 s).

    python tools/bench_neural_estimate.py [--windows 240] [--lbfgs-iterations 1000] [--skip-groups] [--searched-start]
                                          [--out FILE]

--searched-start starts the L-BFGS chains from try_initializations_batch's winners (the 256-trial grid the grouped path
searches before it descends) instead of θ₀.

Per path: wall seconds, loss reached (median, mean, and the number of windows where that path ends higher by more than
1e-6), objective evaluations and, for L-BFGS, rounds (launches) and status counts.  Prints one JSON line, the L-BFGS
path's first (the grouped path's line follows when it has run).  Not part of bench.py.
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

from yfm_amd import create_neural_model, estimate_neural_lbfgs_batch, estimate_neural_steps_batch, get_engine  # noqa: E402
from yfm_amd import params as P  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402
from yfm_amd import try_initializations_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=240)
    ap.add_argument("--max-group-iters", type=int, default=10)
    ap.add_argument("--lbfgs-iterations", type=int, default=1000)
    ap.add_argument("--skip-groups", action="store_true")
    ap.add_argument("--searched-start", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mats = S.maturities_30()
    kind = P.neural_kind("scalar")
    Y = S.simulate_panel(P.KIND_NNS, 600, maturities=mats)  # bench_msedn.py's panel
    th0 = S.theta0_constrained(kind)
    wins = np.linspace(600 - args.windows + 1, 600, args.windows).astype(np.int32)
    Th0 = np.asfortranarray(np.repeat(th0[:, None], len(wins), axis=1))
    torch.cuda.set_device(0)
    eng = get_engine(0)
    model, _ = create_neural_model("1SD-NNS", mats, len(mats), 3)
    eng.set_panel(Y, mats)
    estimate_neural_lbfgs_batch(model, Y, Th0[:, :2], space=1, T_use=wins[:2], iterations=2)  # warm-up
    t0 = time.perf_counter()
    start = try_initializations_batch(Th0, model, Y, T_use=wins)[0] if args.searched_start else Th0
    lb = estimate_neural_lbfgs_batch(model, Y, start, space=1, T_use=wins, iterations=args.lbfgs_iterations)
    lb_s = time.perf_counter() - t0
    out = {"metric": "1SD-NNS rolling re-estimation from θ₀, T ≤ 600, N = 30: estimate! (L-BFGS on the full gradient) "
                     "against estimate_steps! (default groups)",
           "windows": int(len(wins)), "lbfgs_start": "try_initializations" if args.searched_start else "theta0",
           "lbfgs": {"seconds": lb_s, "n_evals": int(lb["n_evals"]), "rounds": int(lb["rounds"]),
                     "ll_start_mean": float(np.mean(lb["ll0"])),
                     "ll_median": float(np.median(lb["ll"])), "ll_mean": float(np.mean(lb["ll"])),
                     "iterations_limit": args.lbfgs_iterations, "iterations_median": float(np.median(lb["iterations"])),
                     "status_counts": np.bincount(lb["status"], minlength=4).tolist()}}
    print(json.dumps(out), flush=True)
    if not args.skip_groups:
        estimate_neural_steps_batch(model, Y, Th0[:, :2], T_use=wins[:2], max_group_iters=1, iterations=5)
        t0 = time.perf_counter()
        gr = estimate_neural_steps_batch(model, Y, Th0, T_use=wins, max_group_iters=args.max_group_iters)
        gr_s = time.perf_counter() - t0
        ok = np.isfinite(gr["ll"]) & np.isfinite(lb["ll"])
        d = lb["ll"][ok] - gr["ll"][ok]
        out["groups"] = {"seconds": gr_s, "n_evals": int(gr["n_evals"]),
                         "evals_by_group": {k: int(v) for k, v in gr["evals_by_group"].items()},
                         "rounds_by_group": {k: int(v) for k, v in gr["rounds_by_group"].items()},
                         "ll_median": float(np.median(gr["ll"])), "ll_mean": float(np.mean(gr["ll"][ok])),
                         "max_group_iters": args.max_group_iters,
                         "status_counts": np.bincount(gr["status"], minlength=3).tolist()}
        out.update({"windows_both_finite": int(ok.sum()), "lbfgs_higher_by_1e-6": int((d > 1e-6).sum()),
                    "groups_higher_by_1e-6": int((d < -1e-6).sum()),
                    "ll_difference_lbfgs_minus_groups": {"min": float(d.min()), "median": float(np.median(d)),
                                                         "max": float(d.max())}})
        print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
