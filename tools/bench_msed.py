"""Cost of the batched loss of the static and score-driven λ models (csrc/yfm_msed.hip).

    python tools/bench_msed.py [--T 600] [--reps 7] [--warmup 2] [--kinds 3,4,5,6,8] [--cases abcdef]

Three cases on the N = 30 grid, one yfm_loglik_batch_device launch each, HIP events around the launch, `warmup`
untimed launches, the median of `reps` with min–max:
  (a) the try_initializations grid of one window: the start and its 30 trials, 31 candidates;
  (b) the rolling driver's grid: 240 T_use windows × 31 candidates = 7,440;
  (c) 65,536 candidates (SD-NS only unless --all-kinds), T = 600.
Two cases for the estimation of these models, SD-NS only:
  (d) one loss-and-gradient launch (yfm_lambda_loss_grad_batch_device) against one loss launch at B = 31 and
      B = 7,440, timed the same way, with the ratio of the medians — the gradient kernel shares the loss kernel's
      passes;
  (e) the 240-window rolling re-estimation with the default parameter groups (models.estimate_steps_batch): wall
      clock, and evaluations and rounds split by group.
One case for the full gradient, every kind:
  (f) one loss-and-full-gradient launch (yfm_lambda_loss_fullgrad_batch_device, all P rows) beside one loss launch and
      one loss-and-δ/Φ-gradient launch at the shapes of (a) — and, SD-NS, at B = 7,440 —, the three alternating within
      every repetition, with the
      ratios of the medians to the loss launch.
For scale: the Float64 NumPy restatement (tests/msed_reference.py) on (a), wall clock, and the project's own
yfm_loglik_batch_device for DNS at the same B.  Prints one JSON line.  Not part of bench.py.
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
sys.path.insert(0, str(ROOT / "tests"))

import msed_reference as R  # noqa: E402
from yfm_amd import KIND_DNS, KIND_SD_NS, Engine, n_params  # noqa: E402
from yfm_amd import models as M  # noqa: E402
from yfm_amd import params as P  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def timed(run, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def launch_stats(eng, kind, Th, space, tu, reps, warmup):
    stream = torch.cuda.current_stream()
    B = Th.shape[1]
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_tu = None if tu is None else torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
    d_out = torch.empty(B, dtype=torch.float64, device="cuda")
    run = lambda: eng.loglik_device(kind, d_th.data_ptr(), Th.shape[0], B, d_out.data_ptr(), space=space,
                                    d_T_use=None if d_tu is None else d_tu.data_ptr(), stream=stream.cuda_stream)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t = [timed(run, stream) for _ in range(reps)]
    out = d_out.cpu().numpy()
    return {"B": B, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t),
            "finite": int(np.isfinite(out).sum())}


def grad_launch_stats(eng, kind, Th, space, tu, reps, warmup):
    """launch_stats for the loss-and-gradient launch."""
    stream = torch.cuda.current_stream()
    B = Th.shape[1]
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_tu = None if tu is None else torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
    d_out = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, 12), dtype=torch.float64, device="cuda")
    run = lambda: eng.lambda_loss_grad_device(kind, d_th.data_ptr(), Th.shape[0], B, d_out.data_ptr(), d_g.data_ptr(),
                                              space=space, d_T_use=None if d_tu is None else d_tu.data_ptr(),
                                              stream=stream.cuda_stream)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t = [timed(run, stream) for _ in range(reps)]
    return {"B": B, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t),
            "finite": int(np.isfinite(d_g.cpu().numpy()).all(axis=1).sum())}


def fullgrad_case(eng, kind, Th, space, tu, reps, warmup):
    """Case (f): the loss launch, the loss-and-δ/Φ-gradient launch and the loss-and-full-gradient launch on the same
    candidates, alternating within every repetition so that a drift of the shared host falls on all three."""
    stream = torch.cuda.current_stream()
    P_, B = Th.shape
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_tu = None if tu is None else torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
    tu_ptr = None if d_tu is None else d_tu.data_ptr()
    d_out = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, 12), dtype=torch.float64, device="cuda")
    d_f = torch.empty((B, P_), dtype=torch.float64, device="cuda")
    runs = {
        "loss": lambda: eng.loglik_device(kind, d_th.data_ptr(), P_, B, d_out.data_ptr(), space=space, d_T_use=tu_ptr,
                                          stream=stream.cuda_stream),
        "loss_and_grad": lambda: eng.lambda_loss_grad_device(kind, d_th.data_ptr(), P_, B, d_out.data_ptr(),
                                                             d_g.data_ptr(), space=space, d_T_use=tu_ptr,
                                                             stream=stream.cuda_stream),
        "loss_and_full_grad": lambda: eng.lambda_loss_full_grad_device(kind, d_th.data_ptr(), P_, B, d_out.data_ptr(),
                                                                       d_f.data_ptr(), space=space, d_T_use=tu_ptr,
                                                                       stream=stream.cuda_stream)}
    for _ in range(warmup):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            t[k].append(timed(run, stream))
    out = {k: {"B": B, "ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in t.items()}
    out["finite_full_gradients"] = int(np.isfinite(d_f.cpu().numpy()).all(axis=1).sum())
    out["grad_over_loss"] = out["loss_and_grad"]["ms_median"] / out["loss"]["ms_median"]
    out["full_grad_over_loss"] = out["loss_and_full_grad"]["ms_median"] / out["loss"]["ms_median"]
    return out


def grid(kind):
    """The start and its (A, B) trials, constrained (P × 31, or P × 7 without B)."""
    start = S.theta0_constrained(kind)
    cols = [start]
    k = 1
    while (p := R.trial_params(kind, start, k)) is not None:
        cols.append(p)
        k += 1
    return np.asfortranarray(np.stack(cols, axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", default="3,4,5,6,8")
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--cases", default="abcdef")
    ap.add_argument("--max-group-iters", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    mats = S.maturities_30()
    Y = S.simulate_panel(KIND_SD_NS, args.T, maturities=mats)
    eng.set_panel(Y, mats)
    res = {"T": args.T, "N": len(mats), "cases": {}}
    windows = np.linspace(args.T - 239, args.T, 240).astype(np.int32)
    for kind in [int(k) for k in args.kinds.split(",")]:
        name = P.KIND_NAMES[kind]
        G = grid(kind) if kind != P.KIND_NS else S.theta_batch(kind, 31, seed=5, bad_frac=0.0)
        space = 1 if kind != P.KIND_NS else 0
        n = G.shape[1]
        r = {}
        if "a" in args.cases:
            r["a_grid"] = launch_stats(eng, kind, G, space, None, args.reps, args.warmup)
        if "b" in args.cases:
            r["b_windows"] = launch_stats(eng, kind, np.asfortranarray(np.tile(G, (1, 240))), space,
                                          np.repeat(windows, n), args.reps, args.warmup)
        if kind == KIND_SD_NS and "d" in args.cases:
            for tag, Th, tu in (("31", G, None), ("7440", np.asfortranarray(np.tile(G, (1, 240))), np.repeat(windows, n))):
                loss = launch_stats(eng, kind, Th, space, tu, args.reps, args.warmup)
                grad = grad_launch_stats(eng, kind, Th, space, tu, args.reps, args.warmup)
                r[f"d_grad_{tag}"] = {"loss": loss, "loss_and_grad": grad,
                                      "ratio_of_medians": grad["ms_median"] / loss["ms_median"]}
        if "f" in args.cases:
            shapes = [(str(n), G, None)]
            if kind == KIND_SD_NS:
                shapes.append(("7440", np.asfortranarray(np.tile(G, (1, 240))), np.repeat(windows, n)))
            for tag, Th, tu in shapes:
                r[f"f_fullgrad_{tag}"] = fullgrad_case(eng, kind, Th, space, tu, args.reps, args.warmup)
        if kind == KIND_SD_NS and "e" in args.cases:
            model, _ = M.create_model("SD-NS", mats, len(mats), 3)
            Theta0 = np.repeat(S.theta0_constrained(kind)[:, None], 240, axis=1)
            t0 = time.perf_counter()
            est = M.estimate_steps_batch(model, Y, Theta0, T_use=windows, max_group_iters=args.max_group_iters)
            r["e_rolling_estimation"] = {
                "windows": 240, "wall_s": time.perf_counter() - t0, "max_group_iters": args.max_group_iters,
                "n_evals": int(est["n_evals"]), "evals_by_group": {k: int(v) for k, v in est["evals_by_group"].items()},
                "rounds_by_group": {k: int(v) for k, v in est["rounds_by_group"].items()},
                "group_iters_max": int(est["group_iters"].max()), "group_iters_mean": float(est["group_iters"].mean()),
                "status_ok": int((est["status"] == 0).sum()), "ll_mean": float(np.mean(est["ll"]))}
        if kind == KIND_SD_NS and "c" in args.cases:
            Th = S.theta_batch(kind, args.big, seed=5, bad_frac=0.0)
            r["c_big"] = launch_stats(eng, kind, Th, 0, None, args.reps, args.warmup)
            t0 = time.perf_counter()
            for b in range(n):
                R.get_loss(kind, mats, Y, G[:, b], space, R.FLOAT)
            r["a_grid_numpy_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
        res["cases"][name] = r
    # the project's own DNS loglik at the same batch sizes
    dns = {}
    for B in (31, 7440, args.big) if "c" in args.cases else ():
        dns[str(B)] = launch_stats(eng, KIND_DNS, S.theta_batch(KIND_DNS, B, seed=5, bad_frac=0.0), 0, None, args.reps,
                                   args.warmup)
    res["dns_loglik"] = dns
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
