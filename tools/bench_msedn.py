"""Cost of the batched loss of the neural Nelson–Siegel models (csrc/yfm_msedn.hip).

    python tools/bench_msedn.py [--T 600] [--reps 7] [--warmup 2] [--cases abcde] [--max-group-iters 10]

The method of tools/bench_msed.py: one yfm_loglik_batch_device launch per case, HIP events around the launch,
`warmup` untimed launches, the median of `reps` with min–max.  All at T = 600 on the N = 30 grid:
  (a) one window's try_initializations grid — the start and its 256 trials, 257 candidates — for 1SD-NNS, 3SD-NNS
      and 3SSD-NNS;
  (b) the rolling driver's grid of 1RWSD-NNS: 240 T_use windows × 17 candidates = 4,080;
  (c) 65,536 candidates of 1SD-NNS (the launch picks L = 4 there);
  (d) NNS at 7,440 candidates.
Each beside the SD-NS λ launch (csrc/yfm_msed.hip) at the same B, in the same visit; and, for scale, the Float64 NumPy
restatement (tests/msedn_reference.py) timed on a few candidates and quoted per candidate.
  (e) one loss-and-gradient launch (yfm_neural_loss_grad_batch_device) against one loss launch for 1SD-NNS at 257
      candidates (its grid) and at 4,080 (17 of them on each of the 240 windows);
  (f) (asked for by name: --cases f) the wall clock of the 240-window rolling re-estimation of 1SD-NNS with its default
      groups (estimate_neural_steps_batch), with evaluations and rounds by group.
  (g) (--cases g) the loss launch, the δ/Φ launch and the full-gradient launch (yfm_neural_loss_fullgrad_batch_device:
      the forward sweep with its trajectory and the adjoint sweep) alternating, for NNS, 1SD-NNS, 3SD-NNS and 3SSD-NNS
      at 257 candidates and at 4,080 (17 on each of the 240 windows): full ÷ loss per kind.
Prints one JSON line.  Not part of bench.py.
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
sys.path.insert(0, str(ROOT / "tools"))

import msedn_reference as R  # noqa: E402
from bench_msed import launch_stats, timed  # noqa: E402
from yfm_amd import Engine  # noqa: E402
from yfm_amd import models as M  # noqa: E402
from yfm_amd import params as P  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def grid(kind):
    """The start and every trial of get_new_initial_params' two-half walk, constrained (P × 257, or P × 17)."""
    start = S.theta0_constrained(kind)
    cols, p, k = [start], start, 1
    while (p := R.trial_params(kind, p, k)) is not None:
        cols.append(p)
        k += 1
    return np.asfortranarray(np.stack(cols, axis=1))


def numpy_ms_per_candidate(kind, mats, Y, Th, space, n=3):
    t0 = time.perf_counter()
    for b in range(n):
        R.get_loss(kind, mats, Y, Th[:, b], space, R.FLOAT)
    return 1e3 * (time.perf_counter() - t0) / n


def alternating_stats(eng, kind, Th, space, tu, reps, warmup):
    """The loss, δ/Φ and full-gradient launches of one batch, timed in turn within every repetition."""
    stream = torch.cuda.current_stream()
    Pn, B = Th.shape
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_tu = None if tu is None else torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
    tup = None if d_tu is None else d_tu.data_ptr()
    d_out = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, Pn), dtype=torch.float64, device="cuda")
    runs = {"loss": lambda: eng.loglik_device(kind, d_th.data_ptr(), Pn, B, d_out.data_ptr(), space=space,
                                              d_T_use=tup, stream=stream.cuda_stream),
            "delta_phi": lambda: eng.neural_loss_grad_device(kind, d_th.data_ptr(), Pn, B, d_out.data_ptr(),
                                                             d_g.data_ptr(), space=space, d_T_use=tup,
                                                             stream=stream.cuda_stream),
            "full": lambda: eng.neural_loss_full_grad_device(kind, d_th.data_ptr(), Pn, B, d_out.data_ptr(),
                                                             d_g.data_ptr(), space=space, d_T_use=tup,
                                                             stream=stream.cuda_stream)}
    for _ in range(warmup):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            t[k].append(timed(run, stream))
    out = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in t.items()}
    out["B"] = B
    out["finite"] = int(np.isfinite(d_g.cpu().numpy()).all(axis=1).sum())
    out["full_over_loss"] = out["full"]["ms_median"] / out["loss"]["ms_median"]
    out["delta_phi_over_loss"] = out["delta_phi"]["ms_median"] / out["loss"]["ms_median"]
    return out


def grad_launch_stats(eng, kind, Th, space, tu, reps, warmup):
    """launch_stats (tools/bench_msed.py) for the neural loss-and-gradient launch."""
    stream = torch.cuda.current_stream()
    B = Th.shape[1]
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_tu = None if tu is None else torch.from_numpy(np.ascontiguousarray(tu, dtype=np.int32)).cuda()
    d_out = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, 12), dtype=torch.float64, device="cuda")
    run = lambda: eng.neural_loss_grad_device(kind, d_th.data_ptr(), Th.shape[0], B, d_out.data_ptr(), d_g.data_ptr(),
                                              space=space, d_T_use=None if d_tu is None else d_tu.data_ptr(),
                                              stream=stream.cuda_stream)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t = [timed(run, stream) for _ in range(reps)]
    return {"B": B, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t),
            "finite": int(np.isfinite(d_g.cpu().numpy()).all(axis=1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--cases", default="abcde")
    ap.add_argument("--max-group-iters", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    mats = S.maturities_30()
    Y = S.simulate_panel(P.KIND_NNS, args.T, maturities=mats)
    eng.set_panel(Y, mats)
    res = {"T": args.T, "N": len(mats), "cases": {}}
    windows = np.linspace(args.T - 239, args.T, 240).astype(np.int32)

    def lam(B, tu=None):
        """The SD-NS λ launch at the same B (and windows)."""
        Th = S.theta_batch(P.KIND_SD_NS, B, seed=5, bad_frac=0.0)
        return launch_stats(eng, P.KIND_SD_NS, Th, 0, tu, args.reps, args.warmup)

    if "a" in args.cases:
        for name in ("1SD-NNS", "3SD-NNS", "3SSD-NNS"):
            kind = next(k for k in P.NEURAL_KINDS if P.KIND_NAMES[k] == name)
            G = grid(kind)
            r = launch_stats(eng, kind, G, 1, None, args.reps, args.warmup)
            r["numpy_restatement_ms_per_candidate"] = numpy_ms_per_candidate(kind, mats, Y, G, 1)
            res["cases"][f"a_grid_{name}"] = r
        res["cases"]["a_grid_SD-NS"] = lam(257)
    if "b" in args.cases:
        kind = P.neural_kind("scalar", True)
        G = grid(kind)
        n = G.shape[1]
        tu = np.repeat(windows, n)
        res["cases"]["b_windows_1RWSD-NNS"] = launch_stats(eng, kind, np.asfortranarray(np.tile(G, (1, 240))), 1, tu,
                                                           args.reps, args.warmup)
        res["cases"]["b_windows_SD-NS"] = lam(240 * n, tu)
    if "c" in args.cases:
        kind = P.neural_kind("scalar")
        Th = S.theta_batch(kind, args.big, seed=5, bad_frac=0.0, a_range=(1e-5, 1e-4))
        res["cases"]["c_big_1SD-NNS"] = launch_stats(eng, kind, Th, 0, None, args.reps, args.warmup)
        res["cases"]["c_big_SD-NS"] = lam(args.big)
    if "d" in args.cases:
        Th = S.theta_batch(P.KIND_NNS, 7440, seed=5, bad_frac=0.0)
        r = launch_stats(eng, P.KIND_NNS, Th, 0, None, args.reps, args.warmup)
        r["numpy_restatement_ms_per_candidate"] = numpy_ms_per_candidate(P.KIND_NNS, mats, Y, Th, 0)
        res["cases"]["d_NNS_7440"] = r
        res["cases"]["d_SD-NS_7440"] = lam(7440)
    if "e" in args.cases:
        kind = P.neural_kind("scalar")
        G = grid(kind)
        for tag, Th, tu in (("257", G, None),
                            ("4080", np.asfortranarray(np.tile(G[:, :17], (1, 240))), np.repeat(windows, 17))):
            loss = launch_stats(eng, kind, Th, 1, tu, args.reps, args.warmup)
            grad = grad_launch_stats(eng, kind, Th, 1, tu, args.reps, args.warmup)
            res["cases"][f"e_grad_1SD-NNS_{tag}"] = {"loss": loss, "loss_and_grad": grad,
                                                     "ratio_of_medians": grad["ms_median"] / loss["ms_median"]}
    if "f" in args.cases:
        kind = P.neural_kind("scalar")
        model, _ = M.create_neural_model("1SD-NNS", mats, len(mats), 3)
        Theta0 = np.repeat(S.theta0_constrained(kind)[:, None], 240, axis=1)
        t0 = time.perf_counter()
        est = M.estimate_neural_steps_batch(model, Y, Theta0, T_use=windows, max_group_iters=args.max_group_iters)
        res["cases"]["f_rolling_estimation_1SD-NNS"] = {
            "windows": 240, "wall_s": time.perf_counter() - t0, "max_group_iters": args.max_group_iters,
            "n_evals": int(est["n_evals"]), "evals_by_group": {k: int(v) for k, v in est["evals_by_group"].items()},
            "rounds_by_group": {k: int(v) for k, v in est["rounds_by_group"].items()},
            "group_iters_max": int(est["group_iters"].max()), "group_iters_mean": float(est["group_iters"].mean()),
            "status_ok": int((est["status"] == 0).sum()), "ll_mean": float(np.mean(est["ll"]))}
    if "g" in args.cases:
        for name in ("NNS", "1SD-NNS", "3SD-NNS", "3SSD-NNS"):
            kind = next(k for k in P.NEURAL_KINDS if P.KIND_NAMES[k] == name)
            G = grid(kind) if name != "NNS" else np.asfortranarray(
                P.transform_params(kind, S.theta_batch(kind, 257, seed=5, bad_frac=0.0)))
            for tag, Th, tu in (("257", G, None),
                                ("4080", np.asfortranarray(np.tile(G[:, :17], (1, 240))), np.repeat(windows, 17))):
                res["cases"][f"g_fullgrad_{name}_{tag}"] = alternating_stats(eng, kind, Th, 1, tu, args.reps, args.warmup)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
