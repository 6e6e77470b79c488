"""Cost and accuracy of the analytic DNS gradient against central differences of the loglik.

    python tools/bench_grad.py [--B 16384] [--T 600] [--reps 7] [--warmup 2]

Speed, at the config-2 shape (T = 600, N = 30): one yfm_loglik_grad_batch_device launch of B candidates against one
yfm_loglik_batch_device launch of the 41·B candidates central differences need (θ and θ ± h·e_i), at its defaults.
HIP events around each launch, `warmup` untimed launches, the median of `reps`, the two alternating.

Accuracy, on fixture case A (tests/golden/grad/grad_cases.npz): the error of central differences of the GPU's
FP64 loglik at each step h, and of the analytic gradient, both as max_i |g − g_fd| / ‖g_fd‖∞ over the compared
candidates (g_fd: fourth-order differences of the binary128 truth).

Prints one JSON line.  Not part of bench.py.
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
sys.path.insert(0, str(ROOT / "tests" / "golden" / "grad"))

import make_grad as MG  # noqa: E402
from yfm_amd import KIND_DNS, Engine, n_params  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402


def timed(run, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    run()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def speed(eng, B, T, reps, warmup):
    mats = S.maturities_30()
    eng.set_panel(S.simulate_panel(KIND_DNS, T, maturities=mats), mats)
    P = n_params(KIND_DNS)
    stream = torch.cuda.current_stream()
    Th = S.theta_batch(KIND_DNS, B, seed=41, bad_frac=0.0)
    d_th = torch.from_numpy(np.ascontiguousarray(Th.T)).cuda()
    d_ll = torch.empty(B, dtype=torch.float64, device="cuda")
    d_g = torch.empty((B, P), dtype=torch.float64, device="cuda")
    # the 2P + 1 points per candidate of central differences
    h = 1e-6
    pts = [Th] + [Th + s * h * np.eye(P)[:, [i]] for i in range(P) for s in (1.0, -1.0)]
    d_fd = torch.from_numpy(np.ascontiguousarray(np.concatenate(pts, axis=1).T)).cuda()
    d_fd_out = torch.empty(d_fd.shape[0], dtype=torch.float64, device="cuda")
    grad = lambda: eng.loglik_grad_device(KIND_DNS, d_th.data_ptr(), P, B, d_ll.data_ptr(), d_g.data_ptr(),
                                          stream=stream.cuda_stream)
    fd = lambda: eng.loglik_device(KIND_DNS, d_fd.data_ptr(), P, d_fd.shape[0], d_fd_out.data_ptr(),
                                   stream=stream.cuda_stream)
    value = lambda: eng.loglik_device(KIND_DNS, d_th.data_ptr(), P, B, d_ll.data_ptr(), stream=stream.cuda_stream)
    for _ in range(warmup):
        grad(), fd(), value()
    torch.cuda.synchronize()
    t = {"grad": [], "fd": [], "value": []}
    for _ in range(reps):
        t["grad"].append(timed(grad, stream))
        t["fd"].append(timed(fd, stream))
        t["value"].append(timed(value, stream))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"B": B, "T": T, "N": len(mats), "grad_launch_ms": med["grad"], "loglik_41B_launch_ms": med["fd"],
            "loglik_B_launch_ms": med["value"], "grad_over_41B": med["grad"] / med["fd"],
            "grad_ms_spread": [min(t["grad"]), max(t["grad"])], "loglik_41B_ms_spread": [min(t["fd"]), max(t["fd"])],
            "finite_gradients": int(np.isfinite(d_g.cpu().numpy()).all(axis=1).sum())}


def accuracy(eng):
    c = MG.load_cases()["A"]
    eng.set_panel(c["Y"], c["maturities"])
    Th, ok = c["Theta"], c["compared"]
    P, B = Th.shape
    gn = np.abs(c["g_fd"]).max(axis=0)
    _, g = eng.loglik_grad(KIND_DNS, Th)
    out = {"analytic_max_rel": float(np.max((np.abs(g - c["g_fd"]).max(axis=0) / gn)[ok]))}
    for h in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
        up = np.concatenate([Th + h * np.eye(P)[:, [i]] for i in range(P)], axis=1)
        dn = np.concatenate([Th - h * np.eye(P)[:, [i]] for i in range(P)], axis=1)
        D = (eng.loglik(KIND_DNS, up) - eng.loglik(KIND_DNS, dn)).reshape(P, B) / (up - dn).reshape(P, P, B)[
            np.arange(P), np.arange(P)]
        out[f"central_h{h:g}_max_rel"] = float(np.max((np.abs(D - c["g_fd"]).max(axis=0) / gn)[ok]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = Engine(0)
    res = {"speed": speed(eng, args.B, args.T, args.reps, args.warmup), "accuracy_case_A": accuracy(eng)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
