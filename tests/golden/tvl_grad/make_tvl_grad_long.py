"""Generator of tests/golden/tvl_grad/tvl_grad_long_cases.npz: reference gradients of the TVλ log-likelihood at
estimation length (T = 200 and 600, N = 30), by make_tvl_grad.py's recipe — fourth-order central differences of the
binary128 truth over a ladder of steps, the step with the smallest e(h)/‖g_h‖∞ kept per candidate — with a longer
ladder: over 600 EKF steps the curvature of the loglik along some directions is large enough that the truncation
error of make_tvl_grad.LADDER's smallest step (1e-7) is still above 1e-9·‖g‖∞, and binary128 leaves room for steps down
to 1e-9.  `compared` is make_tvl_grad.py's: every truth evaluation finite, e_fd ≤ 1e-9·‖g_fd‖∞ and
|oracle − truth| ≤ 1e-9·max(1, |truth|).

Cases (θ = theta_batch(KIND_TVL, 16, 0.02, SEED); the bench panel's recipe at N = 30)
    L200          T = 200, 16 candidates
    L600          T = 600, 16 candidates
    L600-windows  the first 8 candidates of L600 on the panel with column 450 all NaN and one NaN entry in column 598,
                  T_use cycling through (200, 599, 600)

SEED is the first of 11, 12, 13, … with which every case has at least 75% of its candidates compared and one to spare
(NEED: 13 of 16, 13 of 16, 7 of 8); the choice reads the truth and the dense oracle only.  Most seeds miss it at
T = 600: over 600 EKF steps the differences resolve only about 60% of θ₀ + 0.02·N(0, I) at any rung (on the rest g_h
and g_3h still differ by 1e-6 … 0.9 of ‖g‖∞ at h = 1e-9).  Seed 11 gives L600 10 of 16, seed 16 9 of 16, seed 19 at
most 12; seeds 12, 13, 15, 17 give L600-windows 5, 6, 6, 5 of 8 and seed 18 at most 6; seed 14 misses on the oracle's
distance alone.  Seed 20 gives 15 of 16, 15 of 16 and 8 of 8.  `python … --search [first seed]` repeats the choice
(about 6 minutes on 8 threads for a seed that gets as far as L600).

The T = 600 panel is stored once (under L600); L600-windows stores the positions of its NaN entries.

Run from the repository root:  python tests/golden/tvl_grad/make_tvl_grad_long.py      # it prints its own time
"""
from __future__ import annotations

import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_tvl_grad as MT  # noqa: E402  (fd_gradient, REL, ORACLE_REL; it puts the repository on sys.path)
from oracle import truth as TR  # noqa: E402
from yfm_amd import KIND_TVL  # noqa: E402
from yfm_amd import synthetic as S  # noqa: E402

FILE = HERE / "tvl_grad_long_cases.npz"
LADDER = (1e-6, 3e-7, 1e-7, 3e-8, 1e-8, 3e-9, 1e-9)
SEED = 20
NEED = {"L200": 13, "L600": 13, "L600-windows": 7}
CASE_NAMES = ("L200", "L600", "L600-windows")
WINDOWS = (200, 599, 600)


def three(h: float) -> float:
    """3h as the decimal literal (3 × 1e-7 is 3e-7, a rung of the ladder: its evaluations are shared)."""
    return float(f"{3.0 * h:.3g}")


def case_inputs(name: str, seed: int = SEED):
    """(Y, maturities, Theta, T_use or None) of a case."""
    m = S.maturities_30()
    Th = S.theta_batch(KIND_TVL, 16, 0.02, seed, bad_frac=0)
    if name == "L200":
        return S.simulate_panel(KIND_TVL, 200, m, 5), m, Th, None
    Y = S.simulate_panel(KIND_TVL, 600, m, 5)
    if name == "L600":
        return Y, m, Th, None
    if name == "L600-windows":
        Y = Y.copy(order="F")
        Y[:, 450] = np.nan
        Y[3, 598] = np.nan
        return Y, m, np.asfortranarray(Th[:, :8]), np.array((WINDOWS * 3)[:8], dtype=np.int32)
    raise KeyError(name)


def make_case(name: str, seed: int = SEED) -> dict:
    """make_tvl_grad.make_case over this script's LADDER."""
    Y, m, Th, tu = case_inputs(name, seed)
    B = Th.shape[1]
    t0 = time.time()
    with np.errstate(all="ignore"):
        steps = sorted({h for h0 in LADDER for h in (h0, three(h0))})
        gs = {h: MT.fd_gradient(Y, m, Th, tu, h) for h in steps}
        g_fd = np.zeros_like(Th)
        e_fd = np.full(B, np.inf)
        h_used = np.zeros(B)
        ratio = np.full(B, np.inf)
        ok = np.ones(B, dtype=bool)
        for h in steps:
            ok &= gs[h][1]
        for h in LADDER:
            g1, g3 = gs[h][0], gs[three(h)][0]
            e = np.abs(g1 - g3).max(axis=0)
            gn = np.abs(g1).max(axis=0)
            r = np.where(gn > 0, e / np.where(gn > 0, gn, 1.0), np.where(e == 0, 0.0, np.inf))
            r = np.where(np.isfinite(r), r, np.inf)
            better = (r < ratio) | ((h_used == 0) & (r <= ratio))
            g_fd[:, better] = g1[:, better]
            e_fd[better] = e[better]
            h_used[better] = h
            ratio[better] = r[better]
        truth = TR.loglik_truth(KIND_TVL, Y, m, Th, space=0, T_use=tu)
        oracle = TR.loglik_oracle(KIND_TVL, Y, m, Th, space=0, T_use=tu)
        fd_ok = ok & np.isfinite(truth) & np.isfinite(e_fd) & (e_fd <= MT.REL * np.abs(g_fd).max(axis=0))
        oracle_err = np.abs(oracle - truth) / np.maximum(1.0, np.abs(truth))
        compared = fd_ok & (oracle_err <= MT.ORACLE_REL)
    print(f"{name} (seed {seed}): finite-and-e_fd {int(fd_ok.sum())}/{B}, compared {int(compared.sum())}/{B}, "
          f"worst |oracle − truth| {np.nanmax(oracle_err):.2e}, {time.time() - t0:.0f} s", flush=True)
    return dict(Y=Y, maturities=np.asarray(m, dtype=np.float64), Theta=Th,
                T_use=np.full(B, Y.shape[1], dtype=np.int32) if tu is None else tu,
                g_fd=g_fd, e_fd=e_fd, h_used=h_used, compared=compared, loglik_oracle=oracle, loglik_truth=truth)


def oracle_ok(name: str, seed: int) -> int:
    """How many candidates of a case pass the cheap half of `compared`, |oracle − truth| ≤ 1e-9·max(1, |truth|)."""
    Y, m, Th, tu = case_inputs(name, seed)
    with np.errstate(all="ignore"):
        truth = TR.loglik_truth(KIND_TVL, Y, m, Th, space=0, T_use=tu)
        oracle = TR.loglik_oracle(KIND_TVL, Y, m, Th, space=0, T_use=tu)
        return int((np.abs(oracle - truth) / np.maximum(1.0, np.abs(truth)) <= MT.ORACLE_REL).sum())


def search(first: int = 11):
    """The first seed with the margin in every case.  A seed that already misses it on the loglik's own
    condition is passed over without taking its differences."""
    seed = first
    while True:
        cheap = {name: oracle_ok(name, seed) for name in CASE_NAMES}
        print(f"seed {seed}: oracle within the bar on {cheap}", flush=True)
        if all(cheap[name] >= NEED[name] for name in CASE_NAMES):
            # the cheapest of the T = 600 cases first: they are the ones most seeds miss
            if all(int(make_case(name, seed)["compared"].sum()) >= NEED[name] for name in reversed(CASE_NAMES)):
                return seed
        seed += 1


def load_cases(path=FILE) -> dict:
    """{case name: {field: array}} of the committed file; L600-windows gets L600's panel with its NaN entries."""
    out: dict = {}
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            name, field = k.split("/", 1)
            out.setdefault(name, {})[field] = z[k]
    w = out["L600-windows"]
    Y = out["L600"]["Y"].copy(order="F")
    idx = w.pop("nan_index")
    Y[idx[:, 0], idx[:, 1]] = np.nan
    w["Y"], w["maturities"] = Y, out["L600"]["maturities"]
    return {name: out[name] for name in CASE_NAMES}


def main():
    t0 = time.time()
    if "--search" in sys.argv:
        print("first seed with the margin:", search(int(sys.argv[-1]) if sys.argv[-1].isdigit() else 11))
        return
    save({name: make_case(name) for name in CASE_NAMES})
    print(f"generated in {time.time() - t0:.0f} s")


def save(cases: dict):
    flat = {}
    for name in CASE_NAMES:
        c = dict(cases[name])
        assert int(c["compared"].sum()) >= NEED[name], name
        if name == "L600-windows":
            c["nan_index"] = np.argwhere(np.isnan(c["Y"]))
            del c["Y"], c["maturities"]
        for k, v in c.items():
            flat[f"{name}/{k}"] = v
    np.savez_compressed(FILE, **flat)


if __name__ == "__main__":
    main()
