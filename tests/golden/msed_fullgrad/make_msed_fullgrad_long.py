"""Writes msed_fullgrad_long.npz: the truth for the λ models' full loss gradient at estimation length — N = 30,
T = 600 — by make_msed_fullgrad.py's recipe (its fd_gradient, analytic, screen and start grid are imported): central
differences of the 40-digit restatement of get_loss over all P rows, in both parameter spaces.

Per kind (NS, SD-NS, RWSD-NS, SSD-NS, SRWSD-NS)
    n30t600       the 30 × 600 panel, 2 screened candidates θ₀ + 0.1·N(0, I), T_use = 600
and for SD-NS and SRWSD-NS (kinds 4 and 8)
    n30t600win    the same two candidates on the panel with Y[0, 450] = NaN, T_use = (300, 600): the short window ends
                  before the missing column, the long one compares it and returns −Inf with no gradient.

The panel is the same for every kind and is stored once (`Y`, `maturities`); load_cases hands every case its own
`{name}_Y` as make_msed_fullgrad.load_cases does.  One 40-digit loss costs about 4 s at T = 600, a candidate in one
space about 4 minutes.

    python tests/golden/msed_fullgrad/make_msed_fullgrad_long.py      # about a quarter of an hour on 8 processes
"""
from __future__ import annotations

import math
import sys
import time
from multiprocessing import Pool
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_msed_fullgrad as MF  # noqa: E402  (fd_gradient, analytic, screened, START_GRID, SCREEN, n_lead)

FILE = HERE / "msed_fullgrad_long.npz"
KINDS = MF.KINDS
N, T, NB = 30, 600, 2
NAN_AT = (0, 450)
WINDOW_KINDS = (4, 8)
WINDOWS = np.array([300, 600])


def case_names():
    return [f"k{kind}_n30t600" for kind in KINDS] + [f"k{kind}_n30t600win" for kind in WINDOW_KINDS]


def panel():
    from yfm_amd import synthetic as S
    mats = MF.maturities(N)
    return mats, S.simulate_panel(3, T, maturities=mats, seed=7)


def with_nan(Y):
    Y = Y.copy(order="F")
    Y[NAN_AT] = np.nan
    return Y


def candidates(kind, mats, Y):
    """Θ unconstrained P×2: make_msed_fullgrad.case_inputs' replacement loop over two columns, screened at T_use = T
    (and, for the window kinds, at the short window on the panel with the missing column)."""
    from yfm_amd import synthetic as S
    from yfm_amd.params import transform_params
    Th = S.theta_batch(kind, NB, scale=0.1, seed=11 + kind, bad_frac=0.0)
    Yn = with_nan(Y)

    def ok(th, b):
        tc = transform_params(kind, th)
        if not MF.screened(kind, mats, Y, T, th, tc, False):
            return False
        if kind in WINDOW_KINDS and WINDOWS[b] <= NAN_AT[1]:
            return MF.screened(kind, mats, Yn, int(WINDOWS[b]), th, tc, False)
        return True

    for b in range(NB):
        seed, r = 11 + kind, 0
        while not ok(Th[:, b], b):
            seed, r = seed + 100, r + 1
            assert r < 200, (kind, b)
            Th[:, b] = S.theta_batch(kind, NB, scale=0.1, seed=seed, bad_frac=0.0)[:, b]
            if kind != 3:
                a, bb = MF.START_GRID[(r - 1) % len(MF.START_GRID)]
                Th[0, b] += math.log(a / 1e-3)
                if kind in (4, 6):
                    Th[1, b] += math.log(bb / (1 - bb)) - math.log(0.98 / 0.02)
    return Th


def build(processes=8):
    import msed_reference as R
    from yfm_amd.params import transform_params
    mats, Y = panel()
    Yn = with_nan(Y)
    out = {"maturities": mats, "Y": Y, "nan_at": np.array(NAN_AT)}
    jobs, keys = [], []
    for kind in KINDS:
        Th = candidates(kind, mats, Y)
        Tc = np.stack([transform_params(kind, Th[:, b]) for b in range(NB)], axis=1)
        variants = [(f"k{kind}_n30t600", Y, np.array([T, T]))]
        if kind in WINDOW_KINDS:
            variants.append((f"k{kind}_n30t600win", Yn, WINDOWS))
        for pre, Yv, tu in variants:
            out[f"{pre}_T_use"], out[f"{pre}_theta"], out[f"{pre}_theta_c"] = tu, Th, Tc
            for space, X in ((0, Th), (1, Tc)):
                out[f"{pre}_loss_s{space}"] = np.array(
                    [R.get_loss(kind, mats, Yv, X[:, b], space, R.FLOAT, int(tu[b])) for b in range(NB)])
                for b in range(NB):
                    jobs.append((kind, mats, Yv, X[:, b].copy(), space, int(tu[b])))
                    keys.append((pre, space, b))
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][5])  # the long windows first
    with Pool(processes) as pool:
        res = pool.map(MF.fd_gradient, [jobs[i] for i in order], chunksize=1)
    worst = 0.0
    for i, (g, e) in zip(order, res):
        pre, space, b = keys[i]
        kind, _, Yv, x, _, tu = jobs[i]
        out.setdefault(f"{pre}_g_fd_s{space}", np.empty((len(g), NB)))[:, b] = g
        out.setdefault(f"{pre}_e_fd_s{space}", np.empty(NB))[b] = e
        if np.isfinite(g).all():
            K, top = MF.n_lead(kind), np.max(np.abs(g))
            assert np.all(np.abs(g[:K]) >= MF.SCREEN * top), (pre, space, b, g[:K], top)  # the screen, on the truth
            ga = MF.analytic(kind, mats, Yv, x, space, tu)[1]
            ratio = float(np.max(np.abs(ga - g)) / top)
            worst = max(worst, ratio)
            print(f"{pre} space {space} b={b}: e_fd/|g| {e / top:.2e}, formulas / truth ratio {ratio:.3e}")
    print(f"worst max|g_formulas - g_fd| / |g_fd|inf over the fixture: {worst:.3e}")
    return out


def load_cases():
    """{key: array} with the keys of make_msed_fullgrad.load_cases: the panel stored once is handed to every case."""
    with np.load(FILE) as z:
        c = {k: z[k] for k in z.files}
    Yn = c["Y"].copy(order="F")
    Yn[tuple(c["nan_at"])] = np.nan
    for name in case_names():
        c[f"{name}_maturities"] = c["maturities"]
        c[f"{name}_Y"] = Yn if name.endswith("win") else c["Y"]
    return c


if __name__ == "__main__":
    t0 = time.time()
    np.savez_compressed(FILE, **build())
    print(f"generated in {time.time() - t0:.0f} s")
