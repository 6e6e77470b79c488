"""Choose the default step of the Hessian (include/yfm.h YFM_INFO_DEFAULT_STEP), on the CPU.

The Hessian of yfm_loglik_info_batch is a fourth-order central difference of the exact gradient,
D_i = (4 c_h − c_2h)/3 with c the central quotient over the realised step, H = ½(D + D').  This script forms the same
H from the host build of the gradient algebra (tests/grad_host_check.cpp: the functions the kernel runs) for
h ∈ {1e-2, 3e-3, 1e-3, 3e-4, 1e-4} on the truth-Hessian candidates of tests/golden/info/info_cases.npz and prints, per
step, every candidate's max |H − H_truth| / ‖H_truth‖max and the worst of them.  The step with the smallest worst
case is the default (DESIGN.md §3.11 holds the table).

    python tools/hessian_step_table.py
"""
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden" / "info"))
sys.path.insert(0, str(ROOT / "yieldfactormodels.jl_amd"))
sys.path.insert(0, str(ROOT))
import make_info as MI  # noqa: E402
from host_check_io import build_host_check, run_grad_host as run_host  # noqa: E402

STEPS = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4)


def hessian(exe, tmp, Y, m, th, h):
    P = th.size
    cols, den = [], np.empty((P, 2))
    for i in range(P):
        for k, mult in enumerate((1.0, 2.0)):
            up, dn = th.copy(), th.copy()
            up[i] += mult * h
            dn[i] -= mult * h
            den[i, k] = up[i] - dn[i]
            cols += [up, dn]
    X = np.stack(cols, axis=1)
    _, g = run_host(exe, tmp, Y, m, X, np.full(X.shape[1], Y.shape[1]))
    g = g.reshape(P, P, 2, 2)  # [component, direction, h or 2h, up or down]
    c = (g[:, :, :, 0] - g[:, :, :, 1]) / den[None, :, :]
    D = ((4.0 * c[:, :, 0] - c[:, :, 1]) / 3.0).T  # D[i, j] = ∂g_j/∂θ_i
    return 0.5 * (D + D.T)


def main():
    cases = MI.load_cases()
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        exe = build_host_check(tmp, "grad_host_check")
        print("step     " + "  ".join(f"{n}[{b}]" for n in MI.HESS_CASES for b in range(cases[n]["Theta"].shape[1]))
              + "   worst")
        worst = {}
        for h in STEPS:
            row = []
            for n in MI.HESS_CASES:
                c = cases[n]
                for b in range(c["Theta"].shape[1]):
                    H = hessian(exe, tmp, c["Y"], c["maturities"], c["Theta"][:, b], h)
                    row.append(np.abs(H - c["H_truth"][:, :, b]).max() / np.abs(c["H_truth"][:, :, b]).max())
            worst[h] = max(row)
            print(f"{h:<8g} " + "  ".join(f"{v:.2e}" for v in row) + f"   {worst[h]:.2e}")
        best = min(worst, key=worst.get)
        ref = [c["ref_err"][b] / np.abs(c["H_truth"][:, :, b]).max() for c in (cases[n] for n in MI.HESS_CASES)
               for b in range(c["Theta"].shape[1])]
        print("plain FP64 reference (second differences of the dense oracle, its best step): "
              + "  ".join(f"{v:.2e}" for v in ref))
        print(f"smallest worst case: h = {best:g}")


if __name__ == "__main__":
    main()
