"""CPU test that the shared Kalman parameter header (csrc/yfm_kalman_map.hpp: decode, chain_factor, mean_solve,
lyapunov_matrix, gauss_solve) is the reference's map for every (M, LEAD) the project has — DNS (3, 1), TVλ (4, 0) and
GNS5 (5, 2), the last of which no tangent kernel instantiates yet.  tests/kalman_map_host_check.cpp, a stand-alone
program, is built plain and with -fsanitize=address,undefined; both builds run every case and must print the same bytes.

Inputs, per kind: the project's default start (synthetic.theta0), and a hard θ whose Φ diagonal is ±(1 − 1.2e-5) in
the constrained space (unconstrained ±12) with σ² = e⁻⁶⁰ ≈ 8.8e-27; each in the unconstrained space and, transformed,
in the constrained one.

Bounds, with ε = 2⁻⁵² (one ulp of 1) and none of them taken from the program's output:
  exp rows       two correctly-rounded-to-1-ulp exps (libm's, NumPy's) differ by at most 2 ulp: 2ε relative.
  Φ diagonal     e = 2y/(1+y) − 1 with y = eˣ: y differs by 2ε relative, which moves 2y/(1+y) ∈ [0, 2) by at most
                 2y/(1+y)²·2ε ≤ ε; the rounded 1 + y and the rounded quotient can each differ by an ulp of theirs,
                 2ε and 2ε of a value below 2; the subtraction rounds within ε: 6ε absolute.
  Q = U'U        M fmas per entry here, M products and M − 1 sums in NumPy: each within M·ε/2 of Σ|U_li||U_lj|, and the
                 2ε of the two diagonal factors gives 4ε of the same sum: (M + 4)·ε·(|U|'|U|)_ij.
  chain factors  the exp rows are the decoded value itself (the same libm exp): exact.  2y/(1+y)² has |dlog f/dlog y| =
                 |1 − y|/(1 + y) ≤ 1, so 2ε from y, and four rounded operations at ε each: 6ε relative.
  P₁, a₁         Gaussian elimination with partial pivoting is backward stable: the residual of the S × S system is at
                 most c·ε·‖L‖∞‖p̂‖∞ with c of the order of S in practice and 3S³ρ at worst (Higham, Accuracy and
                 Stability of Numerical Algorithms, Theorem 9.5); S² is asserted.  ‖L‖∞‖p̂‖∞ ≤ κ∞(L)·‖Q‖, the form in ‖Q‖
                 and the operator's conditioning, which is printed.  The residual is evaluated in extended precision.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from grad_rule import SPACE_ROWS
from host_check_io import build_host_check, hexf
from yfm_amd import KIND_DNS, KIND_GNS, KIND_TVL, params, synthetic

EPS = 2.0 ** -52
KINDS = {"dns": KIND_DNS, "tvl": KIND_TVL, "gns5": KIND_GNS}


def hard_theta(kind):
    """Φ diagonal ±12 (alternating, so pairs of equal and of opposite sign both occur), σ² row −60."""
    lay = params.param_layout(kind)
    th = synthetic.theta0(kind).copy()
    th[lay.base_offset] = -60.0
    for i in range(lay.M):
        th[lay.phi_offset + i * (lay.M + 1)] = 12.0 if i % 2 == 0 else -12.0
    return th


def cases():
    out = []
    for name, kind in KINDS.items():
        for label, th in (("start", synthetic.theta0(kind)), ("hard", hard_theta(kind))):
            out.append((f"{name}-{label}", kind, 0, th))
            out.append((f"{name}-{label}-constrained", kind, 1, params.transform_params(kind, th)))
    return out


CASES = cases()


def parse(text):
    blocks, cur = [], None
    for ln in text.split("\n"):
        if not ln:
            continue
        label, *vals = ln.split()
        if label == "theta_c":
            cur = {}
            blocks.append(cur)
        cur[label] = np.array([float.fromhex(v) for v in vals])
    return blocks


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("kalman_map")
    words = []
    for _, kind, space, th in CASES:
        lay = params.param_layout(kind)
        words += [str(lay.M), str(lay.n_lead), str(space)] + [hexf(v) for v in th]
    (d / "cases.txt").write_text(" ".join(words))
    outs = [subprocess.run([str(build_host_check(d, "kalman_map_host_check", sanitize=s)), str(d / "cases.txt")],
                           check=True, capture_output=True, text=True).stdout for s in (False, True)]
    assert outs[0] == outs[1]  # the sanitized build computes the same bits
    blocks = parse(outs[0])
    assert len(blocks) == len(CASES)
    return {name: (kind, space, th, b) for (name, kind, space, th), b in zip(CASES, blocks)}


def split(kind, tc):
    """(σ², U, δ, Φ) of a θ_c in θ's layout."""
    lay = params.param_layout(kind)
    M = lay.M
    U = np.zeros((M, M))
    k = lay.u_offset
    for j in range(M):
        for i in range(j + 1):
            U[i, j] = tc[k]
            k += 1
    return tc[lay.base_offset], U, tc[lay.delta_offset:lay.delta_offset + M], tc[lay.phi_offset:].reshape(M, M)


IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name", IDS)
def test_decode_is_transform_params_and_set_params(results, name):
    kind, space, th, b = results[name]
    codes = params.transform_codes(kind)
    want = params.transform_params(kind, th) if space == 0 else th
    got = b["theta_c"]
    assert got.shape == want.shape
    err = np.abs(got - want)
    print(name, "max |θ_c − transform_params| / ε:", (err / EPS).max())
    if space == 1:
        assert np.array_equal(got, th)  # the constrained space returns θ unchanged
    ident = codes == params.ID
    assert np.array_equal(got[ident], want[ident])
    pos = codes == params.POS
    assert np.all(err[pos] <= 2 * EPS * np.abs(want[pos]))
    assert np.all(err[codes == params.R11] <= 6 * EPS)
    M = params.param_layout(kind).M
    _, U, _, _ = split(kind, want)
    Q = b["Q"].reshape(M, M)
    qerr = np.abs(Q - U.T @ U)
    qbound = (M + 4) * EPS * (np.abs(U).T @ np.abs(U))
    print(name, "max Q err / bound:", (qerr / qbound).max())
    assert np.all(qerr <= qbound)
    assert np.array_equal(Q, Q.T)


@pytest.mark.parametrize("name", IDS)
def test_chain_factor_rows_are_the_transform_codes(results, name):
    kind, space, th, b = results[name]
    lay = params.param_layout(kind)
    codes = params.transform_codes(kind)
    f = b["chain"]
    assert f.shape == (lay.P + 1,) and f[lay.P] == 1.0  # the padding row d = P
    f = f[:lay.P]
    if space == 1:
        assert np.all(f == 1.0)
        return
    assert np.array_equal(f != 1.0, codes != params.ID)
    exp_rows, phi_rows = np.flatnonzero(codes == params.POS), np.flatnonzero(codes == params.R11)
    if kind in SPACE_ROWS:
        assert (tuple(exp_rows), tuple(phi_rows)) == SPACE_ROWS[kind][:2]
    assert np.array_equal(f[exp_rows], b["theta_c"][exp_rows])
    y = np.exp(th[phi_rows])
    want = 2.0 * y / ((1.0 + y) * (1.0 + y))
    rel = np.abs(f[phi_rows] - want) / want
    print(name, "max Φ-row factor err / ε:", (rel / EPS).max())
    assert np.all(rel <= 6 * EPS)


def residual_bound(A, x, rhs):
    """(‖Ax − rhs‖∞ in extended precision, n²·ε·‖A‖∞‖x‖∞)."""
    n = A.shape[0]
    r = np.abs(A.astype(np.longdouble) @ x.astype(np.longdouble) - rhs.astype(np.longdouble)).max()
    return float(r), n * n * EPS * np.abs(A).sum(axis=1).max() * np.abs(x).max()


@pytest.mark.parametrize("name", IDS)
def test_initial_moments_solve_their_systems(results, name):
    kind, space, th, b = results[name]
    M = params.param_layout(kind).M
    _, _, delta, Phi = split(kind, b["theta_c"])
    Q = b["Q"].reshape(M, M)
    # a₁ = (I − Φ) \ δ: the same mean and verdict whether or not the inverse is asked for
    A = np.eye(M) - Phi
    assert b["mean"][0] == 1.0 and b["mean_inv"][0] == 1.0
    a = b["mean"][1:]
    assert np.array_equal(a, b["mean_inv"][1:1 + M])
    r, bound = residual_bound(A, a, delta)
    print(name, "mean residual / bound:", r / bound)
    assert r <= bound
    Ainv = b["mean_inv"][1 + M:].reshape(M, M)
    for j in range(M):
        r, bound = residual_bound(A, Ainv[:, j], np.eye(M)[:, j])
        assert r <= bound
    # P₁ − ΦP₁Φ' = Q on the symmetric subspace
    assert b["P1"][0] == 1.0
    P1 = b["P1"][1:].reshape(M, M)
    assert np.array_equal(P1, P1.T)
    pairs = [(i, j) for i in range(M) for j in range(i, M)]
    L = np.array([[(r == c) - (Phi[i, k] * Phi[j, l] + (Phi[i, l] * Phi[j, k] if k != l else 0.0))
                   for c, (k, l) in enumerate(pairs)] for r, (i, j) in enumerate(pairs)])
    p = np.array([P1[i, j] for i, j in pairs])
    q = np.array([Q[i, j] for i, j in pairs])
    r, bound = residual_bound(L, p, q)
    kappa = np.linalg.cond(L, np.inf)
    print(name, f"P₁ residual {r:.3e}, bound {bound:.3e}, κ∞(L) {kappa:.3e}, κ∞·‖Q‖·S²ε "
                f"{len(pairs) ** 2 * EPS * kappa * np.abs(q).max():.3e}")
    assert r <= bound
    ld = np.longdouble  # the matrix equation itself: the same residuals, entry by entry
    assert np.abs(P1.astype(ld) - Phi.astype(ld) @ P1.astype(ld) @ Phi.T.astype(ld) - Q.astype(ld)).max() <= bound
