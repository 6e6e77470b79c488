"""Checkers of the fixed-interval Kalman smoother (include/yfm.h yfm_smooth_batch) — test infrastructure only.

The model is the fixed-loading one of filter.jl:125-179 with initialize_filter (filter.jl:1-10); decoding and loadings
come from the untouched oracle modules.  Three independent statements of β̂_t = E[β_t | y_1..n], V_t and
C_t = Cov(β_{t+1}, β_t | y_1..n), none of them in the kernel's collapsed M × M form:

  (a) smooth_dense    FP64: N × N F_t, filtered moments, then the Rauch–Tung–Striebel gain J_t = P_{t|t}Φ'P_{t+1}⁻¹;
                      C_t = V_{t+1}J_t'.
  (b) smooth_mp       the same in 40-digit mpmath, rounded to FP64 on the way out: the truth.
  (c) smooth_joint    for tiny cases: the Gaussian conditional formed directly from the stacked covariance of
                      (β_1 … β_n, y_obs).

All return (beta_s M × n, V_s M × M × n, C_s M × M × (n − 1)); slot t − 1 holds the quantities of column t, and
C_s[:, :, t − 1] = Cov(β_{t+1}, β_t | ·).  A column with any NaN is missing.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

from oracle import kalman_mp as KM
from oracle import kalman_oracle as O

STATE_DIM = {O.KIND_DNS: 3, O.KIND_GNS: 5}


def model_fp64(kind, mats, theta, space=0):
    """(Z, σ², Q, δ, Φ) as the oracle decodes them."""
    M = STATE_DIM[kind]
    s = O.KalmanState.fresh(kind, mats, M)
    tc = O.transform_params(O.transform_codes(kind, M), theta) if space == 0 else np.asarray(theta, dtype=np.float64)
    O.set_params(s, tc)
    return s.Z.copy(), float(s.Omega_obs[0, 0]), s.Omega_state.copy(), s.delta.copy(), s.Phi.copy()


def initial_fp64(Q, delta, Phi):
    M = len(delta)
    a1 = np.linalg.solve(np.eye(M) - Phi, delta)
    vecP = np.linalg.solve(np.eye(M * M) - np.kron(Phi, Phi), Q.reshape(-1, order="F"))
    return a1, vecP.reshape((M, M), order="F")


def smooth_dense(kind, mats, Y, theta, space=0, n=None):
    """(a): the dense FP64 forward filter and the RTS backward pass."""
    Z, sig2, Q, delta, Phi = model_fp64(kind, mats, theta, space)
    N, M = Z.shape
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1] if n is None else int(n)
    a, P = initial_fp64(Q, delta, Phi)
    ap, Pp, af, Pf = [], [], [], []
    for t in range(n):
        y = Y[:, t]
        ap.append(a)
        Pp.append(P)
        if np.any(np.isnan(y)):
            a_f, P_f = a, P
        else:
            F = Z @ P @ Z.T + sig2 * np.eye(N)
            K = np.linalg.solve(F, Z @ P).T
            a_f = a + K @ (y - Z @ a)
            P_f = P - K @ Z @ P
            P_f = 0.5 * (P_f + P_f.T)
        af.append(a_f)
        Pf.append(P_f)
        a = delta + Phi @ a_f
        P = Phi @ P_f @ Phi.T + Q
    bs = np.empty((M, n))
    Vs = np.empty((M, M, n))
    Cs = np.empty((M, M, max(n - 1, 0)))
    bs[:, n - 1], Vs[:, :, n - 1] = af[n - 1], Pf[n - 1]
    for t in range(n - 2, -1, -1):
        J = np.linalg.solve(Pp[t + 1], Phi @ Pf[t]).T  # P_{t|t} Φ' P_{t+1}⁻¹
        bs[:, t] = af[t] + J @ (bs[:, t + 1] - ap[t + 1])
        V = Pf[t] + J @ (Vs[:, :, t + 1] - Pp[t + 1]) @ J.T
        Vs[:, :, t] = 0.5 * (V + V.T)
        Cs[:, :, t] = Vs[:, :, t + 1] @ J.T
    return bs, Vs, Cs


def _to_np(Mx, r, c):
    return np.array([[float(Mx[i, j]) for j in range(c)] for i in range(r)])


def _mp_solve(A, Bm):
    """A⁻¹B for a matrix B, one LU factorisation."""
    LU, p = mp.mp.LU_decomp(A)
    X = mp.matrix(Bm.rows, Bm.cols)
    for j in range(Bm.cols):
        x = mp.mp.U_solve(LU, mp.mp.L_solve(LU, Bm[:, j], p))
        for i in range(Bm.rows):
            X[i, j] = x[i]
    return X


def smooth_mp(kind, mats, Y, theta, space=0, n=None):
    """(b): smooth_dense in 40-digit arithmetic on the same FP64 inputs."""
    M, gam, sig2, Q, d, Phi = KM._decode(kind, theta, space)
    mm = [mp.mpf(float(x)) for x in mats]
    N = len(mm)
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1] if n is None else int(n)
    Z = mp.matrix(N, M)
    for i in range(N):
        Z[i, 0] = 1
        for l, g in enumerate(gam):
            s, c, _ = KM._pair(mp.mpf("0.01") + mp.exp(g), mm[i])
            Z[i, 1 + 2 * l], Z[i, 2 + 2 * l] = s, c
    I = mp.eye(M)
    a = mp.lu_solve(I - Phi, d)
    K2 = mp.matrix(M * M, M * M)
    for i1 in range(M):
        for i2 in range(M):
            for j1 in range(M):
                for j2 in range(M):
                    r, c = i1 * M + i2, j1 * M + j2
                    K2[r, c] = (1 if r == c else 0) - Phi[i1, j1] * Phi[i2, j2]
    vp = mp.lu_solve(K2, mp.matrix([Q[r % M, r // M] for r in range(M * M)]))
    P = mp.matrix(M, M)
    for r in range(M * M):
        P[r % M, r // M] = vp[r]
    ap, Pp, af, Pf = [], [], [], []
    for t in range(n):
        y = Y[:, t]
        ap.append(a)
        Pp.append(P)
        if np.any(np.isnan(y)):
            a_f, P_f = a, P
        else:
            F = Z * P * Z.T + sig2 * mp.eye(N)
            K = _mp_solve(F, Z * P).T
            a_f = a + K * (mp.matrix(y.tolist()) - Z * a)
            P_f = P - K * Z * P
        af.append(a_f)
        Pf.append(P_f)
        a = d + Phi * a_f
        P = Phi * P_f * Phi.T + Q
    b_cur, V_cur = af[n - 1], Pf[n - 1]
    bs = np.empty((M, n))
    Vs = np.empty((M, M, n))
    Cs = np.empty((M, M, max(n - 1, 0)))
    bs[:, n - 1] = [float(b_cur[i]) for i in range(M)]
    Vs[:, :, n - 1] = _to_np(V_cur, M, M)
    for t in range(n - 2, -1, -1):
        J = _mp_solve(Pp[t + 1], Phi * Pf[t]).T
        C = V_cur * J.T
        b_cur = af[t] + J * (b_cur - ap[t + 1])
        V_cur = Pf[t] + J * (V_cur - Pp[t + 1]) * J.T
        bs[:, t] = [float(b_cur[i]) for i in range(M)]
        Vs[:, :, t] = _to_np(V_cur, M, M)
        Cs[:, :, t] = _to_np(C, M, M)
    Vs = 0.5 * (Vs + np.transpose(Vs, (1, 0, 2)))
    return bs, Vs, Cs


def smooth_joint(kind, mats, Y, theta, space=0, n=None):
    """(c): E and Cov of (β_1 … β_n) given the observed entries' columns, from the joint Gaussian.  Tiny cases only."""
    Z, sig2, Q, delta, Phi = model_fp64(kind, mats, theta, space)
    N, M = Z.shape
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1] if n is None else int(n)
    a1, P1 = initial_fp64(Q, delta, Phi)
    mu = np.empty((n, M))
    S = np.empty((n, M, n, M))  # Cov(β_s, β_t)
    var = []
    a, P = a1, P1
    for t in range(n):
        mu[t] = a
        var.append(P)
        a = delta + Phi @ a
        P = Phi @ P @ Phi.T + Q
    for s in range(n):
        C = var[s]
        for t in range(s, n):
            S[t, :, s, :] = C  # Cov(β_t, β_s) = Φ^{t−s} Var β_s
            S[s, :, t, :] = C.T
            C = Phi @ C
    S = S.reshape(n * M, n * M)
    mu = mu.reshape(-1)
    obs = [t for t in range(n) if not np.any(np.isnan(Y[:, t]))]
    H = np.zeros((len(obs) * N, n * M))
    for k, t in enumerate(obs):
        H[k * N:(k + 1) * N, t * M:(t + 1) * M] = Z
    y = np.concatenate([Y[:, t] for t in obs]) if obs else np.zeros(0)
    Syy = H @ S @ H.T + sig2 * np.eye(len(y))
    Sby = S @ H.T
    G = np.linalg.solve(Syy, Sby.T).T if len(y) else np.zeros((n * M, 0))
    m = mu + G @ (y - H @ mu)
    V = S - G @ Sby.T
    bs = m.reshape(n, M).T.copy()
    Vs = np.stack([V[t * M:(t + 1) * M, t * M:(t + 1) * M] for t in range(n)], axis=2)
    Cs = np.stack([V[(t + 1) * M:(t + 2) * M, t * M:(t + 1) * M] for t in range(n - 1)], axis=2) if n > 1 \
        else np.empty((M, M, 0))
    return bs, Vs, Cs


# ---- the parity rule (tests/test_gpu_states.py, factor 1) ---------------------------------------------------------
REL = 1e-9


def traj_err(x, ref, tru):
    """max over steps of |x_t − ref_t|∞ / |tru_t|∞; arrays R × steps (a covariance array is reshaped to M² × steps)."""
    if np.asarray(x).shape[-1] == 0:  # no step: the lag-one array of a one-column window
        return 0.0
    x, ref, tru = (np.asarray(v).reshape(-1, v.shape[-1]) for v in (x, ref, tru))
    scale = np.maximum(np.abs(tru).max(axis=0), 1e-300)
    return float((np.abs(x - ref).max(axis=0) / scale).max())


def rule_errors(got, checker, truth):
    return traj_err(got, checker, truth), traj_err(got, truth, truth), traj_err(checker, truth, truth)


def assert_rule(got, checker, truth, what):
    """Within 1e-9 of the FP64 checker, or at least as close to the truth as the checker is."""
    e_gc, e_gt, e_ct = rule_errors(got, checker, truth)
    print(what, f"vs checker {e_gc:.3e}  vs truth {e_gt:.3e}  checker vs truth {e_ct:.3e}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert e_gc <= REL or e_gt <= e_ct, (what, e_gc, e_gt, e_ct)
    return e_gc, e_gt, e_ct


def smoothed_yields_ref(kind, mats, theta, factors, space=0):
    Z = model_fp64(kind, mats, theta, space)[0]
    return Z @ factors


def em_moments_ref(bs, Vs, Cs):
    """S00 = Σ_{t<n}(V_t + β̂_tβ̂_t'), S11 over t = 2 … n, S10 = Σ(C_t + β̂_{t+1}β̂_t'), by explicit loops."""
    M, n = bs.shape
    S00, S11, S10 = np.zeros((M, M)), np.zeros((M, M)), np.zeros((M, M))
    for t in range(n - 1):
        S00 += Vs[:, :, t] + np.outer(bs[:, t], bs[:, t])
        S11 += Vs[:, :, t + 1] + np.outer(bs[:, t + 1], bs[:, t + 1])
        S10 += Cs[:, :, t] + np.outer(bs[:, t + 1], bs[:, t])
    return S00, S11, S10
