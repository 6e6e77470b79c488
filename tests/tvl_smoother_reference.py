"""Checkers of the TVλ extended Kalman smoother (include/yfm.h yfm_tvl_smooth_batch) — test infrastructure only.

The model is the one the reference's TVλ filter! runs (filter.jl:12-80 with update_factor_loadings!, tvλdns.jl:53-64,
from initialize_filter, filter.jl:1-10), linearised once, at the forward pass's predicted states; decoding and the
loadings come from the untouched oracle modules.  Three independent statements of β̂_t = E[β_t | y_1..n], V_t and
C_t = Cov(β_{t+1}, β_t | y_1..n), none of them in the kernel's collapsed 4 × 4 form:

  (a) smooth_dense    FP64: the EKF with the N × N F_t, filtered moments, then the Rauch–Tung–Striebel gain
                      J_t = P_{t|t}Φ'P_{t+1}⁻¹; C_t = V_{t+1}J_t'.
  (b) smooth_mp       the same in 40-digit mpmath, rounded to FP64 on the way out: the truth.
  (c) smooth_joint    for tiny cases: the Gaussian conditional of the stacked (β_1 … β_n, ỹ_obs) of the linearised
                      time-varying model, with Z_t and ỹ_t = v_t + Z_ta_t taken from (a)'s forward pass — it checks the
                      backward pass and not the linearisation points.

All return (beta_s 4 × n, V_s 4 × 4 × n, C_s 4 × 4 × (n − 1)); slot t − 1 holds the quantities of column t, and
C_s[:, :, t − 1] = Cov(β_{t+1}, β_t | ·).  A column with any NaN is missing.  The forward pass of a window of n columns
is the first n steps of the whole panel's, so `forward_*` run once and `backward` serves every window.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

from oracle import kalman_mp as KM
from oracle import kalman_oracle as O
from smoother_reference import REL, assert_rule, em_moments_ref, initial_fp64, rule_errors, traj_err  # noqa: F401

KIND = O.KIND_TVL
M = 4


def model_fp64(mats, theta, space=0):
    """(state with the oracle's decoded σ², Q, δ, Φ, ready for tvl_loadings)."""
    s = O.KalmanState.fresh(KIND, mats, M)
    tc = O.transform_params(O.transform_codes(KIND, M), theta) if space == 0 else np.asarray(theta, dtype=np.float64)
    O.set_params(s, tc)
    return s


def loadings_fp64(s, a):
    """Z_t (N × 4) at the predicted state a: tvl_loadings and the Jacobian column as filter_step_tvl writes it."""
    O.tvl_loadings(s, a[3])
    dlam = s.lam - 1e-2
    m = s.maturities
    dZ1 = s.z_i / s.lam - s.z_i / ((s.lam * s.lam) * m)  # filter.jl:43, quirk kept
    dZ2 = m * s.z_i
    Z = s.Z.copy()
    Z[:, 3] = ((a[1] + a[2]) * dZ1 + a[2] * dZ2) * dlam
    return Z


def forward_dense(mats, Y, theta, space=0, n=None):
    """The FP64 EKF over the first n columns: per column a_t, P_t, a_{t|t}, P_{t|t}, Z_t and ỹ_t (None where missing)."""
    s = model_fp64(mats, theta, space)
    sig2, Q, delta, Phi = float(s.Omega_obs[0, 0]), s.Omega_state.copy(), s.delta.copy(), s.Phi.copy()
    Y = np.asarray(Y, dtype=np.float64)
    N = Y.shape[0]
    n = Y.shape[1] if n is None else int(n)
    a, P = initial_fp64(Q, delta, Phi)
    f = dict(ap=[], Pp=[], af=[], Pf=[], Z=[], yt=[], Phi=Phi, delta=delta, Q=Q, sig2=sig2)
    for t in range(n):
        y = Y[:, t]
        f["ap"].append(a)
        f["Pp"].append(P)
        Z = loadings_fp64(s, a)
        if np.any(np.isnan(y)):
            a_f, P_f = a, P
            f["yt"].append(None)
        else:
            v = y - Z[:, :3] @ a[:3]
            F = Z @ P @ Z.T + sig2 * np.eye(N)
            K = np.linalg.solve(F, Z @ P).T
            a_f = a + K @ v
            P_f = P - K @ Z @ P
            P_f = 0.5 * (P_f + P_f.T)
            f["yt"].append(v + Z @ a)
        f["Z"].append(Z)
        f["af"].append(a_f)
        f["Pf"].append(P_f)
        a = delta + Phi @ a_f
        P = Phi @ P_f @ Phi.T + Q
    return f


def backward_dense(f, n):
    """The RTS pass over the first n columns of a forward pass."""
    Phi, ap, Pp, af, Pf = f["Phi"], f["ap"], f["Pp"], f["af"], f["Pf"]
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


def smooth_dense(mats, Y, theta, space=0, n=None):
    """(a): the dense FP64 EKF and the RTS backward pass."""
    n = np.asarray(Y).shape[1] if n is None else int(n)
    return backward_dense(forward_dense(mats, Y, theta, space, n), n)


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


def forward_mp(mats, Y, theta, space=0, n=None):
    """forward_dense in 40-digit arithmetic on the same FP64 inputs."""
    _, _, sig2, Q, d, Phi = KM._decode(KIND, theta, space)
    mm = [mp.mpf(float(x)) for x in mats]
    N = len(mm)
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[1] if n is None else int(n)
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
    f = dict(ap=[], Pp=[], af=[], Pf=[], Phi=Phi)
    for t in range(n):
        y = Y[:, t]
        f["ap"].append(a)
        f["Pp"].append(P)
        if np.any(np.isnan(y)):
            a_f, P_f = a, P
        else:
            lam = mp.mpf("0.01") + mp.exp(a[3])
            dl = lam - mp.mpf("0.01")
            Z = mp.matrix(N, M)
            for i in range(N):
                s_, c_, z = KM._pair(lam, mm[i])
                dz1 = z / lam - z / (lam ** 2 * mm[i])  # filter.jl:43 as written
                dz2 = mm[i] * z
                Z[i, 0], Z[i, 1], Z[i, 2] = 1, s_, c_
                Z[i, 3] = ((a[1] + a[2]) * dz1 + a[2] * dz2) * dl
            v = mp.matrix(y.tolist()) - Z[:, :3] * mp.matrix([a[0], a[1], a[2]])
            F = Z * P * Z.T + sig2 * mp.eye(N)
            K = _mp_solve(F, Z * P).T
            a_f = a + K * v
            P_f = P - K * Z * P
        f["af"].append(a_f)
        f["Pf"].append(P_f)
        a = d + Phi * a_f
        P = Phi * P_f * Phi.T + Q
    return f


def backward_mp(f, n):
    Phi, ap, Pp, af, Pf = f["Phi"], f["ap"], f["Pp"], f["af"], f["Pf"]
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


def smooth_mp(mats, Y, theta, space=0, n=None):
    """(b): smooth_dense in 40-digit arithmetic on the same FP64 inputs."""
    n = np.asarray(Y).shape[1] if n is None else int(n)
    return backward_mp(forward_mp(mats, Y, theta, space, n), n)


def smooth_mp_windows(mats, Y, theta, space, windows):
    """smooth_mp on several windows of one panel: one forward pass."""
    f = forward_mp(mats, Y, theta, space, max(windows))
    return [backward_mp(f, int(n)) for n in windows]


def smooth_joint(mats, Y, theta, space=0, n=None):
    """(c): E and Cov of (β_1 … β_n) given the observed columns of the linearised model ỹ_t = Z_tβ_t + ε_t, from the joint
    Gaussian; Z_t and ỹ_t come from forward_dense.  Tiny cases only."""
    n = np.asarray(Y).shape[1] if n is None else int(n)
    f = forward_dense(mats, Y, theta, space, n)
    Phi, delta, Q, sig2 = f["Phi"], f["delta"], f["Q"], f["sig2"]
    N = np.asarray(Y).shape[0]
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
    obs = [t for t in range(n) if f["yt"][t] is not None]
    H = np.zeros((len(obs) * N, n * M))
    for k, t in enumerate(obs):
        H[k * N:(k + 1) * N, t * M:(t + 1) * M] = f["Z"][t]
    y = np.concatenate([f["yt"][t] for t in obs]) if obs else np.zeros(0)
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


def smoothed_yields_ref(mats, factors):
    """Column t = Z(λ̂_t)[:, 1:3]·β̂_t[1:3], λ̂_t = 0.01 + exp(β̂_{4,t}), by an explicit loop over the oracle's loadings."""
    s = O.KalmanState.fresh(KIND, mats, M)
    out = np.full((len(s.maturities), factors.shape[1]), np.nan)
    for t in range(factors.shape[1]):
        if np.isfinite(factors[:, t]).all():
            O.tvl_loadings(s, factors[3, t])
            out[:, t] = s.Z[:, :3] @ factors[:3, t]
    return out
