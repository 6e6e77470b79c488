"""Checker for the neural Nelson–Siegel models (NNS, NNS-Anchored and the 24 score-driven NNS kinds).

One text run in two arithmetics, as ``tests/msed_reference.py`` (whose arithmetics, ``StepFailed`` and ``parity_ok``
it reuses): ``FLOAT`` — NumPy Float64 — and ``TRUTH`` — mpmath at 40 digits.

Reference lines restated (paths relative to the reference root):

* ``set_params!``  src/models/msedriven/paramteroperations.jl:25-65, src/models/static/paramteroperations.jl:19-43
* duplicator and transforms  src/models/msedriven/mseneural.jl:24-57, msebasemodel.jl:77-90
* networks  src/models/msedriven/mseneural.jl:120-163, src/models/static/staticneural.jl:81-110
* loading transforms  src/utils/neural_network_transform.jl (quirks included: the "last" of Z₂ is index n−1, the
  intercept of Z₃ enters with the sign as written)
* ``filter``, ``get_β_OLS!``, ``update_gamma_with_grad!``  src/models/filter.jl:29-137 (forget factor 0.9)
* ``get_loss``, ``get_loss_array``, ``predict``  src/models/filter.jl:209-306;  forecast blocks
  src/forecasting.jl:236-250;  ``try_initializations``  src/optimization.jl:73-114 with the multi-unique branch of
  ``get_new_initial_params``  src/models/msedriven/paramteroperations.jl:161-184

The score is the exact derivative ∂(−‖y − Z(γ)β‖²)/∂γ that ForwardDiff evaluates (filter.jl:168-184), written out
by back-propagation through the transform and the two networks (:func:`score`); ``tanh`` is the mathematical
function.
"""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from msed_reference import FLOAT, TRUTH, MpArith, StepFailed, _ctx, _data, parity_ok  # noqa: F401

KIND_NNS, KIND_NNS_ANCHORED = 16, 17
A_GUESSES = (1e-6, 1e-5, 1e-4, 1e-3)     # mseneural.jl:59
B_GUESSES = (0.97, 0.98, 0.99, 0.999)    # mseneural.jl:60
FORGET = 0.9                             # mseneural.jl:24
SCALE = 0.9610
G = 18


def sd_kind(dyn, random_walk=False, scaled=False, anchored=False):
    """include/yfm.h: 32 | dyn | RW<<2 | SCALED<<3 | ANCHORED<<4, dyn = 0 scalar, 1 block_diag, 2 diag."""
    return 32 | dyn | (int(random_walk) << 2) | (int(scaled) << 3) | (int(anchored) << 4)


def all_kinds():
    out = [KIND_NNS, KIND_NNS_ANCHORED]
    for anc in (False, True):
        for sc in (False, True):
            for dyn in (0, 1, 2):
                for rw in (False, True):
                    out.append(sd_kind(dyn, rw, sc, anc))
    return out


def is_static(kind):
    return kind in (KIND_NNS, KIND_NNS_ANCHORED)


def is_anchored(kind):
    return kind == KIND_NNS_ANCHORED if is_static(kind) else bool((kind >> 4) & 1)


def has_b(kind):
    return not is_static(kind) and not (kind >> 2) & 1


def scaled(kind):
    return not is_static(kind) and bool((kind >> 3) & 1)


def n_unique(kind):
    return 0 if is_static(kind) else (2, 6, 18)[kind & 3]


def duplicator(kind):
    """mseneural.jl:33-48 (0-based)."""
    return np.arange(G) // (9, 3, 1)[kind & 3]


def n_params(kind):
    return n_unique(kind) * (2 if has_b(kind) else 1) + 30


def _tanh(ar, x):
    if isinstance(ar, MpArith):
        return np.asarray([mp.tanh(v) for v in x], dtype=object)
    return np.tanh(x)


def transform_params(kind, theta, ar=FLOAT):
    th = ar.vec(theta)
    out = th.copy()
    nu = n_unique(kind)
    for k in range(nu):
        out[k] = ar.exp(th[k])  # from_R_to_pos
    k = nu
    if has_b(kind):
        for j in range(nu):
            out[nu + j] = 1 / (1 + ar.exp(-th[nu + j]))  # from_R_to_01
        k = 2 * nu
    phi0 = k + G + 3
    for d in (0, 4, 8):
        y = ar.exp(th[phi0 + d])
        out[phi0 + d] = 2 * y / (1 + y) - 1
    return out


class Model:
    pass


def net(m, g):
    """Chain(Dense(1 => 3, tanh), Dense(3, 1; use_bias = false)) at every maturity: (raw (N), τ (N×3))."""
    ar = m.ar
    tau = ar.zeros(m.N, 3)
    raw = ar.zeros(m.N)
    for h in range(3):
        tau[:, h] = _tanh(ar, g[h] * m.maturities + g[3 + h])
        raw = raw + g[6 + h] * tau[:, h]
    return raw, tau


def update_factor_loadings(m, gamma, ar, keep=False):
    """mseneural.jl:137-163 with transform_net_1! / transform_net_2! (neural_network_transform.jl)."""
    n = m.N
    x = m.maturities
    raw2, tau2 = net(m, gamma[:9])
    raw3, tau3 = net(m, gamma[9:])
    Z = ar.zeros(n, 3)
    Z[:, 0] = ar.num(1.0)
    k = Model()
    with np.errstate(all="ignore"):
        if not m.anchored:
            last = raw2[n - 2]
            k.iu = 1 / (raw2[0] - last + ar.num(1e-7))
            k.t = (raw2 - last) * k.iu
            slope = (raw3[n - 1] - raw3[0]) / (x[n - 1] - x[0])
            icpt = raw3[0] - slope * x[0]
            k.r = raw3 - (slope * x - icpt)
        else:
            k.iu = ar.num(1.0)
            k.t = raw2
            k.r = raw3
        k.q = k.r * k.r
        Q = ar.num(0.0)
        for i in range(1, n - 1):
            Q = Q + k.q[i] * k.q[i]
        k.Q = Q
        rq = ar.sqrt(Q)
        if not m.anchored:
            k.sc = 1 / (rq / ar.num(SCALE) + ar.num(1e-7))
            k.kap = k.sc * k.sc / (ar.num(SCALE) * rq) if rq != 0 else ar.num(math.inf)
        else:
            k.sc = (ar.num(SCALE) / rq if rq != 0 else ar.num(math.inf)) + ar.num(1e-7)
            k.kap = ar.num(SCALE) / (Q * rq) if rq != 0 else ar.num(math.inf)
        Z[0, 1] = ar.num(1.0)
        for i in range(1, n - 2):
            Z[i, 1] = k.t[i] * k.t[i]
        for i in range(1, n - 1):
            Z[i, 2] = k.q[i] * k.sc
    if keep:
        k.tau2, k.tau3 = tau2, tau3
        return Z, k
    return Z


def _dnet(m, g, tau, c):
    """Σᵢ cᵢ·∂rawᵢ/∂g for one block."""
    ar = m.ar
    out = ar.zeros(9)
    for h in range(3):
        w = c * g[6 + h] * (1 - tau[:, h] * tau[:, h])
        out[h] = w @ m.maturities
        out[3 + h] = w.sum()
        out[6 + h] = c @ tau[:, h]
    return out


def score(m, gamma, beta, y):
    """∂(−‖y − Z(γ)β‖²)/∂γ (filter.jl:168-184)."""
    ar = m.ar
    n = m.N
    x = m.maturities
    with np.errstate(all="ignore"):
        Z, k = update_factor_loadings(m, gamma, ar, keep=True)
        v = y - Z @ beta
        a2 = 2 * beta[1] * v
        a3 = 2 * beta[2] * v
        zero = ar.zeros(n)
        # Z₂
        c2 = zero.copy()
        d = 2 * a2 * k.t
        for i in range(1, n - 2):
            c2[i] = d[i] * k.iu
        if not m.anchored:
            for i in range(1, n - 2):
                c2[n - 2] = c2[n - 2] + d[i] * (k.t[i] - 1) * k.iu
                c2[0] = c2[0] - d[i] * k.t[i] * k.iu
        # Z₃
        S = ar.num(0.0)
        for i in range(1, n - 1):
            S = S + a3[i] * k.q[i]
        c3 = zero.copy()
        for i in range(1, n - 1):
            c3[i] = 2 * k.r[i] * (a3[i] * k.sc - S * k.kap * k.q[i])
        if not m.anchored:
            r0 = ar.num(0.0)
            r1 = ar.num(0.0)
            for i in range(1, n - 1):
                r0 = r0 + c3[i]
                r1 = r1 + x[i] * c3[i]
            cn = (-r1 - x[0] * r0) / (x[n - 1] - x[0])
            c3[n - 1] = c3[n - 1] + cn
            c3[0] = c3[0] + (r0 - cn)
        g = ar.zeros(G)
        g[:9] = _dnet(m, gamma[:9], k.tau2, c2)
        g[9:] = _dnet(m, gamma[9:], k.tau3, c3)
    return g


def set_params(kind, theta_c, maturities, ar=FLOAT):
    p = ar.vec(theta_c)
    assert len(p) == n_params(kind)
    m = Model()
    m.kind, m.ar = kind, ar
    m.anchored = is_anchored(kind)
    m.maturities = ar.vec(maturities)
    m.N = len(m.maturities)
    nu = n_unique(kind)
    k = 0
    m.A = m.B = None
    if not is_static(kind):
        dup = duplicator(kind)
        m.A = p[:nu][dup]
        k = nu
        if has_b(kind):
            m.B = p[nu:2 * nu][dup]
            k = 2 * nu
    m.omega = p[k:k + G].copy()
    k += G
    m.delta = p[k:k + 3].copy()
    k += 3
    m.Phi = p[k:k + 9].reshape(3, 3, order="F").copy()
    m.beta = m.delta.copy()
    m.gamma = m.omega.copy()
    I = ar.zeros(3, 3)
    for i in range(3):
        I[i, i] = ar.num(1.0)
    m.mu = (I - m.Phi) @ m.delta
    m.nu = (1 - m.B) * m.omega if m.B is not None else None
    m.Z = update_factor_loadings(m, m.gamma, ar)
    m.ewma = ar.zeros(G)
    m.count = 0
    return m


def get_beta_ols(m, y):
    """filter.jl:122-137."""
    ar = m.ar
    with np.errstate(all="ignore"):
        ZtZ = m.Z.T @ m.Z
        Zty = m.Z.T @ y
    try:
        return ar.chol_solve(ZtZ, Zty)
    except np.linalg.LinAlgError:
        ZtZ = ZtZ.copy()
        for i in range(3):
            ZtZ[i, i] = ZtZ[i, i] + ar.num(1e-3)
        return ar.chol_solve(ZtZ, Zty)


def filter_step(m, y):
    """filter.jl:52-110; raises StepFailed where the reference returns −Inf."""
    ar = m.ar
    with np.errstate(all="ignore"):
        if ar.isnan(y[0]):
            if m.B is not None:
                m.gamma = m.nu + m.B * m.gamma
                m.Z = update_factor_loadings(m, m.gamma, ar)
            m.beta = m.mu + m.Phi @ m.beta
            return m.Z @ m.beta
        try:
            m.beta = get_beta_ols(m, y)
        except np.linalg.LinAlgError:
            raise StepFailed
        if not is_static(m.kind):
            g = score(m, m.gamma, m.beta, y)
            if scaled(m.kind):
                f = ar.num(FORGET)
                m.ewma = f * m.ewma + (1 - f) * (g * g)
                m.count += 1
                denom = 1 - f ** m.count
                g = ar.vec([g[k] / (ar.sqrt(m.ewma[k] / denom) + ar.eps) for k in range(G)])
            m.gamma = m.gamma + g * m.A
            m.Z = update_factor_loadings(m, m.gamma, ar)
            try:
                m.beta = get_beta_ols(m, y)
            except np.linalg.LinAlgError:
                raise StepFailed
            if m.B is not None:
                m.gamma = m.nu + m.B * m.gamma
                m.Z = update_factor_loadings(m, m.gamma, ar)
        m.beta = m.mu + m.Phi @ m.beta
        return m.Z @ m.beta


def _prepare(kind, maturities, theta, space, ar):
    th = transform_params(kind, theta, ar) if space == 0 else ar.vec(theta)
    return set_params(kind, th, maturities, ar)


def _isfin(ar, x):
    return ar.isfinite(x)


def get_loss(kind, maturities, Y, theta, space=1, ar=FLOAT, T_use=None):
    """filter.jl:209-243, K = 1."""
    with _ctx(ar):
        m = _prepare(kind, maturities, theta, space, ar)
        data = _data(Y, ar)[:, :T_use] if T_use is not None else _data(Y, ar)
        nobs = data.shape[1]
        mse = ar.num(0.0)
        for t in range(nobs - 1):
            try:
                pred = filter_step(m, data[:, t])
            except StepFailed:
                return -math.inf
            v = data[:, t + 1] - pred
            mse = mse - v @ v
            if not _isfin(ar, mse):
                return -math.inf
        return float(mse / m.N / nobs)


def get_loss_array(kind, maturities, Y, theta, space=1, ar=FLOAT, T_use=None):
    """filter.jl:245-281, K = 1."""
    with _ctx(ar):
        m = _prepare(kind, maturities, theta, space, ar)
        data = _data(Y, ar)[:, :T_use] if T_use is not None else _data(Y, ar)
        out = []
        for t in range(data.shape[1] - 1):
            try:
                pred = filter_step(m, data[:, t])
            except StepFailed:
                return -math.inf
            v = data[:, t + 1] - pred
            e = -(v @ v)
            if not _isfin(ar, e):
                return -math.inf
            out.append(float(e / m.N))
        return np.asarray(out, dtype=np.float64)


def predict(kind, maturities, Y, theta, space=1, ar=FLOAT, T_use=None, horizon=1):
    """filter.jl:284-306 on hcat(Y[:, 1:T_b], NaN × (horizon − 1))."""
    with _ctx(ar):
        m = _prepare(kind, maturities, theta, space, ar)
        Yf = np.asarray(Y, dtype=np.float64)
        if T_use is not None:
            Yf = Yf[:, :T_use]
        Yf = np.hstack([Yf, np.full((Yf.shape[0], horizon - 1), np.nan)])
        data = _data(Yf, ar)
        n, N = data.shape[1], m.N
        preds, fl1, fl2 = np.empty((N, n)), np.empty((N, n)), np.empty((N, n))
        factors, states = np.empty((3, n)), np.empty((G, n))
        for t in range(n):
            try:
                preds[:, t] = ar.to_float(filter_step(m, data[:, t]))
            except StepFailed:
                preds[:, t] = -np.inf
            factors[:, t] = ar.to_float(m.beta)
            states[:, t] = ar.to_float(m.gamma)
            fl1[:, t] = ar.to_float(m.Z[:, 1])
            fl2[:, t] = ar.to_float(m.Z[:, 2])
        return dict(preds=preds, factors=factors, states=states, factor_loadings_1=fl1, factor_loadings_2=fl2)


def forecast(kind, maturities, Y, theta, T_use, horizon, space=1, ar=FLOAT):
    """forecasting.jl:236-250: vcat(factors, states, preds)[:, end-h+1:end]."""
    r = predict(kind, maturities, Y, theta, space, ar, T_use, horizon)
    return np.vstack([r["factors"], r["states"], r["preds"]])[:, -horizon:]


def loss_at_gamma(kind, maturities, gamma, beta, y, ar=TRUTH):
    """−‖y − Z(γ)β‖² — the function get_grad_gamma! differentiates (for the central-difference check)."""
    m = Model()
    m.ar, m.anchored = ar, is_anchored(kind)
    m.maturities = ar.vec(maturities)
    m.N = len(m.maturities)
    Z = update_factor_loadings(m, gamma, ar)
    v = y - Z @ beta
    return -(v @ v)


def trial_params(kind, params, trial):
    """get_new_initial_params, the multi-unique branch (msedriven/paramteroperations.jl:161-184); None past the
    last trial."""
    nA, nB = len(A_GUESSES), (len(B_GUESSES) if has_b(kind) else 0)
    nu = n_unique(kind)
    half = nu // 2
    total = nA ** 2 * nB ** 2 if nB else nA ** 2
    if trial > total:
        return None
    p = np.array(params, dtype=np.float64)
    if nB:
        a1 = (trial - 1) // (nA * nB ** 2)
        rem = (trial - 1) % (nA * nB ** 2)
        a2 = rem // nB ** 2
        rem = rem % nB ** 2
        b1, b2 = rem // nB, rem % nB
        p[:half] = A_GUESSES[a1]
        p[half:nu] = A_GUESSES[a2]
        p[nu:nu + half] = B_GUESSES[b1]
        p[nu + half:2 * nu] = B_GUESSES[b2]
    else:
        p[:half] = A_GUESSES[(trial - 1) // nA]
        p[half:nu] = A_GUESSES[(trial - 1) % nA]
    return p


def try_initializations(kind, maturities, Y, best_params, ar=FLOAT, T_use=None):
    """optimization.jl:73-114: the sequential walk.  Returns (winner, its loss = −get_loss, winner's trial index,
    0 for the start)."""
    best = np.array(best_params, dtype=np.float64)
    init_loss = -get_loss(kind, maturities, Y, best, 1, ar, T_use)
    trial = best.copy()
    k_best = 0
    for k in range(1, 1001):
        p = trial_params(kind, trial, k)
        if p is None:
            break
        trial = p
        loss = -get_loss(kind, maturities, Y, p, 1, ar, T_use)
        if loss < init_loss:
            init_loss, best, k_best = loss, p.copy(), k
    return best, init_loss, k_best
