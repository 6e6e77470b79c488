"""Checker for the static and score-driven λ models (NS, SD-NS, RWSD-NS, SSD-NS, SRWSD-NS).

Two restatements of the reference, one text run in two arithmetics:

1. ``FLOAT`` — NumPy, Float64, line by line after the reference: ``Z'Z`` and ``Z'y`` by matrix products, the
   factorisation by ``numpy.linalg.cholesky`` inside the reference's try / ridge / −Inf structure;
2. ``TRUTH`` — the same in ``mpmath`` at 40 digits (the pattern of ``oracle/kalman_mp.py``).

Reference lines restated (paths relative to the reference root):

* ``set_params!``  src/models/msedriven/paramteroperations.jl:25-65, src/models/static/paramteroperations.jl:19-43
* transforms  src/models/msedriven/mselambda.jl:17-34, msebasemodel.jl:77-90, src/models/static/staticbasemodel.jl:48-59,
  src/utils/transformations.jl
* ``update_factor_loadings!``  src/models/msedriven/mselambda.jl:63-76, src/models/static/staticlambda.jl:46-60
* ``filter``, ``get_β_OLS!``, ``get_grad_gamma!``, ``update_gamma_with_grad!``  src/models/filter.jl:29-184
* ``get_loss``, ``get_loss_array``, ``predict``  src/models/filter.jl:209-306
* forecast blocks  src/forecasting.jl:236-250;  ``try_initializations``  src/optimization.jl:73-114 with
  ``get_new_initial_params``  src/models/msedriven/paramteroperations.jl:132-187

The score is the exact derivative 2·v'(∂Z/∂γ)β that ForwardDiff evaluates.  The parity rule is the project's:
a value passes when it is within 1e-9 relative of the FLOAT restatement or at least as close to the TRUTH as
the FLOAT restatement is (:func:`parity_ok`).
"""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

KIND_NS, KIND_SD_NS, KIND_RWSD_NS, KIND_SSD_NS, KIND_SRWSD_NS = 3, 4, 5, 6, 8
KINDS = (KIND_NS, KIND_SD_NS, KIND_RWSD_NS, KIND_SSD_NS, KIND_SRWSD_NS)
A_GUESSES = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)  # mselambda.jl:26
B_GUESSES = (0.9, 0.95, 0.98, 0.99, 0.999)         # mselambda.jl:27
FORGET = 0.98                                      # mselambda.jl:15
MP_DIGITS = 40


def is_static(kind):
    return kind == KIND_NS


def has_b(kind):
    return kind in (KIND_SD_NS, KIND_SSD_NS)


def scaled(kind):
    return kind in (KIND_SSD_NS, KIND_SRWSD_NS)


def n_params(kind):
    return 13 if is_static(kind) else (15 if has_b(kind) else 14)


class StepFailed(Exception):
    """get_β_OLS! threw twice: the step returns −Inf (filter.jl:62-67)."""


class FloatArith:
    """Float64 with NumPy / LAPACK."""
    name = "float64"
    eps = float(np.finfo(np.float64).eps)

    def num(self, x):
        return float(x)

    def vec(self, xs):
        return np.asarray([float(x) for x in xs], dtype=np.float64)

    def exp(self, x):
        with np.errstate(over="ignore", under="ignore"):
            return np.exp(x)

    def sqrt(self, x):
        return math.sqrt(x)

    def log(self, x):
        return math.log(x)

    def isnan(self, x):
        return bool(np.isnan(x))

    def isfinite(self, x):
        return bool(np.isfinite(x))

    def zeros(self, *shape):
        return np.zeros(shape)

    def chol_solve(self, G, b):
        L = np.linalg.cholesky(G)  # raises LinAlgError on a pivot that is not > 0
        return np.linalg.solve(L.T, np.linalg.solve(L, b))

    def to_float(self, x):
        return np.asarray(x, dtype=np.float64)


class MpArith:
    """mpmath at MP_DIGITS digits; vectors and matrices are NumPy object arrays of mpf."""
    name = "mp40"

    def __init__(self, digits=MP_DIGITS):
        self.digits = digits
        self.eps = mp.mpf(2) ** -52  # eps(Float64): a constant of the model, not of the arithmetic

    def num(self, x):
        return mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x

    def vec(self, xs):
        return np.asarray([self.num(x) for x in xs], dtype=object)

    def exp(self, x):
        if isinstance(x, np.ndarray):
            return np.asarray([mp.exp(v) for v in x.ravel()], dtype=object).reshape(x.shape)
        return mp.exp(x)

    def sqrt(self, x):
        return mp.sqrt(x)

    def log(self, x):
        return mp.log(x)

    def isnan(self, x):
        return bool(mp.isnan(x))

    def isfinite(self, x):
        return bool(mp.isfinite(x))

    def zeros(self, *shape):
        z = np.empty(shape, dtype=object)
        z.fill(mp.mpf(0))
        return z

    def chol_solve(self, G, b):
        n = G.shape[0]
        L = self.zeros(n, n)
        for j in range(n):
            a = G[j, j] - sum((L[j, k] * L[j, k] for k in range(j)), mp.mpf(0))
            if not (a > 0):  # LAPACK's test, NaN included
                raise np.linalg.LinAlgError("pivot")
            L[j, j] = mp.sqrt(a)
            for i in range(j + 1, n):
                L[i, j] = (G[i, j] - sum((L[i, k] * L[j, k] for k in range(j)), mp.mpf(0))) / L[j, j]
        w = self.zeros(n)
        for i in range(n):
            w[i] = (b[i] - sum((L[i, k] * w[k] for k in range(i)), mp.mpf(0))) / L[i, i]
        x = self.zeros(n)
        for i in reversed(range(n)):
            x[i] = (w[i] - sum((L[k, i] * x[k] for k in range(i + 1, n)), mp.mpf(0))) / L[i, i]
        return x

    def to_float(self, x):
        a = np.asarray(x, dtype=object)
        return np.asarray([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


FLOAT = FloatArith()
TRUTH = MpArith()


def _ctx(ar):
    return mp.workdps(ar.digits) if isinstance(ar, MpArith) else _Null()


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ---- transforms (transformations.jl) -------------------------------------------------------------------------
def transform_params(kind, theta, ar=FLOAT):
    """parameteroperations.jl:22-32 with the λ models' transform vectors."""
    th = ar.vec(theta)
    out = th.copy()
    k = 0
    if not is_static(kind):
        out[0] = ar.exp(th[0])  # from_R_to_pos
        k = 1
        if has_b(kind):
            out[1] = 1 / (1 + ar.exp(-th[1]))  # from_R_to_01
            k = 2
    phi0 = k + 4
    for d in (0, 4, 8):  # from_R_to_11 on the diagonal of Φ
        y = ar.exp(th[phi0 + d])
        out[phi0 + d] = 2 * y / (1 + y) - 1
    return out


# ---- the model (set_params!) -----------------------------------------------------------------------------------
class Model:
    pass


def update_factor_loadings(m, gamma, ar):
    """mselambda.jl:63-76 / staticlambda.jl:46-60."""
    lam = ar.num(0.01) + ar.exp(gamma)
    tau = lam * m.maturities
    z = ar.exp(-tau)
    Z = ar.zeros(m.N, 3)
    Z[:, 0] = ar.num(1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        Z[:, 1] = (1 - z) / tau
    Z[:, 2] = Z[:, 1] - z
    return Z


def dloadings_dgamma(m, gamma, ar):
    """∂Z/∂γ: what ForwardDiff propagates through update_factor_loadings! (filter.jl:172-176)."""
    e = ar.exp(gamma)
    lam = ar.num(0.01) + e
    tau = lam * m.maturities
    z = ar.exp(-tau)
    Z2 = (1 - z) / tau
    dZ = ar.zeros(m.N, 3)
    dZ[:, 1] = (z - Z2) * (e / lam)
    dZ[:, 2] = dZ[:, 1] + z * m.maturities * e
    return dZ


def set_params(kind, theta_c, maturities, ar=FLOAT):
    """msedriven/paramteroperations.jl:25-65, static/paramteroperations.jl:19-43 (θ_c: constrained)."""
    p = ar.vec(theta_c)
    assert len(p) == n_params(kind)
    m = Model()
    m.kind = kind
    m.ar = ar
    m.maturities = ar.vec(maturities)
    m.N = len(m.maturities)
    k = 0
    m.A = m.B = None
    if not is_static(kind):
        m.A = p[k]
        k += 1
        if has_b(kind):
            m.B = p[k]
            k += 1
    m.omega = p[k]
    k += 1
    m.delta = p[k:k + 3].copy()
    k += 3
    m.Phi = p[k:k + 9].reshape(3, 3, order="F").copy()  # reshape: column-major
    m.beta = m.delta.copy()
    m.gamma = m.omega
    I = ar.zeros(3, 3)
    for i in range(3):
        I[i, i] = ar.num(1.0)
    m.mu = (I - m.Phi) @ m.delta
    m.nu = (1 - m.B) * m.omega if m.B is not None else ar.num(0.0)
    m.Z = update_factor_loadings(m, m.gamma, ar)
    initialize_filter(m)
    return m


def initialize_filter(m):
    """filter.jl:19-26: the EWMA and its count are reset."""
    m.ewma = m.ar.num(0.0)
    m.count = 0


def get_beta_ols(m, y):
    """filter.jl:122-137."""
    ar = m.ar
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
    """filter.jl:52-110.  Returns the prediction; raises StepFailed where the reference returns −Inf."""
    ar = m.ar
    static = is_static(m.kind)
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
    if not static:
        v = y - m.Z @ m.beta
        g = 2 * (v @ (dloadings_dgamma(m, m.gamma, ar) @ m.beta))  # ∂(−v'v)/∂γ
        if scaled(m.kind):  # filter.jl:29-44
            f = ar.num(FORGET)
            m.ewma = f * m.ewma + (1 - f) * (g * g)
            m.count += 1
            denom = 1 - f ** m.count
            g = g / (ar.sqrt(m.ewma / denom) + ar.eps)
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


def _data(Y, ar):
    Y = np.asarray(Y, dtype=np.float64)
    if isinstance(ar, MpArith):
        return np.asarray([mp.mpf(float(v)) if v == v else mp.nan for v in Y.ravel()], dtype=object).reshape(Y.shape)
    return Y


def get_loss(kind, maturities, Y, theta, space=1, ar=FLOAT, T_use=None):
    """filter.jl:209-243, K = 1: mse/N/nobs, −Inf as soon as the running sum is not finite."""
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
            if not ar.isfinite(mse):
                return -math.inf
        return float(mse / m.N / nobs)


def get_loss_array(kind, maturities, Y, theta, space=1, ar=FLOAT, T_use=None):
    """filter.jl:245-281, K = 1: entry t = −‖y_{t+1} − pred_t‖²/N, or the scalar −Inf."""
    with _ctx(ar):
        m = _prepare(kind, maturities, theta, space, ar)
        data = _data(Y, ar)[:, :T_use] if T_use is not None else _data(Y, ar)
        nobs = data.shape[1]
        out = []
        for t in range(nobs - 1):
            try:
                pred = filter_step(m, data[:, t])
            except StepFailed:
                return -math.inf
            v = data[:, t + 1] - pred
            e = -(v @ v)
            if not ar.isfinite(e):
                return -math.inf
            out.append(float(e / m.N))
        return np.asarray(out, dtype=np.float64)


def predict(kind, maturities, Y, theta, space=1, ar=FLOAT, T_use=None, horizon=1):
    """filter.jl:284-306 on hcat(Y[:, 1:T_b], NaN × (horizon − 1)) (forecasting.jl:141).  A step that returns −Inf
    gives a −Inf prediction column and leaves the state as the failing call left it."""
    with _ctx(ar):
        m = _prepare(kind, maturities, theta, space, ar)
        Yf = np.asarray(Y, dtype=np.float64)
        if T_use is not None:
            Yf = Yf[:, :T_use]
        Yf = np.hstack([Yf, np.full((Yf.shape[0], horizon - 1), np.nan)])
        data = _data(Yf, ar)
        n = data.shape[1]
        N = m.N
        preds = np.empty((N, n))
        factors = np.empty((3, n))
        states = np.empty((1, n))
        fl1 = np.empty((N, n))
        fl2 = np.empty((N, n))
        for t in range(n):
            try:
                preds[:, t] = ar.to_float(filter_step(m, data[:, t]))
            except StepFailed:
                preds[:, t] = -np.inf
            factors[:, t] = ar.to_float(m.beta)
            states[0, t] = float(m.gamma)
            fl1[:, t] = ar.to_float(m.Z[:, 1])
            fl2[:, t] = ar.to_float(m.Z[:, 2])
        return dict(preds=preds, factors=factors, states=states, factor_loadings_1=fl1, factor_loadings_2=fl2)


def forecast(kind, maturities, Y, theta, T_use, horizon, space=1, ar=FLOAT):
    """forecasting.jl:236-250: vcat(factors, states, preds)[:, end-h+1:end]."""
    r = predict(kind, maturities, Y, theta, space, ar, T_use, horizon)
    return np.vstack([r["factors"], r["states"], r["preds"]])[:, -horizon:]


def trial_params(kind, params, trial):
    """get_new_initial_params (msedriven/paramteroperations.jl:132-187, n_unique == 1); None past the last trial."""
    nA, nB = len(A_GUESSES), (len(B_GUESSES) if has_b(kind) else 0)
    total = nA * nB if nB else nA
    if trial > total:
        return None
    p = np.array(params, dtype=np.float64)
    if nB:
        p[0] = A_GUESSES[(trial - 1) // nB]
        p[1] = B_GUESSES[(trial - 1) % nB]
    else:
        p[0] = A_GUESSES[trial - 1]
    return p


def try_initializations(kind, maturities, Y, best_params, ar=FLOAT, T_use=None):
    """optimization.jl:73-114: the sequential walk.  Returns (winner P, its loss = −get_loss)."""
    best = np.array(best_params, dtype=np.float64)
    init_loss = -get_loss(kind, maturities, Y, best, 1, ar, T_use)
    trial = best.copy()
    for k in range(1, 1001):
        p = trial_params(kind, trial, k)
        if p is None:
            break
        trial = p
        loss = -get_loss(kind, maturities, Y, p, 1, ar, T_use)
        if loss < init_loss:
            init_loss = loss
            best = p.copy()
    return best, init_loss


def parity_ok(got, ref, truth, rel=1e-9):
    """The project's rule (README): within `rel` of the Float64 restatement, or at least as close to the 40-digit
    truth as that restatement is."""
    got, ref, truth = float(got), float(ref), float(truth)
    if abs(got - ref) <= rel * abs(ref):
        return True
    return abs(got - truth) <= abs(ref - truth)
