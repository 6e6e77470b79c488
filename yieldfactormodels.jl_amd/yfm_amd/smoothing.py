"""The fixed-interval Kalman smoother of the fixed-loading models (DNS, GNS5).

An extension: the reference's ``predict`` (src/models/kalman/filter.jl:250-282) returns the forecasts a_{t+1|t} only.
The device gives β̂_t = E[β_t | y_1..n], its covariance V_t and the lag-one covariance C_t = Cov(β_{t+1}, β_t | y_1..n)
(:meth:`yfm_amd.engine.Engine.smooth`, include/yfm.h yfm_smooth_batch); this module wraps it in the model API and adds,
with NumPy, the fitted curves Zβ̂_t and the moment sums an EM step needs.
"""
from __future__ import annotations

import numpy as np

from . import params as _p

SMOOTH_KINDS = (_p.KIND_DNS, _p.KIND_GNS)


def _check_kind(kind, what):
    if kind in SMOOTH_KINDS:
        return
    gap = ("the TVλ model's extended smoother is tvl_smooth_batch" if kind == _p.KIND_TVL
           else "the λ and neural kinds are not Kalman filters and have no state covariance to smooth")
    raise NotImplementedError(f"{what} is built for the DNS and GNS5 models only (model kind {kind}): {gap}")


def smooth_batch(model, data, theta_c, T_use=None) -> dict:
    """The smoothed states of the estimates θ_c (P×B constrained, as ``estimate_`` returns them; column b on the window
    ``data[:, :T_use[b]]``).  Returns ``factors`` (M, T, B: β̂_t in slot t − 1), ``cov`` (M, M, T, B: V_t),
    ``lag_one_cov`` (M, M, T − 1, B: C_t = Cov(β_{t+1}, β_t | y_1..n) in slot t − 1) — NaN beyond a window — and
    ``available`` (B,): False where the device gave no states (a loglik of −Inf or NaN, a candidate evaluated on the
    double-double path, an output that is not finite), whose arrays are NaN throughout."""
    from . import models as _m
    _check_kind(model.kind, "smooth_batch")
    Th = np.asarray(theta_c, dtype=np.float64)
    if Th.ndim == 1:
        Th = Th[:, None]
    eng = _m._engine(model, data)
    bs, Vs, Cs = eng.smooth(model.kind, np.asfortranarray(Th), space=_p.SPACE_CONSTRAINED, T_use=T_use)
    return dict(factors=bs, cov=Vs, lag_one_cov=Cs, available=np.isfinite(bs[0, 0, :]))


def smooth_(model, data, params) -> dict:
    """:func:`smooth_batch` for one constrained parameter vector: the same dict without the batch axis."""
    r = smooth_batch(model, data, np.asarray(params, dtype=np.float64).reshape(-1, 1))
    out = {k: v[..., 0] for k, v in r.items()}
    out["available"] = bool(r["available"][0])
    return out


def _check_tvl(kind, what):
    if kind == _p.KIND_TVL:
        return
    gap = ("the fixed-loading models' smoother is smooth_batch" if kind in SMOOTH_KINDS
           else "the λ and neural kinds are not Kalman filters: there is nothing to smooth")
    raise NotImplementedError(f"{what} is built for the TVλ model only (model kind {kind}): {gap}")


def lambda_path(factors, cov):
    """(λ̂, its standard deviation) from TVλ smoothed arrays (4, T[, B]) and (4, 4, T[, B]): λ̂_t = 0.01 + exp(β̂₄,ₜ) and,
    by the delta method, sd λ̂_t = (λ̂_t − 0.01)·√V₄₄,ₜ.  NaN where the inputs are."""
    f = np.asarray(factors, dtype=np.float64)
    V = np.asarray(cov, dtype=np.float64)
    e = np.exp(f[3])
    with np.errstate(invalid="ignore"):
        return 0.01 + e, e * np.sqrt(V[3, 3])


def tvl_smooth_batch(model, data, theta_c, T_use=None) -> dict:
    """The extended Kalman smoother of the TVλ model at the estimates θ_c (31×B constrained; column b on the window
    ``data[:, :T_use[b]]``), linearised once at the forward pass's predicted states (include/yfm.h
    yfm_tvl_smooth_batch).  Returns the dict of :func:`smooth_batch` — ``factors`` (4, T, B), ``cov`` (4, 4, T, B),
    ``lag_one_cov`` (4, 4, T − 1, B), ``available`` (B,) — and the path of the decay parameter given all the data:
    ``lambda_`` (T, B), λ̂_t = 0.01 + exp(β̂₄,ₜ), and ``lambda_sd`` (T, B), its delta-method standard deviation
    (λ̂_t − 0.01)·√V₄₄,ₜ."""
    from . import models as _m
    _check_tvl(model.kind, "tvl_smooth_batch")
    Th = np.asarray(theta_c, dtype=np.float64)
    if Th.ndim == 1:
        Th = Th[:, None]
    eng = _m._engine(model, data)
    bs, Vs, Cs = eng.tvl_smooth(model.kind, np.asfortranarray(Th), space=_p.SPACE_CONSTRAINED, T_use=T_use)
    lam, sd = lambda_path(bs, Vs)
    return dict(factors=bs, cov=Vs, lag_one_cov=Cs, available=np.isfinite(bs[0, 0, :]), lambda_=lam, lambda_sd=sd)


def tvl_smooth_(model, data, params) -> dict:
    """:func:`tvl_smooth_batch` for one constrained parameter vector: the same dict without the batch axis."""
    r = tvl_smooth_batch(model, data, np.asarray(params, dtype=np.float64).reshape(-1, 1))
    out = {k: v[..., 0] for k, v in r.items()}
    out["available"] = bool(r["available"][0])
    return out


def tvl_smoothed_yields(model, factors) -> np.ndarray:
    """The fitted curves of the TVλ model (N × T) from one candidate's ``factors`` (4 × T): column t is
    Z(λ̂_t)[:, 1:3]·β̂_t[1:3] with λ̂_t = 0.01 + exp(β̂₄,ₜ) (tvλdns.jl:53-64); NaN columns stay NaN."""
    _check_tvl(model.kind, "tvl_smoothed_yields")
    f = np.asarray(factors, dtype=np.float64)
    m = np.asarray(model.base.maturities, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        tau = (0.01 + np.exp(f[3]))[None, :] * m
        z = np.exp(-tau)
        s = (1.0 - z) / tau
        return f[0][None, :] + s * f[1][None, :] + (s - z) * f[2][None, :]


def loadings(model, theta_c) -> np.ndarray:
    """Z (N × M) of a fixed-loading model at the constrained θ_c: [1, S(λ₁), C(λ₁) (, S(λ₂), C(λ₂))], λ = 0.01 + e^γ
    (dns.jl:51-65; the GNS5 extension takes two γ)."""
    _check_kind(model.kind, "loadings")
    th = np.asarray(theta_c, dtype=np.float64)
    m = np.asarray(model.base.maturities, dtype=np.float64)
    M = _p.state_dim(model.kind)
    Z = np.ones((len(m), M))
    for l in range((M - 1) // 2):
        tau = (0.01 + np.exp(th[l])) * m
        z = np.exp(-tau)
        Z[:, 1 + 2 * l] = (1.0 - z) / tau
        Z[:, 2 + 2 * l] = Z[:, 1 + 2 * l] - z
    return Z


def smoothed_yields(model, theta_c, factors) -> np.ndarray:
    """The fitted curves Zβ̂_t (N × T) from one candidate's ``factors`` (M × T); NaN columns stay NaN."""
    return loadings(model, theta_c) @ np.asarray(factors, dtype=np.float64)


def em_moments(factors, cov, lag_one_cov, n: int) -> dict:
    """The second-moment sums of an EM step over a window of n columns, from one candidate's smoothed arrays:
    S00 = Σ_{t=1}^{n−1} (V_t + β̂_tβ̂_t'), S11 = Σ_{t=2}^{n} (V_t + β̂_tβ̂_t'), S10 = Σ_{t=1}^{n−1} (C_t + β̂_{t+1}β̂_t')."""
    b = np.asarray(factors, dtype=np.float64)[:, :n]
    V = np.asarray(cov, dtype=np.float64)[:, :, :n]
    C = np.asarray(lag_one_cov, dtype=np.float64)[:, :, :max(n - 1, 0)]
    outer = np.einsum("it,jt->ijt", b, b)
    S = V + outer
    return dict(S00=S[:, :, :n - 1].sum(axis=2), S11=S[:, :, 1:].sum(axis=2),
                S10=(C + np.einsum("it,jt->ijt", b[:, 1:], b[:, :n - 1])).sum(axis=2))
