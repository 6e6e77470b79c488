"""Standard errors of a maximum-likelihood estimate of the DNS and TVλ models.

An extension: the reference's ``estimate!`` (optimization.jl) returns the optimum and its loss and no covariance.
The device gives the Hessian H of the log-likelihood and the OPG / HAC matrix J of its score series
(:meth:`yfm_amd.engine.Engine.loglik_info` and ``tvl_loglik_info``, include/yfm.h yfm_loglik_info_batch and
yfm_tvl_loglik_info_batch); this module turns them into
covariance matrices and standard errors with NumPy, in the unconstrained space estimation runs in and, by the delta
method, in the constrained space of ``set_params!``.
"""
from __future__ import annotations

import numpy as np

from . import params as _p

COV_KINDS = ("hessian", "opg", "sandwich")


def _batched(M, name):
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 2:
        M = M[:, :, None]
    if M.ndim != 3 or M.shape[0] != M.shape[1]:
        raise ValueError(f"{name} must be P×P or P×P×B, got {M.shape}")
    return M


def _spd_inverse(A):
    """(A⁻¹, True) by Cholesky for a symmetric positive definite A; (NaN, False) for any other matrix."""
    nan = np.full_like(A, np.nan)
    if not np.all(np.isfinite(A)):
        return nan, False
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return nan, False
    Li = np.linalg.solve(L, np.eye(A.shape[0]))
    inv = Li.T @ Li
    if not np.all(np.isfinite(inv)):
        return nan, False
    return 0.5 * (inv + inv.T), True


def covariance(H, J, kind: str = "sandwich"):
    """The covariance of θ̂ from the Hessian H of the log-likelihood and the OPG / HAC matrix J (P×P×B, or P×P for one
    candidate): ``"hessian"`` (−H)⁻¹, ``"opg"`` J⁻¹, ``"sandwich"`` H⁻¹ J H⁻¹.  The inverses are taken by Cholesky
    (of −H and of J), so a matrix that is not positive definite — a θ that is no maximum, a NaN — gives NaN for that
    candidate and ``pd[b] = False``; nothing is raised.  The matrix a kind does not use may be None.
    Returns (cov[P, P, B], pd[B])."""
    if kind not in COV_KINDS:
        raise ValueError(f"kind must be one of {COV_KINDS}, got {kind!r}")
    need_h, need_j = kind != "opg", kind != "hessian"
    if (need_h and H is None) or (need_j and J is None):
        raise ValueError(f"covariance kind {kind!r} needs {'H' if need_h and H is None else 'J'}")
    Hs = _batched(H, "H") if need_h else None
    Js = _batched(J, "J") if need_j else None
    ref = Hs if need_h else Js
    if need_h and need_j and Hs.shape != Js.shape:
        raise ValueError(f"H {Hs.shape} and J {Js.shape} differ in shape")
    P, _, B = ref.shape
    cov = np.full((P, P, B), np.nan, order="F")
    pd = np.zeros(B, dtype=bool)
    for b in range(B):
        if need_h:
            Hi, ok = _spd_inverse(-Hs[:, :, b])  # (−H)⁻¹
            if not ok:
                continue
        if kind == "hessian":
            cov[:, :, b], pd[b] = Hi, True
        elif kind == "opg":
            cov[:, :, b], pd[b] = _spd_inverse(Js[:, :, b])
        else:
            Jb = Js[:, :, b]
            # J has to be a covariance itself: positive definite, as its Cholesky factor shows
            if not _spd_inverse(Jb)[1]:
                continue
            C = Hi @ Jb @ Hi
            cov[:, :, b], pd[b] = 0.5 * (C + C.T), True
    return cov, pd


def transform_jacobian(kind: int, theta_u):
    """dθ_c/dθ_u of ``transform_params`` at θ_u (P or P×B): the transform acts entry by entry, so the Jacobian is
    diagonal — eˣ for a positive entry, 2y/(1 + y)² with y = eˣ for an entry mapped into (−1, 1), 1 elsewhere."""
    th = np.asarray(theta_u, dtype=np.float64)
    codes = _p.transform_codes(kind)
    if np.any(codes == _p.U01):
        raise NotImplementedError("transform_jacobian covers the Kalman kinds' transforms (positive, (−1, 1), identity)")
    d = np.ones_like(th)
    with np.errstate(over="ignore", invalid="ignore"):
        pos = codes == _p.POS
        d[pos] = np.exp(th[pos])
        r = codes == _p.R11
        y = np.exp(th[r])
        d[r] = 2.0 * y / ((1.0 + y) * (1.0 + y))
    return d


def delta_method(cov_u, jac):
    """cov_c = D cov_u D for the diagonal Jacobian D = diag(jac): cov_u P×P×B, jac P×B."""
    cov_u = _batched(cov_u, "cov_u")
    jac = np.asarray(jac, dtype=np.float64).reshape(cov_u.shape[0], -1)
    return np.asfortranarray(cov_u * jac[:, None, :] * jac[None, :, :])


def _se(cov):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.einsum("iib->ib", cov))


def _standard_errors(info, what, kind, refusal, model, data, theta_c, T_use, cov, lags, step) -> dict:
    from . import models as _m
    if cov not in COV_KINDS:
        raise ValueError(f"cov must be one of {COV_KINDS}, got {cov!r}")
    if model.kind != kind:
        raise NotImplementedError(f"{what} {refusal(model.kind)}")
    Th = np.asarray(theta_c, dtype=np.float64)
    if Th.ndim == 1:
        Th = Th[:, None]
    X = np.asfortranarray(_p.untransform_params(model.kind, Th))
    eng = _m._engine(model, data)
    r = getattr(eng, info)(model.kind, X, space=_p.SPACE_UNCONSTRAINED, T_use=T_use, lags=lags, step=step,
                           hessian=cov != "opg", opg=cov != "hessian")
    cov_u, pd = covariance(r["hess"], r["opg"], cov)
    cov_c = delta_method(cov_u, transform_jacobian(model.kind, X))
    return dict(cov_u=cov_u, se_u=_se(cov_u), cov_c=cov_c, se_c=_se(cov_c), ll=r["ll"], grad=r["grad"], pd=pd,
                unavailable=eng.last_grad_unavailable())


def standard_errors_batch(model, data, theta_c, T_use=None, cov: str = "sandwich", lags: int = 0, step=None) -> dict:
    """Standard errors of the DNS estimates θ_c (P×B constrained, as ``estimate_`` returns them; column b on the window
    ``data[:, :T_use[b]]``).  θ_c is untransformed and the log-likelihood's Hessian and OPG matrix (``lags`` Bartlett
    lags) are evaluated at θ_u, the space estimation runs in.  Returns cov_u, se_u there, cov_c, se_c by the delta
    method with the diagonal Jacobian of ``transform_params``, ll and grad (of +loglik, at θ_u), pd (False where the
    matrix was not positive definite: NaN covariances, no exception) and ``unavailable``, the candidates the device
    gave no matrices for.  ``cov``: "hessian", "opg" or "sandwich"."""
    def refusal(kind):
        if kind == _p.KIND_TVL:
            return (f"are built for the DNS model only (model kind {kind}): the TVλ model's are "
                    "tvl_standard_errors_batch")
        return (f"are built for the DNS model only (model kind {kind}): the "
                "other kinds have no score series, information matrix or Hessian")
    return _standard_errors("loglik_info", "standard errors", _p.KIND_DNS, refusal, model, data, theta_c, T_use, cov,
                            lags, step)


def tvl_standard_errors_batch(model, data, theta_c, T_use=None, cov: str = "sandwich", lags: int = 0,
                              step=None) -> dict:
    """:func:`standard_errors_batch` for the TVλ model (31×B constrained estimates): the same dict, from
    :meth:`yfm_amd.engine.Engine.tvl_loglik_info` and the TVλ transform's Jacobian."""
    def refusal(kind):
        return (f"are built for the TVλ model only (model kind {kind}): the DNS model's are standard_errors_batch, and "
                "the other kinds have no score series, information matrix or Hessian")
    return _standard_errors("tvl_loglik_info", "TVλ standard errors", _p.KIND_TVL, refusal, model, data, theta_c, T_use,
                            cov, lags, step)


def standard_errors_(model, data, params, **opts) -> dict:
    """:func:`standard_errors_batch` for one constrained parameter vector: the same dict without the batch axis."""
    r = standard_errors_batch(model, data, np.asarray(params, dtype=np.float64).reshape(-1, 1), **opts)
    out = {k: (v[..., 0] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    out["pd"] = bool(r["pd"][0])
    return out


def tvl_standard_errors_(model, data, params, **opts) -> dict:
    """:func:`tvl_standard_errors_batch` for one constrained parameter vector: the same dict without the batch axis."""
    r = tvl_standard_errors_batch(model, data, np.asarray(params, dtype=np.float64).reshape(-1, 1), **opts)
    out = {k: (v[..., 0] if isinstance(v, np.ndarray) else v) for k, v in r.items()}
    out["pd"] = bool(r["pd"][0])
    return out
