"""Second checker for the neural models' full loss gradient: the filter of ``tests/msedn_reference.py`` restated on
torch Float64 tensors (CPU), its gradient with respect to every row of θ from ``torch.autograd`` — reverse-mode
differentiation of the restated text, an algorithm that shares nothing with the hand-written adjoint of
``csrc/yfm_msedn_adj.hpp``.

What is differentiated is the function get_loss computes (filter.jl:209-243, K = 1): the score is the exact partial
derivative ∂(−‖y − Z(γ)β‖²)/∂γ at fixed β written out as in :func:`msedn_reference.score` (so autograd sees β inside
it, as get_loss's value does), and both OLS fits are differentiated through.  The ridge retry of get_β_OLS!
(filter.jl:128-135) is restated; ``tanh`` is torch's.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import msedn_reference as R

F64 = torch.float64
EPS = 2.220446049250313e-16


def _net(x, g):
    """raw (N) and τ (N×3) of one block g = [w₁(3), b(3), w₂(3)]."""
    tau = torch.tanh(x[:, None] * g[None, 0:3] + g[None, 3:6])
    return tau @ g[6:9], tau


class _Load:
    pass


def loadings(x, gamma, anchored):
    """update_factor_loadings (mseneural.jl:137-163 with neural_network_transform.jl) → Z (N×3) and what the score
    needs."""
    n = x.shape[0]
    raw2, tau2 = _net(x, gamma[:9])
    raw3, tau3 = _net(x, gamma[9:])
    k = _Load()
    k.tau2, k.tau3 = tau2, tau3
    idx = torch.arange(n)
    k.in2 = ((idx >= 1) & (idx <= n - 3)).to(F64)
    k.in3 = ((idx >= 1) & (idx <= n - 2)).to(F64)
    if not anchored:
        last = raw2[n - 2]
        k.iu = 1 / (raw2[0] - last + 1e-7)
        k.t = (raw2 - last) * k.iu
        slope = (raw3[n - 1] - raw3[0]) / (x[n - 1] - x[0])
        icpt = raw3[0] - slope * x[0]
        k.r = raw3 - (slope * x - icpt)
    else:
        k.iu = torch.ones((), dtype=F64)
        k.t = raw2
        k.r = raw3
    k.q = k.r * k.r
    Q = (k.in3 * k.q * k.q).sum()
    rq = torch.sqrt(Q)
    if not anchored:
        k.sc = 1 / (rq / R.SCALE + 1e-7)
        k.kap = k.sc * k.sc / (R.SCALE * rq)
    else:
        k.sc = R.SCALE / rq + 1e-7
        k.kap = R.SCALE / (Q * rq)
    e0 = (idx == 0).to(F64)
    Z = torch.stack([torch.ones(n, dtype=F64), e0 + k.in2 * k.t * k.t, k.in3 * k.q * k.sc], dim=1)
    return Z, k


def _dnet(x, g, tau, c):
    w = c[:, None] * g[None, 6:9] * (1 - tau * tau)
    return torch.cat([x @ w, w.sum(0), c @ tau])


def score(x, gamma, beta, y, anchored):
    """∂(−‖y − Z(γ)β‖²)/∂γ at fixed β (filter.jl:168-184), as msedn_reference.score writes it."""
    n = x.shape[0]
    Z, k = loadings(x, gamma, anchored)
    v = y - Z @ beta
    a2 = 2 * beta[1] * v
    a3 = 2 * beta[2] * v
    d = 2 * a2 * k.t * k.in2
    c2 = d * k.iu
    if not anchored:
        e_last = torch.zeros(n, dtype=F64)
        e_last[n - 2] = 1.0
        e_first = torch.zeros(n, dtype=F64)
        e_first[0] = 1.0
        c2 = c2 + e_last * (d * (k.t - 1)).sum() * k.iu - e_first * (d * k.t).sum() * k.iu
    S = (k.in3 * a3 * k.q).sum()
    c3 = k.in3 * 2 * k.r * (a3 * k.sc - S * k.kap * k.q)
    if not anchored:
        r0 = c3.sum()
        r1 = (x * c3).sum()
        cn = (-r1 - x[0] * r0) / (x[n - 1] - x[0])
        e_n = torch.zeros(n, dtype=F64)
        e_n[n - 1] = 1.0
        c3 = c3 + e_n * cn + e_first * (r0 - cn)
    return torch.cat([_dnet(x, gamma[:9], k.tau2, c2), _dnet(x, gamma[9:], k.tau3, c3)])


class StepFailed(Exception):
    pass


def _ols(Z, y):
    """get_β_OLS! (filter.jl:122-137)."""
    G = Z.T @ Z
    _, info = torch.linalg.cholesky_ex(G.detach())
    if int(info) != 0:
        G = G + 1e-3 * torch.eye(3, dtype=F64)
        _, info = torch.linalg.cholesky_ex(G.detach())
        if int(info) != 0:
            raise StepFailed
    return torch.linalg.solve(G, Z.T @ y)


def transform(kind, th):
    """θ unconstrained → constrained (msedn_reference.transform_params)."""
    nu = R.n_unique(kind)
    parts = []
    if nu:
        parts.append(torch.exp(th[:nu]))
    k = nu
    if R.has_b(kind):
        parts.append(1 / (1 + torch.exp(-th[nu:2 * nu])))
        k = 2 * nu
    parts.append(th[k:k + R.G + 3])
    phi = th[k + R.G + 3:]
    y = torch.exp(phi)
    diag = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], dtype=F64)
    parts.append(diag * (2 * y / (1 + y) - 1) + (1 - diag) * phi)
    return torch.cat(parts)


def loss_tensor(kind, maturities, Y, th, space, T_use=None):
    """get_loss (filter.jl:209-243, K = 1) of the tensor θ as a tensor in its graph; −inf (a float) where it fails."""
    x = torch.as_tensor(np.asarray(maturities, dtype=np.float64))
    Yn = np.asarray(Y, dtype=np.float64)
    if T_use is not None:
        Yn = Yn[:, :int(T_use)]
    data = torch.as_tensor(np.nan_to_num(Yn, nan=0.0))
    N, nobs = Yn.shape
    tc = transform(kind, th) if space == 0 else th
    anchored, static, hasb, scaled = R.is_anchored(kind), R.is_static(kind), R.has_b(kind), R.scaled(kind)
    nu = R.n_unique(kind)
    dup = torch.as_tensor(R.duplicator(kind))
    k = 0
    A = B = None
    if not static:
        A = tc[:nu][dup]
        k = nu
        if hasb:
            B = tc[nu:2 * nu][dup]
            k = 2 * nu
    omega = tc[k:k + R.G]
    delta = tc[k + R.G:k + R.G + 3]
    Phi = tc[k + R.G + 3:].reshape(3, 3).T
    mu = (torch.eye(3, dtype=F64) - Phi) @ delta
    nuv = (1 - B) * omega if hasb else None
    gamma, beta = omega, delta
    ewma, count = torch.zeros(R.G, dtype=F64), 0
    mse = torch.zeros((), dtype=F64)
    Z, _ = loadings(x, gamma, anchored)
    for t in range(nobs - 1):
        y = data[:, t]
        if np.isnan(Yn[0, t]):
            if hasb:
                gamma = nuv + B * gamma
                Z, _ = loadings(x, gamma, anchored)
        else:
            try:
                beta = _ols(Z, y)
                if not static:
                    g = score(x, gamma, beta, y, anchored)
                    if scaled:
                        ewma = R.FORGET * ewma + (1 - R.FORGET) * (g * g)
                        count += 1
                        g = g / (torch.sqrt(ewma / (1 - R.FORGET ** count)) + EPS)
                    gamma = gamma + g * A
                    Z, _ = loadings(x, gamma, anchored)
                    beta = _ols(Z, y)
                    if hasb:
                        gamma = nuv + B * gamma
                        Z, _ = loadings(x, gamma, anchored)
            except StepFailed:
                return -math.inf
        beta = mu + Phi @ beta
        if np.isnan(Yn[:, t + 1]).any():
            return -math.inf
        v = data[:, t + 1] - Z @ beta
        mse = mse - v @ v
        if not bool(torch.isfinite(mse)):
            return -math.inf
    return mse / N / nobs


def loss_and_grad(kind, maturities, Y, theta, space=0, T_use=None):
    """(get_loss, ∂get_loss/∂θ [P] in the caller's space); (−inf, NaN) where the loss is −Inf."""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    loss = loss_tensor(kind, maturities, Y, th, space, T_use)
    if not isinstance(loss, torch.Tensor):
        return -math.inf, np.full(th.shape[0], np.nan)
    if loss.requires_grad:
        loss.backward()
        g = th.grad.numpy().copy()
    else:  # a window that compares nothing
        g = np.zeros(th.shape[0])
    return float(loss.detach()), g
