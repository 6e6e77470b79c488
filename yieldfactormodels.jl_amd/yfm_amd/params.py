"""Parameter layout and the unconstrained<->constrained maps (host side).

Mirrors the reference's per-parameter transform vectors:

* ``src/models/kalman/kalmanbasemodel.jl:74-120`` — base block
  ``[σ² (exp), U upper-triangular by column (exp on the diagonal), δ (id),
  Φ row-major (2eˣ/(1+eˣ)−1 on the diagonal)]``;
* ``src/models/kalman/dns.jl:15-22`` — DNS prepends one identity (γ);
* ``src/models/kalman/tvλdns.jl:12-35`` — TVλ prepends nothing and uses a
  4-dimensional state;
* ``src/utils/transformations.jl:2-26`` and
  ``src/models/parameteroperations.jl:22-60`` — the elementwise maps.

The static and score-driven λ models (``src/models/filter.jl:52-110``) have their own layouts:

* ``src/models/msedriven/paramteroperations.jl:25-65`` — ``[A, B, ω, δ (3), vec Φ (9)]``, without ``B`` for
  the random-walk variants; ``src/models/static/paramteroperations.jl:19-43`` — ``[γ, δ, vec Φ]``.  Φ is
  filled with ``reshape``, so it is COLUMN-major, unlike the Kalman models' row-major Φ;
* ``src/models/msedriven/mselambda.jl:17-34``, ``msebasemodel.jl:77-90``, ``static/staticbasemodel.jl:48-59``
  — ``A → exp``, ``B → 1/(1+e^−x)``, the diagonal of Φ → ``2eˣ/(1+eˣ)−1``, the rest identity.

The device kernels decode θ themselves (``csrc/yfm_device.hpp``); this module
is the host API surface (``transform_params`` / ``untransform_params``) and
the single source of the layout offsets the host code uses.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

KIND_DNS, KIND_TVL, KIND_GNS = 0, 1, 2
# include/yfm.h: YFM_MODEL_NS .. YFM_MODEL_SRWSD_NS (7 is not a kind)
KIND_NS, KIND_SD_NS, KIND_RWSD_NS, KIND_SSD_NS, KIND_SRWSD_NS = 3, 4, 5, 6, 8
LAMBDA_KINDS = (KIND_NS, KIND_SD_NS, KIND_RWSD_NS, KIND_SSD_NS, KIND_SRWSD_NS)
KIND_NAMES = {KIND_DNS: "1C", KIND_TVL: "TVλ", KIND_GNS: "GNS5", KIND_NS: "NS", KIND_SD_NS: "SD-NS",
              KIND_RWSD_NS: "RWSD-NS", KIND_SSD_NS: "SSD-NS", KIND_SRWSD_NS: "SRWSD-NS"}

ID, POS, R11, U01 = 0, 1, 2, 3


def is_lambda_kind(kind: int) -> bool:
    return kind in LAMBDA_KINDS


def lambda_has_b(kind: int) -> bool:
    """B exists unless γ is a random walk (mselambda.jl:20-27)."""
    return kind in (KIND_SD_NS, KIND_SSD_NS)


def lambda_scaled(kind: int) -> bool:
    """scale_grad (model_dictionary.jl:30-35)."""
    return kind in (KIND_SSD_NS, KIND_SRWSD_NS)


@dataclass(frozen=True)
class LambdaLayout:
    """Offsets into θ of a λ model: [A, B, ω | γ, δ(3), vec Φ(9, column-major)]."""
    kind: int
    n_lead: int  # A (and B) before ω / γ
    P: int
    M: int = 3

    @property
    def gamma_offset(self):  # ω (NS: γ)
        return self.n_lead

    @property
    def delta_offset(self):
        return self.n_lead + 1

    @property
    def phi_offset(self):
        return self.n_lead + 4


def lambda_layout(kind: int) -> LambdaLayout:
    if not is_lambda_kind(kind):
        raise KeyError(kind)
    n_lead = 0 if kind == KIND_NS else (2 if lambda_has_b(kind) else 1)
    return LambdaLayout(kind, n_lead, n_lead + 13)


@dataclass(frozen=True)
class ParamLayout:
    kind: int
    M: int  # state dimension
    n_lead: int  # γ entries before the base block
    P: int

    @property
    def base_offset(self):  # index of σ²
        return self.n_lead

    @property
    def u_offset(self):
        return self.n_lead + 1

    @property
    def delta_offset(self):
        return self.u_offset + self.M * (self.M + 1) // 2

    @property
    def phi_offset(self):
        return self.delta_offset + self.M


def state_dim(kind: int) -> int:
    if is_lambda_kind(kind):
        return 3
    return {KIND_DNS: 3, KIND_TVL: 4, KIND_GNS: 5}[kind]


def gamma_dim(kind: int) -> int:
    """L = length of base.gamma (kalmanbasemodel.jl:58), reported by predict as `states`."""
    if is_lambda_kind(kind):
        return 1  # γ_t (mselambda.jl:29, staticlambda.jl:20)
    return {KIND_DNS: 1, KIND_TVL: 1, KIND_GNS: 2}[kind]


def param_layout(kind: int) -> ParamLayout:
    M = state_dim(kind)
    n_lead = {KIND_DNS: 1, KIND_TVL: 0, KIND_GNS: 2}[kind]
    P = n_lead + 1 + M * (M + 1) // 2 + M + M * M
    return ParamLayout(kind, M, n_lead, P)


def n_params(kind: int) -> int:
    if is_lambda_kind(kind):
        return lambda_layout(kind).P
    return param_layout(kind).P


def transform_codes(kind: int) -> np.ndarray:
    if is_lambda_kind(kind):
        # mselambda.jl:17-34 / staticlambda.jl:13-18, then msebasemodel.jl:77-83 / staticbasemodel.jl:47-53
        lead = [] if kind == KIND_NS else ([POS, U01] if lambda_has_b(kind) else [POS])
        phi = [R11 if i % 4 == 0 else ID for i in range(9)]
        return np.asarray(lead + [ID] + [ID] * 3 + phi, dtype=np.int8)
    lay = param_layout(kind)
    M = lay.M
    cov = []
    for i in range(M):  # kalmanbasemodel.jl:76-89
        for j in range(i + 1):
            cov.append(POS if i == j else ID)
    phi = [R11 if i == j else ID for i in range(M) for j in range(M)]
    return np.asarray([ID] * lay.n_lead + [POS] + cov + [ID] * M + phi, dtype=np.int8)


def transform_params(kind: int, theta) -> np.ndarray:
    """parameteroperations.jl:22-32 (works on a vector or a P×B matrix)."""
    theta = np.asarray(theta, dtype=np.float64)
    codes = transform_codes(kind)
    out = theta.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        pos = codes == POS
        out[pos] = np.exp(theta[pos])
        r = codes == R11
        y = np.exp(theta[r])
        out[r] = 2.0 * y / (1.0 + y) - 1.0  # transformations.jl:21-26, evaluated as written
        u = codes == U01
        out[u] = 1.0 / (1.0 + np.exp(-theta[u]))  # transformations.jl:28-32
    return out


def untransform_params(kind: int, theta_c) -> np.ndarray:
    """parameteroperations.jl:34-60."""
    theta_c = np.asarray(theta_c, dtype=np.float64)
    codes = transform_codes(kind)
    out = theta_c.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = codes == POS
        out[pos] = np.log(theta_c[pos])
        r = codes == R11
        out[r] = np.log1p(theta_c[r]) - np.log1p(-theta_c[r])
        u = codes == U01
        out[u] = np.log(theta_c[u] / (1.0 - theta_c[u]))  # transformations.jl:34-38
    return out

SPACE_UNCONSTRAINED, SPACE_CONSTRAINED = 0, 1
