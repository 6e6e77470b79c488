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

# include/yfm.h: the neural kinds — YFM_MODEL_NNS, YFM_MODEL_NNS_ANCHORED and, for the score-driven ones,
# 32 | dyn | RW<<2 | SCALED<<3 | ANCHORED<<4 with dyn = 0 scalar, 1 block_diag, 2 diag
KIND_NNS, KIND_NNS_ANCHORED = 16, 17
NEURAL_SD_BASE = 32
NEURAL_DYNAMICS = ("scalar", "block_diag", "diag")
NEURAL_GAMMA = 18  # two 1→3→1 networks: [w₁(3), b(3), w₂(3)] each (mseneural.jl:29-30)


def neural_kind(dynamics, random_walk: bool = False, scale_grad: bool = False, transform_bool: bool = True) -> int:
    """The kind of MSEDNeuralModel(dynamics, random_walk; scale_grad, transform_bool) (mseneural.jl:17-24)."""
    dyn = NEURAL_DYNAMICS.index(dynamics) if isinstance(dynamics, str) else int(dynamics)
    if not 0 <= dyn <= 2:
        raise ValueError("dynamics must be 'scalar', 'block_diag' or 'diag'")
    return NEURAL_SD_BASE | dyn | (int(bool(random_walk)) << 2) | (int(bool(scale_grad)) << 3) | (
        int(not transform_bool) << 4)


def neural_name(kind: int) -> str:
    """model_dictionary.jl:20-112: the standardized string of a neural kind."""
    if kind in (KIND_NNS, KIND_NNS_ANCHORED):
        return "NNS" if kind == KIND_NNS else "NNS-Anchored"
    return (f"{(kind & 3) + 1}{'S' if kind >> 3 & 1 else ''}{'RW' if kind >> 2 & 1 else ''}SD-NNS"
            f"{'-Anchored' if kind >> 4 & 1 else ''}")


NEURAL_KINDS = (KIND_NNS, KIND_NNS_ANCHORED) + tuple(
    NEURAL_SD_BASE | d | rw << 2 | sc << 3 | an << 4 for an in (0, 1) for sc in (0, 1) for d in (0, 1, 2) for rw in (0, 1))
KIND_NAMES.update({k: neural_name(k) for k in NEURAL_KINDS})

ID, POS, R11, U01 = 0, 1, 2, 3


def is_neural_kind(kind: int) -> bool:
    return kind in NEURAL_KINDS


def neural_is_static(kind: int) -> bool:
    return kind in (KIND_NNS, KIND_NNS_ANCHORED)


def neural_has_b(kind: int) -> bool:
    """B exists unless γ is a random walk (mseneural.jl:53-57)."""
    return not neural_is_static(kind) and not kind >> 2 & 1


def neural_scaled(kind: int) -> bool:
    return not neural_is_static(kind) and bool(kind >> 3 & 1)


def neural_anchored(kind: int) -> bool:
    """transform_bool = false (model_dictionary.jl:74-112)."""
    return kind == KIND_NNS_ANCHORED if neural_is_static(kind) else bool(kind >> 4 & 1)


def neural_unique(kind: int) -> int:
    """maximum(duplicator) (mseneural.jl:33-48): the unique values of A (and of B)."""
    return 0 if neural_is_static(kind) else (2, 6, NEURAL_GAMMA)[kind & 3]


def neural_duplicator(kind: int) -> np.ndarray:
    """0-based duplicator: component k of γ takes unique value duplicator[k]."""
    return np.arange(NEURAL_GAMMA) // (9, 3, 1)[kind & 3]


def expand_unique(kind: int, unique) -> np.ndarray:
    """expand_params (paramteroperations.jl:36): the 18-vector (or 18×B) of unique values (n_unique[, B])."""
    return np.asarray(unique)[neural_duplicator(kind)]


@dataclass(frozen=True)
class NeuralLayout:
    """Offsets into θ of a neural model: [A_unique, B_unique | ω(18) (static: γ), δ(3), vec Φ(9, column-major)]."""
    kind: int
    n_unique: int
    n_lead: int  # A (and B) before ω / γ
    P: int
    M: int = 3

    @property
    def gamma_offset(self):
        return self.n_lead

    @property
    def delta_offset(self):
        return self.n_lead + NEURAL_GAMMA

    @property
    def phi_offset(self):
        return self.n_lead + NEURAL_GAMMA + 3


def neural_layout(kind: int) -> NeuralLayout:
    if not is_neural_kind(kind):
        raise KeyError(kind)
    nu = neural_unique(kind)
    n_lead = nu * (2 if neural_has_b(kind) else 1)
    return NeuralLayout(kind, nu, n_lead, n_lead + NEURAL_GAMMA + 12)


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
    if is_lambda_kind(kind) or is_neural_kind(kind):
        return 3
    return {KIND_DNS: 3, KIND_TVL: 4, KIND_GNS: 5}[kind]


def gamma_dim(kind: int) -> int:
    """L = length of base.gamma (kalmanbasemodel.jl:58), reported by predict as `states`."""
    if is_lambda_kind(kind):
        return 1  # γ_t (mselambda.jl:29, staticlambda.jl:20)
    if is_neural_kind(kind):
        return NEURAL_GAMMA
    return {KIND_DNS: 1, KIND_TVL: 1, KIND_GNS: 2}[kind]


def param_layout(kind: int) -> ParamLayout:
    M = state_dim(kind)
    n_lead = {KIND_DNS: 1, KIND_TVL: 0, KIND_GNS: 2}[kind]
    P = n_lead + 1 + M * (M + 1) // 2 + M + M * M
    return ParamLayout(kind, M, n_lead, P)


def n_params(kind: int) -> int:
    if is_lambda_kind(kind):
        return lambda_layout(kind).P
    if is_neural_kind(kind):
        return neural_layout(kind).P
    return param_layout(kind).P


def transform_codes(kind: int) -> np.ndarray:
    if is_lambda_kind(kind):
        # mselambda.jl:17-34 / staticlambda.jl:13-18, then msebasemodel.jl:77-83 / staticbasemodel.jl:47-53
        lead = [] if kind == KIND_NS else ([POS, U01] if lambda_has_b(kind) else [POS])
        phi = [R11 if i % 4 == 0 else ID for i in range(9)]
        return np.asarray(lead + [ID] + [ID] * 3 + phi, dtype=np.int8)
    if is_neural_kind(kind):
        # mseneural.jl:33-57, :74-75 / staticneural.jl:37-38, then msebasemodel.jl:77-83 / staticbasemodel.jl:47-53
        nu = neural_unique(kind)
        lead = [POS] * nu + ([U01] * nu if neural_has_b(kind) else [])
        phi = [R11 if i % 4 == 0 else ID for i in range(9)]
        return np.asarray(lead + [ID] * NEURAL_GAMMA + [ID] * 3 + phi, dtype=np.int8)
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
