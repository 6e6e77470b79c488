"""Host-side mirror of the reference's model API (the drop-in surface): the Kalman models and the static and
score-driven λ models.

Reference interface mirrored (paths relative to the reference root):

=======================================  =================================================
reference                                 here
=======================================  =================================================
``create_model`` model_dictionary.jl:7-16  :func:`create_model` (codes "1C"/"0", "TVλ"/"1";
                                            "GNS5" is this build's extension)
``DNSModel`` dns.jl:3-37                    :class:`DNSModel`
``TVλDNSModel`` tvλdns.jl:3-35              :class:`TVLambdaDNSModel`
``get_params`` paramoperations.jl:1-4       :func:`get_params`
``set_params!`` paramoperations.jl:45-68    :func:`set_params_` (Julia ``!`` → trailing ``_``)
``transform_params`` parameteroperations.jl:22-32    :func:`transform_params`
``untransform_params`` parameteroperations.jl:34-60  :func:`untransform_params`
``get_loss`` kalman/filter.jl:182-209       :func:`get_loss`
``compute_loss`` optimization.jl:10-23      :func:`compute_loss`
``predict`` kalman/filter.jl:250-282        :func:`predict` (``horizon`` = NaN padding of
                                            forecasting.jl:141)
``get_loss_array`` kalman/filter.jl:211-247 :func:`get_loss_array`
forecast blocks forecasting.jl:236-250      :func:`forecast_batch`
``estimate_steps!`` optimization.jl:137-312 :func:`estimate_steps_` (+ batched
                                            :func:`estimate_batch`; the λ models:
                                            :func:`estimate_steps_batch`, gradient of group "2":
                                            :func:`compute_loss_grad_block`)
``estimate!`` optimization.jl:329-410       :func:`estimate_` (+ batched
                                            :func:`estimate_lbfgs_batch`; gradient:
                                            :func:`compute_loss_grad_batch`)
``StaticλModel`` staticlambda.jl:3-32        :class:`StaticLambdaModel` ("NS" / "2")
``MSEDλModel`` mselambda.jl:3-49            :class:`MSEDLambdaModel` ("SD-NS" / "4", "RWSD-NS" / "5",
                                            "SSD-NS" / "6", "SRWSD-NS" / "7")
``get_loss`` / ``get_loss_array`` /         the same functions: for the λ models they restate
``predict`` src/models/filter.jl:209-306    src/models/filter.jl (K = 1)
``get_param_groups`` msebasemodel.jl:153-162  :func:`get_param_groups`
``try_initializations``                     :func:`try_initializations` (+ batched
optimization.jl:73-114                      :func:`try_initializations_batch`): the (A, B) grid in one launch
``create_model`` model_dictionary.jl:20-112  :func:`create_neural_model` (the 26 neural codes; `create_model`
                                            keeps refusing them)
``StaticNeuralModel`` staticneural.jl:3-60   :class:`StaticNeuralModel` ("NNS" / "3", "NNS-Anchored" / "20")
``MSEDNeuralModel`` mseneural.jl:3-102       :class:`MSEDNeuralModel` ("1SD-NNS" / "8" … "3SRWSD-NNS-Anchored" /
                                            "32"): loss, predict, get_loss_array, forecast blocks and the two-half
                                            (A₁, A₂, B₁, B₂) grid of try_initializations; estimation is not built
=======================================  =================================================

plus the batched forms the device boundary exists for: :func:`get_loss_batch` and
:func:`compute_loss_batch` (one call evaluates B parameter vectors).

All numerics run in libyfm_hip.so on the GPU; this module only holds parameters,
validates shapes and forwards pointers.  Errors mirror the reference: a batch
entry is ``-inf`` where ``get_loss`` returns ``-Inf`` and ``nan`` where the
reference would throw (singular ``I-Φ`` / ``I-Φ⊗Φ``); :func:`get_loss` raises
:class:`SingularException` in that case, as Julia does.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import groups as _groups
from . import params as _p
from .engine import get_engine
from .groups import EstimationError  # noqa: F401  (raised here and by the group descent)




class SingularException(ArithmeticError):
    """Raised where the reference's initialize_filter throws (filter.jl:4, :7)."""


@dataclass
class KalmanBaseModel:
    """kalmanbasemodel.jl:6-41 — the fields the hot path reads."""
    maturities: np.ndarray
    N: int
    M: int
    L: int
    kind: int
    model_string: str
    results_folder: str = "results/"
    flat_params: np.ndarray = field(default=None)

    def __post_init__(self):
        if self.flat_params is None:
            self.flat_params = np.zeros(_p.n_params(self.kind))

    @property
    def transformations(self):
        return _p.transform_codes(self.kind)


class AbstractKalmanModel:
    base: KalmanBaseModel
    device: int = 0

    @property
    def kind(self) -> int:
        return self.base.kind


class DNSModel(AbstractKalmanModel):
    """dns.jl:3-37: fixed-λ dynamic Nelson–Siegel, M = 3, P = 20."""

    def __init__(self, maturities, N: int, M: int = 3, model_string: str = "1C", results_location: str = "results/",
                 device: int = 0):
        if M != 3:
            raise ValueError("DNSModel is a 3-factor model (M = 3)")
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, 3, 1, _p.KIND_DNS, model_string,
                                    results_location)
        self.device = device


class TVLambdaDNSModel(AbstractKalmanModel):
    """tvλdns.jl:3-35: time-varying λ (EKF), state dimension M + 1 = 4, P = 31."""

    def __init__(self, maturities, N: int, M: int = 3, model_string: str = "TVλ", results_location: str = "results/",
                 device: int = 0):
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, M + 1, 1, _p.KIND_TVL, model_string,
                                    results_location)
        self.device = device


class GNS5Model(AbstractKalmanModel):
    """Extension (not in the reference): 5-factor generalised NS, loadings
    [1, S(λ₁), C(λ₁), S(λ₂), C(λ₂)], P = 48 ([γ₁, γ₂, base block])."""

    def __init__(self, maturities, N: int, M: int = 5, model_string: str = "GNS5", results_location: str = "results/",
                 device: int = 0):
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, 5, 2, _p.KIND_GNS, model_string,
                                    results_location)
        self.device = device


class StaticLambdaModel(AbstractKalmanModel):
    """staticlambda.jl:3-32: static Nelson–Siegel, θ_c = [γ, δ, vec Φ], P = 13.  (The base record is shared with
    the Kalman models: it holds the fields the device path reads.)"""

    def __init__(self, maturities, N: int, M: int = 3, model_string: str = "NS", results_location: str = "results/",
                 device: int = 0):
        if M != 3:
            raise ValueError("StaticLambdaModel is a 3-factor model (M = 3)")
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, 3, 1, _p.KIND_NS, model_string,
                                    results_location)
        self.device = device


class MSEDLambdaModel(AbstractKalmanModel):
    """mselambda.jl:3-49: score-driven λ, θ_c = [A, B, ω, δ, vec Φ] (no B when ``random_walk``), P = 15 / 14.
    ``scale_grad`` divides the score by the bias-corrected root of its EWMA, forget factor 0.98
    (filter.jl:29-44)."""

    A_guesses = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)  # mselambda.jl:26
    B_guesses = (0.9, 0.95, 0.98, 0.99, 0.999)         # mselambda.jl:27
    forget_factor = 0.98

    def __init__(self, maturities, N: int, M: int = 3, random_walk: bool = False, model_string: str = "MSEDλ",
                 results_location: str = "results/", scale_grad: bool = False, device: int = 0):
        if M != 3:
            raise ValueError("MSEDLambdaModel is a 3-factor model (M = 3)")
        kind = {(False, False): _p.KIND_SD_NS, (True, False): _p.KIND_RWSD_NS, (False, True): _p.KIND_SSD_NS,
                (True, True): _p.KIND_SRWSD_NS}[(bool(random_walk), bool(scale_grad))]
        self.random_walk = bool(random_walk)
        self.scale_grad = bool(scale_grad)
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, 3, 1, kind, model_string,
                                    results_location)
        self.device = device


_NEURAL_GAP = ("the λ and Kalman models' entry point; the neural kinds (NNS, …SD-NNS) are estimated through names of "
               "their own: estimate_neural_steps_ / estimate_neural_steps_batch (groups \"1\" and \"2\"), "
               "compute_neural_loss_grad_block (the δ/Φ gradient), compute_neural_loss_fullgrad_batch, "
               "estimate_neural_lbfgs_batch / estimate_neural_ (the L-BFGS multistart over every parameter) and "
               "driver.run_neural_estimation_; under this name the L-BFGS multistart and the Kalman Nelder–Mead driver "
               "are not built for them")


_NEURAL_RESTARTS = ("try_initializations of the static neural models draws its restarts from Julia's seeded generator "
                    "(Random.seed!(trial); randn, static/paramteroperations.jl:99-113), which is not restated here")


class StaticNeuralModel(AbstractKalmanModel):
    """staticneural.jl:3-60: static neural Nelson–Siegel, θ_c = [γ(18), δ, vec Φ], P = 30; ``transform_bool = False``
    is NNS-Anchored."""

    def __init__(self, maturities, N: int, M: int = 3, model_string: str = "NNS", results_location: str = "results/",
                 transform_bool: bool = True, device: int = 0):
        if M != 3:
            raise ValueError("StaticNeuralModel is a 3-factor model (M = 3)")
        self.transform_bool = bool(transform_bool)
        kind = _p.KIND_NNS if transform_bool else _p.KIND_NNS_ANCHORED
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, 3, _p.NEURAL_GAMMA, kind, model_string,
                                    results_location)
        self.device = device


class MSEDNeuralModel(AbstractKalmanModel):
    """mseneural.jl:3-102: score-driven neural Nelson–Siegel, θ_c = [A_unique, B_unique, ω(18), δ, vec Φ] (no B when
    ``random_walk``); ``dynamics`` ("scalar", "block_diag", "diag") is the duplicator that expands 2, 6 or 18 unique
    values of A and of B over the 18 components of γ.  ``scale_grad`` divides every component of the score by the
    bias-corrected root of its own EWMA, forget factor 0.9."""

    A_guesses = (1e-6, 1e-5, 1e-4, 1e-3)      # mseneural.jl:59
    B_guesses = (0.97, 0.98, 0.99, 0.999)     # mseneural.jl:60
    forget_factor = 0.9

    def __init__(self, maturities, N: int, M: int = 3, dynamics: str = "scalar", random_walk: bool = False,
                 model_string: str = "MSEDNeural", results_location: str = "results/", scale_grad: bool = False,
                 transform_bool: bool = True, device: int = 0):
        if M != 3:
            raise ValueError("MSEDNeuralModel is a 3-factor model (M = 3)")
        kind = _p.neural_kind(dynamics, random_walk, scale_grad, transform_bool)
        self.dynamics = _p.NEURAL_DYNAMICS[kind & 3]
        self.random_walk = bool(random_walk)
        self.scale_grad = bool(scale_grad)
        self.transform_bool = bool(transform_bool)
        self.duplicator = _p.neural_duplicator(kind) + 1  # 1-based, as the reference's
        self.base = KalmanBaseModel(np.asarray(maturities, dtype=np.float64), N, 3, _p.NEURAL_GAMMA, kind, model_string,
                                    results_location)
        self.device = device


def _nns(transform_bool):
    def make(mats, N, M, model_string, results_location, device):
        return StaticNeuralModel(mats, N, M, model_string=model_string, results_location=results_location,
                                 transform_bool=transform_bool, device=device)
    return make


def _msedn(dynamics, random_walk, scale_grad, transform_bool):
    def make(mats, N, M, model_string, results_location, device):
        return MSEDNeuralModel(mats, N, M, dynamics, random_walk, model_string=model_string,
                               results_location=results_location, scale_grad=scale_grad,
                               transform_bool=transform_bool, device=device)
    return make


def _neural_codes() -> dict:
    """model_dictionary.jl:20-112: "NNS" / "3", "1SD-NNS" / "8" … "3SRWSD-NNS" / "19", "NNS-Anchored" / "20",
    "1SD-NNS-Anchored" / "21" … "3SRWSD-NNS-Anchored" / "32"."""
    codes = {}
    for anchored, code in ((False, 3), (True, 20)):
        name = _p.neural_name(_p.KIND_NNS_ANCHORED if anchored else _p.KIND_NNS)
        codes[name] = codes[str(code)] = (name, _nns(not anchored))
        code = 8 if not anchored else 21
        for scaled in (False, True):
            for dyn in (0, 1, 2):
                for rw in (False, True):
                    name = _p.neural_name(_p.neural_kind(dyn, rw, scaled, not anchored))
                    codes[name] = codes[str(code)] = (name, _msedn(_p.NEURAL_DYNAMICS[dyn], rw, scaled, not anchored))
                    code += 1
    return codes


def _msed(random_walk, scale_grad):
    def make(mats, N, M, model_string, results_location, device):
        return MSEDLambdaModel(mats, N, M, random_walk, model_string=model_string, results_location=results_location,
                               scale_grad=scale_grad, device=device)
    return make


_CODES = {
    "1C": ("1C", DNSModel), "0": ("1C", DNSModel),
    "TVλ": ("TVλ", TVLambdaDNSModel), "1": ("TVλ", TVLambdaDNSModel),
    "GNS5": ("GNS5", GNS5Model),
    # model_dictionary.jl:17-35
    "NS": ("NS", StaticLambdaModel), "2": ("NS", StaticLambdaModel),
    "SD-NS": ("SD-NS", _msed(False, False)), "4": ("SD-NS", _msed(False, False)),
    "RWSD-NS": ("RWSD-NS", _msed(True, False)), "5": ("RWSD-NS", _msed(True, False)),
    "SSD-NS": ("SSD-NS", _msed(False, True)), "6": ("SSD-NS", _msed(False, True)),
    "SRWSD-NS": ("SRWSD-NS", _msed(True, True)), "7": ("SRWSD-NS", _msed(True, True)),
}
# model_dictionary.jl:20-112 (codes "3" and "8" … "32"): the neural models, a table of their own —
# :func:`create_neural_model`.  `create_model` keeps refusing these codes: the drivers built on it (estimation, the
# rolling forecasts) are not built for them, and a caller that reaches a neural model says so by the call it makes.
_NEURAL_CODES = _neural_codes()


def create_model(model_type: str, maturities, N: int, M: int = 3, float_type=np.float64,
                 results_location: str = "results/", device: int = 0):
    """model_dictionary.jl:7-35 for the Kalman codes and the static / score-driven λ codes; returns
    (model, standardized model_type)."""
    return _create(_CODES, model_type, maturities, N, M, float_type, results_location, device,
                   " — the neural codes are create_neural_model's" if model_type in _NEURAL_CODES else "")


def create_neural_model(model_type: str, maturities, N: int, M: int = 3, float_type=np.float64,
                        results_location: str = "results/", device: int = 0):
    """model_dictionary.jl:20-112 for the neural codes — "NNS" / "3", "1SD-NNS" / "8" … "3SRWSD-NNS" / "19",
    "NNS-Anchored" / "20", "1SD-NNS-Anchored" / "21" … "3SRWSD-NNS-Anchored" / "32" — with create_model's arguments
    and result: (model, standardized model_type)."""
    return _create(_NEURAL_CODES, model_type, maturities, N, M, float_type, results_location, device)


def _create(codes, model_type, maturities, N, M, float_type, results_location, device, hint=""):
    if np.dtype(float_type) != np.float64:
        raise ValueError("the MI355X path computes in Float64 only (the reference's Float64 path, test.jl:25)")
    if model_type not in codes:
        raise ValueError(f"Invalid model type: {model_type} (codes: {sorted(codes)}){hint}")
    std, cls = codes[model_type]
    mats = np.asarray(maturities, dtype=np.float64)
    if len(mats) != N:
        raise ValueError("len(maturities) != N")
    return cls(mats, N, M, model_string=model_type, results_location=results_location, device=device), std


def get_params(model: AbstractKalmanModel) -> np.ndarray:
    return model.base.flat_params


def set_params_(model: AbstractKalmanModel, params) -> None:
    """set_params! — stores the constrained parameter vector the filter will use."""
    params = np.asarray(params, dtype=np.float64).reshape(-1)
    if params.shape[0] != _p.n_params(model.kind):
        raise ValueError(f"expected {_p.n_params(model.kind)} parameters, got {params.shape[0]}")
    model.base.flat_params = params.copy()


def transform_params(model: AbstractKalmanModel, params) -> np.ndarray:
    return _p.transform_params(model.kind, params)


def untransform_params(model: AbstractKalmanModel, params) -> np.ndarray:
    return _p.untransform_params(model.kind, params)


def get_param_groups(model: AbstractKalmanModel, param_groups=()) -> list:
    """msebasemodel.jl:153-162 / staticbasemodel.jl:103-112: the caller's groups when there is one per parameter,
    else the defaults — "1" for the leading parameters, "2" for the M(M + 1) entries of δ and Φ."""
    if not (_p.is_lambda_kind(model.kind) or _p.is_neural_kind(model.kind)):
        raise NotImplementedError("Kalman models estimate every parameter in group \"1\"")
    P, M = _p.n_params(model.kind), model.base.M
    groups = list(param_groups)
    if len(groups) == P:
        return groups
    return ["1"] * (P - M * (M + 1)) + ["2"] * (M * (M + 1))


def _trial_grid(model) -> np.ndarray:
    """get_new_initial_params (msedriven/paramteroperations.jl:132-187, the n_unique == 1 branch): the (A, B)
    of trial 1, 2, … — B cycles fastest; the random-walk variants have the A trials only.  2×n_trials (row 2 NaN
    without B)."""
    if isinstance(model, MSEDNeuralModel):
        return _neural_trial_grid(model)
    A, Bg = MSEDLambdaModel.A_guesses, MSEDLambdaModel.B_guesses
    if _p.lambda_has_b(model.kind):
        return np.array([[a, b] for a in A for b in Bg]).T
    return np.array([[a, np.nan] for a in A]).T


def _neural_trial_grid(model) -> np.ndarray:
    """get_new_initial_params, the multi-unique branch (msedriven/paramteroperations.jl:161-184): trial k writes
    A₁ to the first half of the unique A values, A₂ to the second, and B₁, B₂ likewise; B₂ cycles fastest, then B₁,
    A₂, A₁ (random walk: A₂, then A₁).  n_lead×n_trials: the leading rows of θ_c for trial 1, 2, … (256, or 16)."""
    A, Bg = MSEDNeuralModel.A_guesses, MSEDNeuralModel.B_guesses
    nu = _p.neural_unique(model.kind)
    half = nu // 2
    has_b = _p.neural_has_b(model.kind)
    nA, nB = len(A), (len(Bg) if has_b else 0)
    total = nA ** 2 * nB ** 2 if has_b else nA ** 2
    grid = np.empty((nu * (2 if has_b else 1), total))
    for k in range(total):
        if has_b:
            a1, rem = divmod(k, nA * nB ** 2)
            a2, rem = divmod(rem, nB ** 2)
            b1, b2 = divmod(rem, nB)
            grid[nu:nu + half, k] = Bg[b1]
            grid[nu + half:, k] = Bg[b2]
        else:
            a1, a2 = divmod(k, nA)
        grid[:half, k] = A[a1]
        grid[half:nu, k] = A[a2]
    return grid


def try_initializations_batch(best_params, model: AbstractKalmanModel, data, T_use=None):
    """optimization.jl:73-114 for W starts at once: column w of ``best_params`` (P×W, constrained) on the window
    ``data[:, :T_use[w]]``.  The start and its 30 (A, B) trials (6 for the random-walk variants) of every window go
    through ONE launch; the winner is the reference's: a trial replaces the running best only on a strict
    improvement, in trial order.  Returns (P×W winners, W losses, the loss being −get_loss)."""
    if isinstance(model, StaticNeuralModel):
        raise NotImplementedError(_NEURAL_RESTARTS)
    if not isinstance(model, (MSEDLambdaModel, MSEDNeuralModel)):
        raise TypeError("try_initializations walks the (A, B) grid of a score-driven model")
    best = np.asarray(best_params, dtype=np.float64)
    best = best.reshape(best.shape[0], -1)
    P, W = best.shape
    grid = _trial_grid(model)
    n = grid.shape[1]
    cand = np.repeat(best[:, :, None], n + 1, axis=2)  # P × W × (1 + n): the start, then the trials
    if isinstance(model, MSEDNeuralModel):
        # the two-half (A₁, A₂, B₁, B₂) grid: 256 trials, 16 for the random-walk kinds
        cand[:grid.shape[0], :, 1:] = grid[:, None, :]
    else:
        cand[0, :, 1:] = grid[0]
        if _p.lambda_has_b(model.kind):
            cand[1, :, 1:] = grid[1]
    tu = None if T_use is None else np.repeat(np.broadcast_to(T_use, (W,)), n + 1)
    loss = -get_loss_batch(model, data, cand.reshape(P, W * (n + 1)), space=_p.SPACE_CONSTRAINED, T_use=tu)
    loss = loss.reshape(W, n + 1)
    out = np.empty((P, W), order="F")
    out_loss = np.empty(W)
    for w in range(W):
        k_best = 0
        for k in range(1, n + 1):
            if loss[w, k] < loss[w, k_best]:  # `loss < init_loss` (optimization.jl:105)
                k_best = k
        out[:, w] = cand[:, w, k_best]
        out_loss[w] = loss[w, k_best]
    return out, out_loss


def try_initializations(best_params, model: AbstractKalmanModel, data):
    """optimization.jl:73-114: the P×1 winner among the start and the (A, B) trials.  Other models return the
    start unchanged (optimization.jl:33-35)."""
    best = np.asarray(best_params, dtype=np.float64).reshape(-1)
    if isinstance(model, StaticNeuralModel):
        raise NotImplementedError(_NEURAL_RESTARTS)
    if not isinstance(model, (MSEDLambdaModel, MSEDNeuralModel)):
        return best.reshape(-1, 1).copy()
    out, _ = try_initializations_batch(best[:, None], model, data)
    set_params_(model, out[:, 0])  # the reference leaves the model at the last trial; the winner is the useful state
    return out


def _is_kalman(kind: int) -> bool:
    return not (_p.is_lambda_kind(kind) or _p.is_neural_kind(kind))


def _engine(model, data):
    eng = get_engine(model.device)
    eng.set_panel(data, model.base.maturities)
    return eng


def get_loss(model: AbstractKalmanModel, data) -> float:
    """filter.jl:182-209 for the model's current (constrained) parameters."""
    eng = _engine(model, data)
    ll = float(eng.loglik(model.kind, model.base.flat_params, space=_p.SPACE_CONSTRAINED)[0])
    if np.isnan(ll) and _is_kalman(model.kind):
        raise SingularException("initialize_filter: singular I - Φ or I - Φ⊗Φ")
    return ll


def compute_loss(model: AbstractKalmanModel, data, params) -> float:
    """optimization.jl:10-23: transform, set_params!, return -get_loss."""
    set_params_(model, transform_params(model, params))
    return -get_loss(model, data)


def get_loss_batch(model: AbstractKalmanModel, data, Theta, space: int = 1, T_use=None) -> np.ndarray:
    """Batched get_loss over the columns of Θ (P×B).  ``space`` 1 = constrained θ_c
    (set_params! input), 0 = unconstrained θ (compute_loss input).  ``T_use[b]``
    evaluates ``get_loss(model, data[:, :T_use[b]])``."""
    eng = _engine(model, data)
    return eng.loglik(model.kind, Theta, space=space, T_use=T_use)


def compute_loss_batch(model: AbstractKalmanModel, data, Theta, T_use=None) -> np.ndarray:
    """Batched compute_loss: −loglik for every unconstrained θ_b (column of Θ)."""
    return -get_loss_batch(model, data, Theta, space=_p.SPACE_UNCONSTRAINED, T_use=T_use)


def filter_states(model: AbstractKalmanModel, data, Theta=None, space: int = 1, T_use=None):
    """(loglik[B], beta[M,T-1,B], P[M,M,T-1,B]): the predicted state after every filter! call."""
    eng = _engine(model, data)
    if Theta is None:
        Theta = model.base.flat_params
    return eng.filter_states(model.kind, Theta, space=space, T_use=T_use)


def predict(model: AbstractKalmanModel, data, horizon: int = 1, Theta=None, space: int = 1, T_use=None):
    """filter.jl:250-282 — ``predict(model, data)`` for the model's parameters (horizon = 1), or
    ``predict(model, hcat(data[:, 1:T_b], NaN × (horizon − 1)))`` as the forecasting driver calls it
    (forecasting.jl:141, :181-183).  With ``Theta`` (P×B) the call is batched and every array gets a
    trailing batch axis; otherwise returns the reference's named tuple of N×n / M×n / L×n arrays,
    n = T + horizon − 1."""
    eng = _engine(model, data)
    single = Theta is None
    if single:
        Theta = model.base.flat_params
    out = eng.predict(model.kind, Theta, space=space, T_use=T_use, horizon=horizon)
    if single:
        out = {k: v[:, :, 0] for k, v in out.items()}
        if np.isnan(out["factors"]).all() and _is_kalman(model.kind):
            raise SingularException("initialize_filter: singular I - Φ or I - Φ⊗Φ")
    return out


def get_loss_array(model: AbstractKalmanModel, data, K: int = 1, Theta=None, space: int = 1, T_use=None):
    """filter.jl:211-247: the per-step −‖y_t − ŷ_t‖²/N/K (length T−1), or the scalar −Inf where the
    reference returns it.  With ``Theta`` (P×B): a (T−1)×B array, −Inf rows for −Inf candidates."""
    eng = _engine(model, data)
    single = Theta is None
    out = eng.loss_array(model.kind, model.base.flat_params if single else Theta, space=space, T_use=T_use, K=K)
    if single:
        row = out[:, 0]
        if np.isnan(row).all() and row.size and _is_kalman(model.kind):
            raise SingularException("initialize_filter: singular I - Φ or I - Φ⊗Φ")
        if row.size and np.isneginf(row).all():
            return -np.inf
        return row
    return out


def forecast_batch(model: AbstractKalmanModel, data, Theta, T_use, horizon: int, space: int = 1) -> np.ndarray:
    """The rolling-window driver's per-task record (forecasting.jl:236-250): for window b,
    ``vcat(factors, states, preds)[:, end-h+1:end]`` of predict on hcat(data[:, 1:T_use[b]], NaN × (h−1)).
    Returns (M + L + N, h, B)."""
    eng = _engine(model, data)
    return eng.forecast(model.kind, Theta, space=space, T_use=T_use, horizon=horizon)


def estimate_steps_(model: AbstractKalmanModel, data, all_params, param_groups=None, max_group_iters: int = 10,
                    tol: float = 1e-8, printing: bool = False, iterations: int = 500, full_gradient: bool = False):
    """estimate_steps! (optimization.jl:137-312): all_params (P×n, constrained; column 1 only is used, :153)
    → (init_p, ll, best_p, ir), init_p and best_p constrained like the
    reference: init_p = transform_params of the untransformed, sanitised and ×0.95-rescaled start
    (:157-184, :298-302).
    Kalman models: parameter groups other than all-"1" are not supported (their default, kalmanbasemodel.jl:150-159).
    λ models: :func:`estimate_steps_batch` with one chain (`full_gradient` is its keyword, for them alone).
    `iterations`: the NelderMead budget per group (opt1, optimization.jl:442-451: 500)."""
    if _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_steps_ is " + _NEURAL_GAP)
    A = np.asarray(all_params, dtype=np.float64)
    start = A[:, 0] if A.ndim == 2 else A
    if _p.is_lambda_kind(model.kind):
        # the λ models: block-coordinate descent over param_groups (default get_param_groups), column 1 only (:153)
        r = estimate_steps_batch(model, data, start[:, None], param_groups=param_groups,
                                 max_group_iters=max_group_iters, tol=tol, iterations=iterations,
                                 full_gradient=full_gradient)
        return _first_chain(r, printing)
    if param_groups is not None and any(g != "1" for g in param_groups):
        raise NotImplementedError("Kalman models estimate every parameter in group \"1\"")
    r = estimate_batch(model, data, start[:, None], max_group_iters=max_group_iters, tol=tol, iterations=iterations)
    if r["status"][0] == 1:
        raise EstimationError("compute_loss threw on the first group iteration (singular initialize_filter)")
    return _first_chain(r, printing)


def _first_chain(r, printing):
    """What estimate_steps! returns for a one-chain result `r`: (init_p, ll, best_p, ir)."""
    if printing:
        print(f"✓ Best overall LL = {r['ll'][0]} from start 1")
    return r["init_c"][:, 0].copy(), float(r["ll"][0]), r["theta_c"][:, 0].copy(), 0


def estimate_batch(model: AbstractKalmanModel, data, Theta0, T_use=None, space: int = 1, iterations: int = 500,
                   g_tol: float = 1e-6, max_group_iters: int = 10, tol: float = 1e-8) -> dict:
    """R independent estimate_steps! chains (windows × starts) whose objective evaluations share one device
    launch per round (libyfm_hip.so: yfm_estimate).  Θ₀: P×R starts (constrained by default, as all_params)."""
    if _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_batch is " + _NEURAL_GAP)
    eng = _engine(model, data)
    return eng.estimate(model.kind, Theta0, space=space, T_use=T_use, iterations=iterations, g_tol=g_tol,
                        max_group_iters=max_group_iters, tol=tol)


def estimate_steps_batch(model: AbstractKalmanModel, data, Theta0, T_use=None, param_groups=None,
                         max_group_iters: int = 10, tol: float = 1e-8, iterations=None,
                         full_gradient: bool = False) -> dict:
    """R independent estimate_steps! chains of a λ model (optimization.jl:137-312), one per column of Θ₀ (P×R,
    constrained, as all_params) on the window ``data[:, :T_use[r]]``, advancing in lockstep: every step of the
    block-coordinate descent (:mod:`yfm_amd.groups`) is one batched call for all unfinished chains.

    * start: :func:`try_initializations_batch` for the score-driven kinds (NS keeps its start,
      optimization.jl:33-35), untransform, sanitise, ×0.95 while the loss is not finite;
    * group "1" / "4" (and any id without an optimiser of its own): Optim.NelderMead with opt1 on the group's
      coordinates — ``yfm_nm_block``, one launch per round for all chains;
    * group "2": L-BFGS (:mod:`yfm_amd.lbfgs`, opt2's options) on δ and Φ with value and gradient rows from
      :func:`compute_loss_grad_block`, one launch per round;
    * groups "3" / "5" (Adam) and a "2" group holding a leading parameter raise NotImplementedError;
    * ``full_gradient=True``: a "2" group may hold leading parameters (A, B, ω; γ for NS) — its rows then come from
      the full gradient, :func:`compute_lambda_loss_grad_batch`, one launch per round as before.

    `iterations` caps both optimisers' budgets (None: the reference's 500 and 250).  Returns what
    :func:`estimate_batch` returns — theta_c, p, init_c (the reference's init_p), ll, status, n_evals — plus
    evals_by_group, rounds_by_group and group_iters."""
    if _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_steps_batch is " + _NEURAL_GAP)
    if not _p.is_lambda_kind(model.kind):
        raise NotImplementedError("estimate_steps_batch is the λ models' driver; Kalman models use estimate_batch")
    return _estimate_groups(model, data, Theta0, T_use, param_groups, max_group_iters, tol, iterations,
                            searched=isinstance(model, MSEDLambdaModel),
                            grad="lambda_loss_full_grad" if full_gradient else "lambda_loss_grad", full=full_gradient)


def _estimate_groups(model, data, Theta0, T_use, param_groups, max_group_iters, tol, iterations, searched: bool,
                     grad: str, full: bool = False) -> dict:
    """The body of :func:`estimate_steps_batch` and :func:`estimate_neural_steps_batch`: they differ in whether the
    start is searched (try_initializations_batch) and in the engine method that returns the gradient — the δ/Φ rows,
    or with `full` all P rows, so that no row counts as a leading one an L-BFGS group must not hold."""
    kind = model.kind
    Th = np.asarray(Theta0, dtype=np.float64)
    Th = Th.reshape(Th.shape[0], -1)
    P, R = Th.shape
    groups = get_param_groups(model, () if param_groups is None else param_groups)
    n_lead = 0 if full else P - model.base.M * (model.base.M + 1)  # rows without a gradient
    _groups.check_groups(groups, n_lead)  # before any launch
    tu = None if T_use is None else np.ascontiguousarray(np.broadcast_to(T_use, (R,)), dtype=np.int32)
    if searched:
        Th, _ = try_initializations_batch(Th, model, data, T_use=tu)
    eng = _engine(model, data)
    loss_grad = getattr(eng, grad)

    def win(cols):
        return None if tu is None else tu[cols]

    def value(X, cols):
        return -eng.loglik(kind, X, space=_p.SPACE_UNCONSTRAINED, T_use=win(cols))

    def value_grad(X, cols, rows):
        loss, g = loss_grad(kind, X, space=_p.SPACE_UNCONSTRAINED, T_use=win(cols))
        return -loss, -g[np.asarray(rows) - n_lead]

    def nelder_mead(X, cols, rows, its, g_tol):
        return eng.nm_block(kind, X, rows, T_use=win(cols), iterations=its, g_tol=g_tol)

    opts = dict(_groups.LBFGS_OPTIONS)
    nm_its = _groups.NM_ITERATIONS
    if iterations is not None:
        opts["iterations"] = min(opts["iterations"], int(iterations))
        nm_its = min(nm_its, int(iterations))
    r = _groups.descend(_p.untransform_params(kind, Th), groups, value, value_grad, nelder_mead, n_lead,
                        max_group_iters=max_group_iters, tol=tol, nm_iterations=nm_its, lbfgs_options=opts)
    return dict(theta_c=np.asfortranarray(_p.transform_params(kind, r["p"])), p=r["p"],
                init_c=np.asfortranarray(_p.transform_params(kind, r["init"])), ll=r["ll"], status=r["status"],
                n_evals=r["n_evals"], evals_by_group=r["evals_by_group"], rounds_by_group=r["rounds_by_group"],
                group_iters=r["group_iters"])


def estimate_neural_steps_batch(model: AbstractKalmanModel, data, Theta0, T_use=None, param_groups=None,
                                max_group_iters: int = 10, tol: float = 1e-8, iterations=None,
                                full_gradient: bool = False) -> dict:
    """:func:`estimate_steps_batch` for the neural kinds (a model from :func:`create_neural_model`): the same
    arguments, descent and returned dict.  The start is :func:`try_initializations_batch` for the score-driven kinds
    (the 256-trial grid, 16 for the random-walk kinds); NNS and NNS-Anchored keep their start, as the reference's
    ``max_tries = 0`` does (optimization.jl:37-43).  Group "1" (A, B, ω; γ for the static kinds: 18–54 coordinates)
    is ``yfm_nm_block``, group "2" is L-BFGS on value and gradient rows from ``yfm_neural_loss_grad_batch``.
    ``full_gradient=True``: a "2" group may hold leading parameters — its rows then come from the full gradient,
    :func:`compute_neural_loss_fullgrad_batch`, one launch per round as before."""
    if not _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_neural_steps_batch is the neural models' driver; λ models use "
                                  "estimate_steps_batch, Kalman models estimate_batch")
    return _estimate_groups(model, data, Theta0, T_use, param_groups, max_group_iters, tol, iterations,
                            searched=isinstance(model, MSEDNeuralModel),
                            grad="neural_loss_full_grad" if full_gradient else "neural_loss_grad", full=full_gradient)


def estimate_neural_steps_(model: AbstractKalmanModel, data, all_params, param_groups=None, max_group_iters: int = 10,
                           tol: float = 1e-8, printing: bool = False, iterations: int = 500):
    """estimate_steps! (optimization.jl:137-312) for a neural model: all_params (P×n, constrained; column 1 only is
    used, :153) → (init_p, ll, best_p, ir) — :func:`estimate_neural_steps_batch` with one chain."""
    A = np.asarray(all_params, dtype=np.float64)
    start = A[:, 0] if A.ndim == 2 else A
    r = estimate_neural_steps_batch(model, data, start[:, None], param_groups=param_groups,
                                    max_group_iters=max_group_iters, tol=tol, iterations=iterations)
    return _first_chain(r, printing)


def _neg_loss_grad(model, data, Theta, T_use, method, guard):
    """(−value[B], −gradient[rows, B]) of the engine's gradient call `method` at the unconstrained columns of Θ, the
    reference's loss sign.  `guard`: None, or why the model's kind is not served (raised before the panel is set)."""
    if guard:
        raise NotImplementedError(guard)
    val, g = getattr(_engine(model, data), method)(model.kind, Theta, space=_p.SPACE_UNCONSTRAINED, T_use=T_use)
    return -val, -g


def compute_loss_grad_batch(model: AbstractKalmanModel, data, Theta, T_use=None):
    """Batched compute_loss with its gradient — what estimate!'s TwiceDifferentiable(...; autodiff=:forward)
    evaluates (optimization.jl:367): (−loglik[B], −∂loglik/∂θ[P, B]) for every unconstrained θ_b, the
    reference's loss sign.  DNS with N ≤ 64 (:meth:`Engine.loglik_grad`), TVλ (:meth:`Engine.tvl_loglik_grad`) and
    the λ models (:meth:`Engine.lambda_loss_full_grad`: −get_loss and its full gradient); NaN gradient columns as
    there."""
    method = ("lambda_loss_full_grad" if _p.is_lambda_kind(model.kind)
              else "tvl_loglik_grad" if model.kind == _p.KIND_TVL else "loglik_grad")
    return _neg_loss_grad(model, data, Theta, T_use, method, None)


def compute_lambda_loss_grad_batch(model: AbstractKalmanModel, data, Theta, T_use=None):
    """Batched compute_loss of a λ model with its gradient over every row of θ — what an L-BFGS group of
    estimate_steps! that holds leading parameters evaluates: (−loss[B], −∂loss/∂θ[P, B]) for every unconstrained θ_b
    (:meth:`Engine.lambda_loss_full_grad`).  NaN gradient columns where the loss is −Inf or a tangent is not finite."""
    guard = None if _p.is_lambda_kind(model.kind) else (
        "the full loss gradient is the λ models'; Kalman models use compute_loss_grad_batch, "
        "neural models compute_neural_loss_grad_block")
    return _neg_loss_grad(model, data, Theta, T_use, "lambda_loss_full_grad", guard)


def compute_loss_grad_block(model: AbstractKalmanModel, data, Theta, T_use=None):
    """Batched compute_loss of a λ model with its gradient over parameter group "2" — what Optim.LBFGS evaluates
    in estimate_steps! for the δ/Φ block (optimization.jl:442-479): (−loss[B], −∂loss/∂θ[12, B]) for every
    unconstrained θ_b, the rows being θ's last 12 (δ, then vec Φ column-major).  NaN gradient columns where the
    loss is −Inf."""
    guard = ("compute_loss_grad_block is " + _NEURAL_GAP if _p.is_neural_kind(model.kind)
             else None if _p.is_lambda_kind(model.kind)
             else "the δ/Φ block gradient is the λ models'; Kalman models use compute_loss_grad_batch")
    return _neg_loss_grad(model, data, Theta, T_use, "lambda_loss_grad", guard)


def compute_neural_loss_grad_block(model: AbstractKalmanModel, data, Theta, T_use=None):
    """:func:`compute_loss_grad_block` for the neural kinds: (−loss[B], −∂loss/∂θ[12, B]) over θ's last 12 rows."""
    guard = None if _p.is_neural_kind(model.kind) else (
        "compute_neural_loss_grad_block is the neural models'; λ models use compute_loss_grad_block")
    return _neg_loss_grad(model, data, Theta, T_use, "neural_loss_grad", guard)


def compute_neural_loss_fullgrad_batch(model: AbstractKalmanModel, data, Theta, T_use=None):
    """Batched compute_loss of a neural model with its gradient over every row of θ — what an L-BFGS over all
    parameters evaluates: (−loss[B], −∂loss/∂θ[P, B]) for every unconstrained θ_b
    (:meth:`Engine.neural_loss_full_grad`).  NaN gradient columns where the loss is −Inf or an adjoint is not finite."""
    guard = None if _p.is_neural_kind(model.kind) else (
        "compute_neural_loss_fullgrad_batch is the neural models'; λ models use "
        "compute_lambda_loss_grad_batch, Kalman models compute_loss_grad_batch")
    return _neg_loss_grad(model, data, Theta, T_use, "neural_loss_full_grad", guard)


def estimate_lbfgs_batch(model: AbstractKalmanModel, data, Theta0, space: int = 1, T_use=None, **opts) -> dict:
    """One L-BFGS chain of estimate! (optimization.jl:329-410) per column of Θ₀ (P×R; constrained by default, as
    all_params), all chains advancing in lockstep with one gradient launch per round (:mod:`yfm_amd.lbfgs`;
    `opts`: iterations, g_tol, f_abstol, allow_f_increases).  Returns the per-start arrays: theta_c (P×R),
    p (P×R unconstrained optimum), init_c (P×R: the start, constrained), ll (R), ll0 (R: the loglik at the
    start), status (R: lbfgs status; 0 = converged), iterations (R), n_evals, rounds.  ``T_use`` (an int, or one per
    column) runs chain r on the window ``data[:, :T_use[r]]``; None is the whole panel."""
    if _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_ (the L-BFGS multistart) is " + _NEURAL_GAP)
    return _lbfgs_chains(model, data, Theta0, space, T_use, compute_loss_grad_batch, opts)


def _lbfgs_chains(model, data, Theta0, space, T_use, loss_grad, opts) -> dict:
    """The body of :func:`estimate_lbfgs_batch` and :func:`estimate_neural_lbfgs_batch`: they differ in the function
    that returns (−loss, −gradient) over every row of θ."""
    from . import lbfgs as _lbfgs
    Th = np.asarray(Theta0, dtype=np.float64)
    if Th.ndim == 1:
        Th = Th[:, None]
    X0 = Th if space == _p.SPACE_UNCONSTRAINED else _p.untransform_params(model.kind, Th)
    tu = None if T_use is None else np.ascontiguousarray(np.broadcast_to(T_use, (X0.shape[1],)), dtype=np.int32)
    ll0 = -loss_grad(model, data, X0, T_use=tu)[0]
    if tu is None:
        r = _lbfgs.minimize_batch(lambda X: loss_grad(model, data, X), X0, **opts)
    else:  # finished chains drop out of the batch: every column brings its chain's window
        r = _lbfgs.minimize_batch(lambda X, idx: loss_grad(model, data, X, T_use=tu[np.asarray(idx)]),
                                  X0, with_index=True, **opts)
    return dict(theta_c=np.asfortranarray(_p.transform_params(model.kind, r["x"])), p=r["x"],
                init_c=np.asfortranarray(_p.transform_params(model.kind, X0)), ll=-r["f"], ll0=ll0,
                status=r["status"], iterations=r["iterations"], n_evals=r["n_evals"] + X0.shape[1],
                rounds=r["rounds"] + 1)


def estimate_(model: AbstractKalmanModel, data, all_params, printing: bool = False, **opts):
    """estimate! (optimization.jl:329-410): multistart L-BFGS from the columns of all_params (P×n, constrained)
    → (init_params, ll, best_params, ir) of the start with the largest ll, both parameter vectors constrained,
    ir = 0 if that chain converged else 1.  Raises :class:`EstimationError` where the reference throws:
    compute_loss throws at a start (singular initialize_filter), or no start ends with ll > −Inf (the
    reference then indexes its results with best_j = 0)."""
    return _best_start(estimate_lbfgs_batch, model, data, all_params, printing, opts)


def _best_start(chains, model, data, all_params, printing, opts):
    """The body of :func:`estimate_` and :func:`estimate_neural_`: the multistart over `chains` and its best start."""
    A = np.asarray(all_params, dtype=np.float64)
    if A.ndim == 1:
        A = A[:, None]
    r = chains(model, data, A, space=_p.SPACE_CONSTRAINED, **opts)
    if np.isnan(r["ll0"]).any():
        raise EstimationError("compute_loss threw at a starting point (singular initialize_filter)")
    ll = np.where(np.isnan(r["ll"]), -np.inf, r["ll"])
    if not (ll > -np.inf).any():
        raise EstimationError("no starting point reached a finite log-likelihood")
    j = int(np.argmax(ll))  # the first of equal maxima, as the reference's `ll > best_ll`
    if printing:
        print(f"✓ Best LL = {r['ll'][j]} from starting point {j + 1}")
    return r["init_c"][:, j].copy(), float(r["ll"][j]), r["theta_c"][:, j].copy(), 0 if r["status"][j] == 0 else 1


def estimate_neural_lbfgs_batch(model: AbstractKalmanModel, data, Theta0, space: int = 1, T_use=None, **opts) -> dict:
    """:func:`estimate_lbfgs_batch` for a model from :func:`create_neural_model`: one L-BFGS chain over all P rows per
    column of Θ₀, on value and gradient from :func:`compute_neural_loss_fullgrad_batch` (one launch per round); the
    same arguments, `opts` and returned dict."""
    if not _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_neural_lbfgs_batch is the neural models'; λ and Kalman models use "
                                  "estimate_lbfgs_batch")
    return _lbfgs_chains(model, data, Theta0, space, T_use, compute_neural_loss_fullgrad_batch, opts)


def estimate_neural_(model: AbstractKalmanModel, data, all_params, printing: bool = False, **opts):
    """:func:`estimate_` for a model from :func:`create_neural_model`: the multistart L-BFGS over the columns of
    all_params through :func:`estimate_neural_lbfgs_batch` → (init_params, ll, best_params, ir), with
    :class:`EstimationError` as there."""
    if not _p.is_neural_kind(model.kind):
        raise NotImplementedError("estimate_neural_ is the neural models'; λ and Kalman models use estimate_")
    return _best_start(estimate_neural_lbfgs_batch, model, data, all_params, printing, opts)
