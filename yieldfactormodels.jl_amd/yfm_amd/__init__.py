"""yfm_amd — MI355X-native batched Kalman log-likelihood for YieldFactorModels.jl.

The numerics live in ``libyfm_hip.so`` (HIP, gfx950) behind the C ABI of
``include/yfm.h``; this package is the host-side mirror of the reference's
model / objective API (see :mod:`yfm_amd.models`).
"""
from .params import (KIND_NS, KIND_RWSD_NS, KIND_SD_NS, KIND_SRWSD_NS, KIND_SSD_NS, LAMBDA_KINDS)
from .params import (KIND_DNS, KIND_GNS, KIND_TVL, SPACE_CONSTRAINED, SPACE_UNCONSTRAINED, gamma_dim, n_params,
                     param_layout, state_dim)
from .models import (DNSModel, EstimationError, GNS5Model, SingularException, TVLambdaDNSModel, compute_loss, compute_loss_batch, compute_loss_grad_batch,
                     create_model, estimate_, estimate_batch, estimate_lbfgs_batch, estimate_steps_, filter_states, forecast_batch, get_loss, get_loss_array, get_loss_batch,
                     get_params, predict, set_params_, transform_params, untransform_params)
from .models import (MSEDLambdaModel, StaticLambdaModel, compute_lambda_loss_grad_batch, compute_loss_grad_block, estimate_steps_batch,
                     get_param_groups, try_initializations, try_initializations_batch)
from .models import MSEDNeuralModel, StaticNeuralModel, create_neural_model
from .models import compute_neural_loss_grad_block, estimate_neural_steps_, estimate_neural_steps_batch
from .models import compute_neural_loss_fullgrad_batch, estimate_neural_, estimate_neural_lbfgs_batch
from .params import KIND_NNS, KIND_NNS_ANCHORED, NEURAL_KINDS, is_neural_kind, neural_kind
from .engine import Engine, get_engine
from .driver import load_initial_parameters_, run, run_neural_estimation_
from . import lbfgs
from . import inference
from .inference import covariance, standard_errors_, standard_errors_batch
from .inference import tvl_standard_errors_, tvl_standard_errors_batch
from . import smoothing
from .smoothing import em_moments, smooth_, smooth_batch, smoothed_yields
from .smoothing import tvl_smooth_, tvl_smooth_batch, tvl_smoothed_yields

__all__ = [
    "KIND_DNS", "KIND_TVL", "KIND_GNS", "SPACE_CONSTRAINED", "SPACE_UNCONSTRAINED", "n_params", "param_layout",
    "state_dim", "DNSModel", "TVLambdaDNSModel", "GNS5Model", "SingularException", "create_model", "get_params",
    "set_params_", "transform_params", "untransform_params", "get_loss", "compute_loss", "get_loss_batch",
    "compute_loss_batch", "filter_states", "estimate_steps_", "estimate_batch", "predict", "get_loss_array", "forecast_batch", "gamma_dim", "Engine",
    "get_engine", "run", "load_initial_parameters_", "compute_loss_grad_batch", "estimate_", "estimate_lbfgs_batch",
    "EstimationError", "lbfgs", "KIND_NS", "KIND_SD_NS", "KIND_RWSD_NS", "KIND_SSD_NS", "KIND_SRWSD_NS", "LAMBDA_KINDS",
    "StaticLambdaModel", "MSEDLambdaModel", "get_param_groups", "try_initializations", "try_initializations_batch",
    "compute_loss_grad_block", "compute_lambda_loss_grad_batch", "estimate_steps_batch", "StaticNeuralModel", "MSEDNeuralModel", "create_neural_model", "KIND_NNS",
    "KIND_NNS_ANCHORED", "NEURAL_KINDS", "is_neural_kind", "neural_kind",
    "compute_neural_loss_grad_block", "estimate_neural_steps_", "estimate_neural_steps_batch", "run_neural_estimation_",
    "compute_neural_loss_fullgrad_batch", "estimate_neural_lbfgs_batch", "estimate_neural_",
    "inference", "covariance", "standard_errors_batch", "standard_errors_",
    "tvl_standard_errors_batch", "tvl_standard_errors_",
    "smoothing", "smooth_batch", "smooth_", "smoothed_yields", "em_moments",
    "tvl_smooth_batch", "tvl_smooth_", "tvl_smoothed_yields",
]
