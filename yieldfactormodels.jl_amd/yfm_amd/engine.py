"""Device context: one libyfm_hip context per GPU, with the panel kept resident.

Replaces the reference's per-model preallocated buffers
(``src/models/kalman/kalmanbasemodel.jl:53-69``): the panel is uploaded once and
re-used by every objective evaluation until a different panel is passed.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _lib
from .params import KIND_DNS, KIND_GNS, KIND_TVL, gamma_dim, n_params, state_dim


def _vp(x):
    """An optional raw address (``torch.Tensor.data_ptr()``, a stream handle) as a C pointer; None or 0: null."""
    return ctypes.c_void_p(x) if x else None


class Engine:
    """Owns one ``yfm_ctx`` (include/yfm.h) on ``device``."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        ctx = self.lib.yfm_create(device)
        if not ctx:
            raise _lib.YFMError(-2, self.lib.yfm_last_error().decode())
        self.ctx = ctypes.c_void_p(ctx)
        self.device = device
        self._panel = None
        self._mats = None

    def close(self):
        if self.ctx:
            self.lib.yfm_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- precision (TVλ arithmetic, include/yfm.h: yfm_set_precision) -----------------
    @property
    def precision(self) -> int:
        return self.lib.yfm_get_precision(self.ctx)

    @precision.setter
    def precision(self, mode: int) -> None:
        _lib.check(self.lib.yfm_set_precision(self.ctx, int(mode)))

    # ---- page-locked host buffers (yfm_alloc_host) ----------------------------------
    def host_array(self, shape, dtype=np.float64) -> np.ndarray:
        """A Fortran-ordered array in page-locked host memory: θ batches and loglik outputs built in
        it reach the device by DMA without a staging copy.  Freed when the array is collected."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        ptr = self.lib.yfm_alloc_host(n)
        if not ptr:
            raise _lib.YFMError(-2, self.lib.yfm_last_error().decode())
        buf = (ctypes.c_char * n).from_address(ptr)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape, order="F")
        import weakref
        weakref.finalize(buf, self.lib.yfm_free_host, ctypes.c_void_p(ptr))
        return arr

    # ---- panel -------------------------------------------------------------------
    def set_panel(self, data, maturities, force: bool = False):
        """data: N×T (maturities × months) like the reference's ``data`` matrix."""
        Y = np.asfortranarray(np.asarray(data, dtype=np.float64))
        m = np.ascontiguousarray(np.asarray(maturities, dtype=np.float64))
        if Y.ndim != 2 or m.ndim != 1 or Y.shape[0] != m.shape[0]:
            raise ValueError(f"panel must be N×T with N = len(maturities); got {Y.shape}, {m.shape}")
        if (not force and self._panel is not None and self._panel.shape == Y.shape
                and np.array_equal(self._panel, Y, equal_nan=True) and np.array_equal(self._mats, m)):
            return
        N, T = Y.shape
        _lib.check(self.lib.yfm_set_panel(self.ctx, _lib.dptr(Y), N, T, _lib.dptr(m)))
        self._panel = Y.copy(order="F")
        self._mats = m.copy()

    @property
    def T(self):
        return 0 if self._panel is None else self._panel.shape[1]

    # ---- batched evaluation ----------------------------------------------------------
    # One path per call family: the public methods below forward to these with the library symbol and what differs.
    def _grad_call(self, symbol, kind, theta, space, T_use, rows):
        """A host-pointer value-and-gradient call: (value[B], grad[rows, B]); rows None: one per row of θ."""
        Th = self._batch(theta, kind)
        P, B = Th.shape
        val = np.empty(B, dtype=np.float64)
        grad = np.empty((P if rows is None else rows, B), dtype=np.float64, order="F")
        _lib.check(getattr(self.lib, symbol)(self.ctx, kind, space, _lib.dptr(Th), P, B,
                                             _lib.iptr(self._tuse(T_use, B)), _lib.dptr(val), _lib.dptr(grad)))
        return val, grad

    def _grad_call_device(self, symbol, kind, d_theta, P, B, d_out, d_grad, space, d_T_use, stream):
        """The device-pointer twin: raw addresses in, nothing returned, asynchronous on ``stream``."""
        _lib.check(getattr(self.lib, symbol)(self.ctx, kind, space, _vp(d_theta), P, B, _vp(d_T_use), _vp(d_out),
                                             _vp(d_grad), _vp(stream)))

    def _smooth_call(self, symbol, guard, what, kind, theta, space, T_use, lag_one):
        """A host-pointer smoother call: (beta_s[M, T, B], V_s[M, M, T, B], C_s[M, M, T−1, B] or None)."""
        guard(kind, what)
        Th = self._batch(theta, kind)
        P, B = Th.shape
        M, T = state_dim(kind), self.T
        bs = np.empty((M, T, B), dtype=np.float64, order="F")
        Vs = np.empty((M, M, T, B), dtype=np.float64, order="F")
        Cs = np.empty((M, M, max(T - 1, 0), B), dtype=np.float64, order="F") if lag_one else None
        _lib.check(getattr(self.lib, symbol)(self.ctx, kind, space, _lib.dptr(Th), P, B,
                                             _lib.iptr(self._tuse(T_use, B)), _lib.dptr(bs), _lib.dptr(Vs),
                                             _lib.dptr(Cs) if lag_one else None))
        return bs, Vs, Cs

    def _smooth_call_device(self, symbol, guard, what, kind, d_theta, P, B, d_beta_s, d_V_s, d_C_s, space, d_T_use,
                            stream):
        """The device-pointer twin of :meth:`_smooth_call`."""
        guard(kind, what)
        _lib.check(getattr(self.lib, symbol)(self.ctx, kind, space, _vp(d_theta), P, B, _vp(d_T_use), _vp(d_beta_s),
                                             _vp(d_V_s), _vp(d_C_s), _vp(stream)))

    def loglik(self, kind: int, theta, space: int = 0, T_use=None, out=None) -> np.ndarray:
        """Θ: P×B (or a length-P vector).  Returns B logliks (+loglik, get_loss sign), written into
        `out` when given (e.g. a page-locked `host_array`)."""
        Th = self._batch(theta, kind)
        P, B = Th.shape
        if out is None:
            out = np.empty(B, dtype=np.float64)
        elif out.shape != (B,) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous float64 vector of length B")
        _lib.check(self.lib.yfm_loglik_batch(self.ctx, kind, space, _lib.dptr(Th), P, B,
                                             _lib.iptr(self._tuse(T_use, B)), _lib.dptr(out)))
        return out

    def loglik_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, space: int = 0,
                      d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant (raw addresses, e.g. ``torch.Tensor.data_ptr()``); asynchronous on ``stream``."""
        _lib.check(self.lib.yfm_loglik_batch_device(self.ctx, kind, space, _vp(d_theta), P, B, _vp(d_T_use),
                                                    _vp(d_out), _vp(stream)))

    def loglik_grad(self, kind: int, theta, space: int = 0, T_use=None):
        """(ll[B], grad[P, B]): the logliks of :meth:`loglik` and ∂(+loglik)/∂θ in the space passed
        (include/yfm.h yfm_loglik_grad_batch; DNS with N ≤ 64).  A candidate's gradient is NaN where its loglik
        is −Inf or NaN, and where it was evaluated on the double-double path (:meth:`last_grad_unavailable`)."""
        return self._grad_call("yfm_loglik_grad_batch", kind, theta, space, T_use, None)

    def loglik_grad_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_grad: int, space: int = 0,
                           d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`loglik_grad` (raw addresses; d_grad: P×B column-major); asynchronous
        on ``stream``."""
        self._grad_call_device("yfm_loglik_grad_batch_device", kind, d_theta, P, B, d_out, d_grad, space, d_T_use,
                               stream)

    def loglik_scores(self, kind: int, theta, space: int = 0, T_use=None):
        """(ll[B], S[P, T−1, B]): the logliks of :meth:`loglik` and the score series S[d, k, b] = ∂ℓ_k/∂θ_d, ℓ_k the
        term get_loss adds after column k — exact zeros outside a window's accumulated columns 1 … T_use − 2, NaN for
        a candidate without a gradient (include/yfm.h yfm_loglik_scores_batch; DNS with N ≤ 64)."""
        self._dns_only(kind, "loglik_scores")
        return self._scores_call("yfm_loglik_scores_batch", kind, theta, space, T_use)

    def loglik_scores_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_scores: int, space: int = 0,
                             d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`loglik_scores` (raw addresses; d_scores: P×(T−1)×B column-major);
        asynchronous on ``stream``."""
        self._dns_only(kind, "loglik_scores_device")
        self._grad_call_device("yfm_loglik_scores_batch_device", kind, d_theta, P, B, d_out, d_scores, space, d_T_use,
                               stream)

    def loglik_info(self, kind: int, theta, space: int = 0, T_use=None, lags: int = 0, step: float | None = None,
                    hessian: bool = True, opg: bool = True) -> dict:
        """ll[B], grad[P, B] (those of :meth:`loglik_grad`, bit for bit), hess[P, P, B] = ∂²ll/∂θ∂θ' (fourth-order
        central differences of the exact gradient, step ``step``; None: the library's default) and opg[P, P, B] =
        Γ₀ + Σ_ℓ (1 − ℓ/(lags+1))(Γ_ℓ + Γ_ℓ') of the score series, as a dict; ``hessian`` / ``opg`` False skips that
        half (its entry is None).  NaN matrices for a candidate without a gradient, and a NaN Hessian where one of
        its perturbed points has none (include/yfm.h yfm_loglik_info_batch; DNS with N ≤ 64)."""
        self._dns_only(kind, "loglik_info")
        return self._info_call("yfm_loglik_info_batch", "loglik_info", "loglik_grad", kind, theta, space, T_use, lags,
                               step, hessian, opg)

    def tvl_loglik_scores(self, kind: int, theta, space: int = 0, T_use=None):
        """(ll[B], S[31, T−1, B]) of the TVλ model: :meth:`loglik_scores` for the extended Kalman filter
        (include/yfm.h yfm_tvl_loglik_scores_batch) — NaN in all of a candidate that :meth:`tvl_loglik_grad` gives a
        NaN gradient."""
        self._tvl_only(kind, "tvl_loglik_scores")
        return self._scores_call("yfm_tvl_loglik_scores_batch", kind, theta, space, T_use)

    def tvl_loglik_scores_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_scores: int,
                                 space: int = 0, d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`tvl_loglik_scores` (raw addresses; d_scores: 31×(T−1)×B column-major);
        asynchronous on ``stream``."""
        self._tvl_only(kind, "tvl_loglik_scores_device")
        self._grad_call_device("yfm_tvl_loglik_scores_batch_device", kind, d_theta, P, B, d_out, d_scores, space,
                               d_T_use, stream)

    def tvl_loglik_info(self, kind: int, theta, space: int = 0, T_use=None, lags: int = 0, step: float | None = None,
                        hessian: bool = True, opg: bool = True) -> dict:
        """:meth:`loglik_info` for the TVλ model (include/yfm.h yfm_tvl_loglik_info_batch): ll[B] and grad[31, B]
        those of :meth:`tvl_loglik_grad`, bit for bit, hess[31, 31, B] from the 124 perturbed gradients per candidate
        and opg[31, 31, B] from the score series."""
        self._tvl_only(kind, "tvl_loglik_info")
        return self._info_call("yfm_tvl_loglik_info_batch", "tvl_loglik_info", "tvl_loglik_grad", kind, theta, space,
                               T_use, lags, step, hessian, opg)

    def _scores_call(self, fn: str, kind, theta, space, T_use):
        Th = self._batch(theta, kind)
        P, B = Th.shape
        ll = np.empty(B, dtype=np.float64)
        S = np.empty((P, max(self.T - 1, 0), B), dtype=np.float64, order="F")
        _lib.check(getattr(self.lib, fn)(self.ctx, kind, space, _lib.dptr(Th), P, B, _lib.iptr(self._tuse(T_use, B)),
                                         _lib.dptr(ll), _lib.dptr(S)))
        return ll, S

    def _info_call(self, fn: str, what: str, grad: str, kind, theta, space, T_use, lags, step, hessian, opg) -> dict:
        if not (hessian or opg):
            raise ValueError(f"{what}: hessian and opg are both off ({grad} gives the loglik and gradient)")
        if lags < 0:
            raise ValueError(f"lags = {lags} < 0")
        Th = self._batch(theta, kind)
        P, B = Th.shape
        ll = np.empty(B, dtype=np.float64)
        grad = np.empty((P, B), dtype=np.float64, order="F")
        H = np.empty((P, P, B), dtype=np.float64, order="F") if hessian else None
        J = np.empty((P, P, B), dtype=np.float64, order="F") if opg else None
        _lib.check(getattr(self.lib, fn)(self.ctx, kind, space, _lib.dptr(Th), P, B, _lib.iptr(self._tuse(T_use, B)),
                                         int(lags), 0.0 if step is None else float(step), _lib.dptr(ll),
                                         _lib.dptr(grad), _lib.dptr(H) if hessian else None,
                                         _lib.dptr(J) if opg else None))
        return dict(ll=ll, grad=grad, hess=H, opg=J)

    @staticmethod
    def _dns_only(kind, what):
        if kind != KIND_DNS:
            raise NotImplementedError(f"{what} is built for the DNS model (kind {KIND_DNS}) only, not kind {kind}: the "
                                      "other kinds have no score series, information matrix or Hessian")

    @staticmethod
    def _tvl_only(kind, what):
        if kind != KIND_TVL:
            gap = ("the DNS model has loglik_scores and loglik_info" if kind == KIND_DNS
                   else "only DNS and TVλ have score series, information matrices and Hessians")
            raise NotImplementedError(f"{what} is built for the TVλ model (kind {KIND_TVL}) only, not kind {kind}: {gap}")

    def tvl_loglik_grad(self, kind: int, theta, space: int = 0, T_use=None):
        """(ll[B], grad[31, B]) of the TVλ model: the logliks of :meth:`loglik`, bit for bit under the context's
        precision, and ∂(+loglik)/∂θ in the space passed from the FP64 tangent recursion (include/yfm.h
        yfm_tvl_loglik_grad_batch).  A candidate's gradient is NaN where its loglik is −Inf or NaN, and where the
        tangent recursion's own value or tangents are not usable (:meth:`last_grad_unavailable`)."""
        return self._grad_call("yfm_tvl_loglik_grad_batch", kind, theta, space, T_use, None)

    def tvl_loglik_grad_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_grad: int, space: int = 0,
                               d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`tvl_loglik_grad` (raw addresses; d_grad: 31×B column-major); asynchronous
        on `stream`, with the ordering rules of :meth:`loglik_device`."""
        self._grad_call_device("yfm_tvl_loglik_grad_batch_device", kind, d_theta, P, B, d_out, d_grad, space,
                               d_T_use, stream)

    def lambda_loss_grad(self, kind: int, theta, space: int = 0, T_use=None):
        """(loss[B], grad[12, B]) of a λ model: get_loss as :meth:`loglik` returns it, bit for bit, and its
        derivative with respect to δ(3) and vec Φ(9, column-major) — θ's last 12 rows — in the space passed
        (include/yfm.h yfm_lambda_loss_grad_batch).  A candidate's gradient is NaN where its loss is −Inf."""
        return self._grad_call("yfm_lambda_loss_grad_batch", kind, theta, space, T_use, 12)

    def lambda_loss_grad_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_grad: int,
                                space: int = 0, d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`lambda_loss_grad` (raw addresses; d_grad: 12×B column-major);
        asynchronous on ``stream``."""
        self._grad_call_device("yfm_lambda_loss_grad_batch_device", kind, d_theta, P, B, d_out, d_grad, space,
                               d_T_use, stream)

    def lambda_loss_full_grad(self, kind: int, theta, space: int = 0, T_use=None):
        """(loss[B], grad[P, B]) of a λ model: get_loss as :meth:`loglik` returns it, bit for bit, and its derivative
        with respect to every row of θ in the space passed (include/yfm.h yfm_lambda_loss_fullgrad_batch) — the
        leading rows (A, B, ω; γ for NS) from the tangent of the score recursion, the last 12 the rows of
        :meth:`lambda_loss_grad`, bit for bit.  A candidate's gradient is NaN where its loss is −Inf, and where a
        tangent is not finite (:meth:`last_grad_unavailable`)."""
        return self._grad_call("yfm_lambda_loss_fullgrad_batch", kind, theta, space, T_use, None)

    def lambda_loss_full_grad_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_grad: int,
                                     space: int = 0, d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`lambda_loss_full_grad` (raw addresses; d_grad: P×B column-major);
        asynchronous on ``stream``."""
        self._grad_call_device("yfm_lambda_loss_fullgrad_batch_device", kind, d_theta, P, B, d_out, d_grad, space,
                               d_T_use, stream)

    def neural_loss_grad(self, kind: int, theta, space: int = 0, T_use=None):
        """:meth:`lambda_loss_grad` for a neural kind (include/yfm.h yfm_neural_loss_grad_batch): (loss[B],
        grad[12, B]), the loss :meth:`loglik`'s bit for bit, the gradient NaN where it is −Inf."""
        return self._grad_call("yfm_neural_loss_grad_batch", kind, theta, space, T_use, 12)

    def neural_loss_grad_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_grad: int,
                                space: int = 0, d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`neural_loss_grad` (raw addresses; d_grad: 12×B column-major);
        asynchronous on ``stream``."""
        self._grad_call_device("yfm_neural_loss_grad_batch_device", kind, d_theta, P, B, d_out, d_grad, space,
                               d_T_use, stream)

    def neural_loss_full_grad(self, kind: int, theta, space: int = 0, T_use=None):
        """:meth:`lambda_loss_full_grad` for a neural kind (include/yfm.h yfm_neural_loss_fullgrad_batch): (loss[B],
        grad[P, B]) — the loss :meth:`loglik`'s bit for bit, the leading rows (A, B, ω; γ for the static kinds) from an
        adjoint sweep over the score recursion, the last 12 the rows of :meth:`neural_loss_grad`, bit for bit.  A
        candidate's gradient is NaN where its loss is −Inf, and where an adjoint is not finite
        (:meth:`last_grad_unavailable`)."""
        return self._grad_call("yfm_neural_loss_fullgrad_batch", kind, theta, space, T_use, None)

    def neural_loss_full_grad_device(self, kind: int, d_theta: int, P: int, B: int, d_out: int, d_grad: int,
                                     space: int = 0, d_T_use: int | None = None, stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`neural_loss_full_grad` (raw addresses; d_grad: P×B column-major);
        asynchronous on ``stream``."""
        self._grad_call_device("yfm_neural_loss_fullgrad_batch_device", kind, d_theta, P, B, d_out, d_grad, space,
                               d_T_use, stream)

    def filter_states(self, kind: int, theta, space: int = 0, T_use=None):
        """Returns (loglik[B], beta[M, T-1, B], P[M, M, T-1, B]) — a_{t+1|t}, P_{t+1|t} after each filter! call."""
        Th = self._batch(theta, kind)
        P, B = Th.shape
        M = state_dim(kind)
        T = self.T
        out = np.empty(B)
        beta = np.empty((M, max(T - 1, 0), B), order="F")
        Pm = np.empty((M, M, max(T - 1, 0), B), order="F")
        _lib.check(self.lib.yfm_filter_states(self.ctx, kind, space, _lib.dptr(Th), P, B,
                                              _lib.iptr(self._tuse(T_use, B)), _lib.dptr(beta), _lib.dptr(Pm),
                                              _lib.dptr(out)))
        return out, beta, Pm

    @staticmethod
    def _smooth_kinds(kind, what):
        if kind not in (KIND_DNS, KIND_GNS):
            gap = ("the TVλ model's extended smoother is tvl_smooth" if kind == KIND_TVL
                   else "the λ and neural kinds are not Kalman filters and have no state covariance to smooth")
            raise NotImplementedError(f"{what} is built for the DNS and GNS5 models (kinds {KIND_DNS}, {KIND_GNS}), not "
                                      f"kind {kind}: {gap}")

    def smooth(self, kind: int, theta, space: int = 0, T_use=None, lag_one: bool = True):
        """(beta_s[M, T, B], V_s[M, M, T, B], C_s[M, M, T−1, B] or None): the fixed-interval smoother of the DNS and
        GNS5 models (include/yfm.h yfm_smooth_batch) — β̂_t = E[β_t | y_1..n] in slot t − 1, its covariance V_t and,
        ``lag_one``, C_t = Cov(β_{t+1}, β_t | y_1..n), with n = T_use[b] (None: every column).  NaN beyond a window, and
        in all of a candidate whose loglik is −Inf or NaN, that was evaluated on the double-double path or that has an
        output that is not finite (:meth:`last_grad_unavailable` counts them)."""
        return self._smooth_call("yfm_smooth_batch", self._smooth_kinds, "smooth", kind, theta, space, T_use, lag_one)

    def smooth_device(self, kind: int, d_theta: int, P: int, B: int, d_beta_s: int, d_V_s: int,
                      d_C_s: int | None = None, space: int = 0, d_T_use: int | None = None,
                      stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`smooth` (raw addresses; d_beta_s M×T×B, d_V_s M×M×T×B, d_C_s M×M×(T−1)×B
        column-major or None); asynchronous on ``stream``."""
        self._smooth_call_device("yfm_smooth_batch_device", self._smooth_kinds, "smooth_device", kind, d_theta, P, B,
                                 d_beta_s, d_V_s, d_C_s, space, d_T_use, stream)

    @staticmethod
    def _tvl_smooth_kinds(kind, what):
        if kind != KIND_TVL:
            gap = ("the fixed-loading models' smoother is smooth" if kind in (KIND_DNS, KIND_GNS)
                   else "the λ and neural kinds are not Kalman filters: there is nothing to smooth")
            raise NotImplementedError(f"{what} is built for the TVλ model (kind {KIND_TVL}), not kind {kind}: {gap}")

    def tvl_smooth(self, kind: int, theta, space: int = 0, T_use=None, lag_one: bool = True):
        """(beta_s[4, T, B], V_s[4, 4, T, B], C_s[4, 4, T−1, B] or None): the extended Kalman smoother of the TVλ model
        (include/yfm.h yfm_tvl_smooth_batch), linearised once at the forward pass's predicted states — β̂_t =
        E[β_t | y_1..n] in slot t − 1, its covariance V_t and, ``lag_one``, C_t = Cov(β_{t+1}, β_t | y_1..n), with
        n = T_use[b] (None: every column).  NaN beyond a window, and in all of a candidate whose loglik is −Inf or NaN,
        that has a data column with det(σ²I + P_tG_t) ≤ 0 or an output that is not finite
        (:meth:`last_grad_unavailable` counts them)."""
        return self._smooth_call("yfm_tvl_smooth_batch", self._tvl_smooth_kinds, "tvl_smooth", kind, theta, space,
                                 T_use, lag_one)

    def tvl_smooth_device(self, kind: int, d_theta: int, P: int, B: int, d_beta_s: int, d_V_s: int,
                          d_C_s: int | None = None, space: int = 0, d_T_use: int | None = None,
                          stream: int | None = None) -> None:
        """Device-pointer variant of :meth:`tvl_smooth` (raw addresses; d_beta_s 4×T×B, d_V_s 4×4×T×B, d_C_s
        4×4×(T−1)×B column-major or None); asynchronous on ``stream``."""
        self._smooth_call_device("yfm_tvl_smooth_batch_device", self._tvl_smooth_kinds, "tvl_smooth_device", kind,
                                 d_theta, P, B, d_beta_s, d_V_s, d_C_s, space, d_T_use, stream)

    @staticmethod
    def _batch(theta, kind):
        Th = np.asfortranarray(np.atleast_2d(np.asarray(theta, dtype=np.float64).T).T)
        if Th.shape[0] != n_params(kind):
            raise ValueError(f"theta has {Th.shape[0]} rows, model kind {kind} needs {n_params(kind)}")
        return Th

    @staticmethod
    def _tuse(T_use, B):
        return None if T_use is None else np.ascontiguousarray(np.broadcast_to(T_use, (B,)), dtype=np.int32)

    def predict(self, kind: int, theta, space: int = 1, T_use=None, horizon: int = 1) -> dict:
        """predict (filter.jl:250-282) per θ_b on hcat(data[:, :T_b], NaN × (horizon−1)).
        Returns arrays with a trailing batch axis: preds/factor_loadings_1/2 (N, ncol, B),
        factors (M, ncol, B), states (L, ncol, B), ncol = T + horizon − 1."""
        Th = self._batch(theta, kind)
        P, B = Th.shape
        M, L, N = state_dim(kind), gamma_dim(kind), self._panel.shape[0]
        ncol = self.T + horizon - 1
        preds = np.empty((N, ncol, B), order="F")
        fl1 = np.empty((N, ncol, B), order="F")
        fl2 = np.empty((N, ncol, B), order="F")
        fac = np.empty((M, ncol, B), order="F")
        st = np.empty((L, ncol, B), order="F")
        _lib.check(self.lib.yfm_predict(self.ctx, kind, space, _lib.dptr(Th), P, B, _lib.iptr(self._tuse(T_use, B)),
                                        horizon, _lib.dptr(preds), _lib.dptr(fac), _lib.dptr(st), _lib.dptr(fl1),
                                        _lib.dptr(fl2)))
        return dict(preds=preds, factors=fac, states=st, factor_loadings_1=fl1, factor_loadings_2=fl2)

    def forecast(self, kind: int, theta, space: int = 1, T_use=None, horizon: int = 1) -> np.ndarray:
        """forecasting.jl:236-250 blocks vcat(factors, states, preds)[:, end-h+1:end]: (M+L+N, h, B)."""
        Th = self._batch(theta, kind)
        P, B = Th.shape
        R = state_dim(kind) + gamma_dim(kind) + self._panel.shape[0]
        out = np.empty((R, horizon, B), order="F")
        _lib.check(self.lib.yfm_forecast(self.ctx, kind, space, _lib.dptr(Th), P, B, _lib.iptr(self._tuse(T_use, B)),
                                         horizon, _lib.dptr(out)))
        return out

    def loss_array(self, kind: int, theta, space: int = 1, T_use=None, K: int = 1) -> np.ndarray:
        """get_loss_array (filter.jl:211-247) per θ_b: (T−1, B)."""
        Th = self._batch(theta, kind)
        P, B = Th.shape
        out = np.empty((max(self.T - 1, 0), B), order="F")
        _lib.check(self.lib.yfm_loss_array(self.ctx, kind, space, _lib.dptr(Th), P, B,
                                           _lib.iptr(self._tuse(T_use, B)), K, _lib.dptr(out)))
        return out

    def estimate(self, kind: int, theta0, space: int = 1, T_use=None, iterations: int = 500, g_tol: float = 1e-6,
                 max_group_iters: int = 10, tol: float = 1e-8) -> dict:
        """Batched estimate_steps! (optimization.jl:137-312): one Nelder–Mead chain per column of Θ₀ (P×R),
        on window T_use[r].  Returns theta_c (P×R), p (P×R unconstrained), init_c (P×R: the reference's
        init_p — the sanitised, rescaled start, constrained), ll (R), status (R), n_evals."""
        Th = self._batch(theta0, kind)
        P, R = Th.shape
        th_c = np.empty((P, R), order="F")
        p = np.empty((P, R), order="F")
        init_c = np.empty((P, R), order="F")
        ll = np.empty(R)
        st = np.empty(R, dtype=np.int32)
        ne = ctypes.c_longlong(0)
        _lib.check(self.lib.yfm_estimate(self.ctx, kind, space, _lib.dptr(Th), P, R, _lib.iptr(self._tuse(T_use, R)),
                                         iterations, g_tol, max_group_iters, tol, _lib.dptr(th_c), _lib.dptr(p),
                                         _lib.dptr(init_c), _lib.dptr(ll), _lib.iptr(st), ctypes.byref(ne)))
        return dict(theta_c=th_c, p=p, init_c=init_c, ll=ll, status=st, n_evals=ne.value)

    def nm_block(self, kind: int, p, idx, T_use=None, iterations: int = 500, g_tol: float = 1e-6):
        """One Optim.NelderMead run per column of p (P×R, unconstrained) on the coordinates ``idx`` (0-based rows of
        θ), the rest held (include/yfm.h yfm_nm_block).  Returns (p with the block at its minimiser — a copy —,
        f[R] = compute_loss there, n_evals).  f is NaN, and the column unchanged, where the objective threw."""
        X = self._batch(p, kind).copy(order="F")
        P, R = X.shape
        ix = np.ascontiguousarray(idx, dtype=np.int32)
        f = np.empty(R)
        ne = ctypes.c_longlong(0)
        _lib.check(self.lib.yfm_nm_block(self.ctx, kind, _lib.dptr(X), P, R, _lib.iptr(self._tuse(T_use, R)),
                                         _lib.iptr(ix), len(ix), iterations, g_tol, _lib.dptr(f), ctypes.byref(ne)))
        return X, f, ne.value

    def last_flags(self):
        a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
        _lib.check(self.lib.yfm_last_batch_flags(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def last_deferred(self) -> int:
        """Candidates of the last batch evaluated on the double-double capacitance path (fixed-loading
        models with an ill-conditioned Z'Z; include/yfm.h yfm_last_batch_deferred)."""
        n = ctypes.c_longlong(0)
        _lib.check(self.lib.yfm_last_batch_deferred(self.ctx, ctypes.byref(n)))
        return n.value

    def last_grad_unavailable(self) -> int:
        """Candidates of the last gradient batch whose loglik came from the double-double path and whose
        gradient is therefore NaN (include/yfm.h yfm_last_batch_grad_unavailable)."""
        n = ctypes.c_longlong(0)
        _lib.check(self.lib.yfm_last_batch_grad_unavailable(self.ctx, ctypes.byref(n)))
        return int(n.value)

    def last_steady(self) -> int:
        """Wave-steps (64 filter steps each) of the last batch that ran the DNS kernel's frozen-covariance
        steady state (include/yfm.h yfm_last_batch_steady)."""
        n = ctypes.c_longlong(0)
        _lib.check(self.lib.yfm_last_batch_steady(self.ctx, ctypes.byref(n)))
        return int(n.value)


_engines: dict[int, Engine] = {}
_lock = threading.Lock()


def get_engine(device: int = 0) -> Engine:
    with _lock:
        e = _engines.get(device)
        if e is None:
            e = Engine(device)
            _engines[device] = e
        return e
