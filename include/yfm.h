/*
 * yfm.h — C ABI of libyfm_hip.so: the batched Kalman-filter log-likelihood of
 * YieldFactorModels.jl on MI355X (gfx950).
 *
 * The reference has no FFI on this path; its plug-in point is Julia multiple
 * dispatch.  Each entry point below names the reference function it replaces
 * (paths relative to the reference root) — the Julia-side `@ccall` binding a
 * maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *   - All arrays are plain host (or, for *_device, device) pointers with explicit
 *     sizes.  Matrices are column-major like Julia's: the panel Y is N×T
 *     (rows = maturities, columns = months, data_management.jl:1-5) and a batch
 *     of parameter vectors Θ is P×B (candidate b is Θ[:, b], contiguous).
 *   - FP64 throughout (the reference's Float64 path, test.jl:25).
 *   - Return value: YFM_OK (0) or a negative yfm_status; yfm_last_error() then
 *     holds a thread-local message.  Numeric failures of one candidate are NOT
 *     errors: they are written into that candidate's output (see below).
 *   - A context is bound to one HIP device and is not thread-safe; use one
 *     context per host thread / per GPU.  Host-pointer calls are synchronous.
 *
 * Per-candidate numeric semantics (bitwise the reference's values)
 *   loglik_out[b] = +loglik as returned by get_loss (filter.jl:182-209):
 *     -Inf  where the reference returns -Inf (det F < 0 at t ≥ 2: DomainError in
 *           logdet, filter.jl:197-200; any non-finite loglik, filter.jl:202-204);
 *     NaN   where the reference would THROW from initialize_filter (singular
 *           I − Φ or I − Φ⊗Φ, filter.jl:4,7) — counted in n_init_throw.
 */
#ifndef YFM_H
#define YFM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YFM_ABI_VERSION 5

typedef struct yfm_ctx yfm_ctx;

/* model_kind — create_model codes (src/model_dictionary.jl:11-16) */
enum yfm_model_kind {
  YFM_MODEL_DNS = 0,  /* "1C" / "0": DNSModel, fixed λ, M = 3, P = 20 (dns.jl) */
  YFM_MODEL_TVL = 1,  /* "TVλ" / "1": TVλDNSModel EKF, M = 4, P = 31 (tvλdns.jl) */
  YFM_MODEL_GNS5 = 2, /* extension, not in the reference: 5-factor generalised NS, M = 5, P = 48 */
  /* The static and score-driven λ models of src/models/filter.jl:52-110 (model_dictionary.jl:17-35): not Kalman
   * filters.  M = 3 factors, L = 1 observation-driven parameter γ = log(λ − 0.01).  θ_c = [A, B, ω, δ(3), vec Φ(9)]
   * (msedriven/paramteroperations.jl:25-65), Φ COLUMN-major (reshape), without B for the random-walk variants and
   * [γ, δ(3), vec Φ(9)] for NS (static/paramteroperations.jl:19-43).  Unconstrained space: A → exp,
   * B → 1/(1 + e^−x), the diagonal of Φ → from_R_to_11, the rest identity (mselambda.jl:17-34, msebasemodel.jl:77-90).
   * For these kinds loglik_out is get_loss of src/models/filter.jl:209-243 — minus the mean squared one-step
   * prediction error, mse/N/nobs — and −Inf where that returns −Inf (a non-finite running sum: a NaN anywhere in a
   * compared column, or a step whose OLS fails twice, filter.jl:62-67, :122-137).  Nothing throws at
   * initialisation: n_init_throw stays 0.  Value 7 is not a kind.  The two scaled kinds evaluate their score at the
   * refined OLS β (csrc/yfm_msed.hpp): where the Float64 reference's score is rounding noise (N = 3) they follow the
   * exact recursion, not the noise. */
  YFM_MODEL_NS = 3,      /* "NS" / "2": StaticλModel, P = 13 (staticlambda.jl) */
  YFM_MODEL_SD_NS = 4,   /* "SD-NS" / "4": MSEDλModel, P = 15 (mselambda.jl) */
  YFM_MODEL_RWSD_NS = 5, /* "RWSD-NS" / "5": random walk γ (no B), P = 14 */
  YFM_MODEL_SSD_NS = 6,  /* "SSD-NS" / "6": score scaled by its EWMA root (filter.jl:29-44, f = 0.98), P = 15 */
  YFM_MODEL_SRWSD_NS = 8, /* "SRWSD-NS" / "7": scaled, random walk, P = 14 */
  /* The neural Nelson–Siegel models (ABI 5; model_dictionary.jl:20-112, mseneural.jl, staticneural.jl): the same
   * filter with L = 18 — γ[0..8] drives Z₂ and γ[9..17] drives Z₃, each block [w₁(3), b(3), w₂(3)] of a 1→3→1 tanh
   * network without output bias, followed by the transforms of src/utils/neural_network_transform.jl (the
   * -Anchored kinds: transform_bool = false).  tanh is the mathematical function.  θ_c = [γ(18), δ(3), vec Φ(9)],
   * P = 30, for the static kinds and [A_unique, B_unique (absent for random walk), ω(18), δ(3), vec Φ(9)] for the
   * score-driven ones, whose duplicator (`dynamics`) expands 2 (scalar: 9 + 9), 6 (block_diag: 3 each) or 18
   * (diag) unique values: P = 34 / 42 / 66, random walk 32 / 36 / 48.  Unconstrained space: A → exp,
   * B → 1/(1 + e^−x), the diagonal of Φ → from_R_to_11.  The scaled kinds' EWMA is per component with f = 0.9.
   * 4 ≤ N ≤ 1024 (below 4 the transforms' anchor slots alias): other N return YFM_EUNSUPPORTED, as do
   * yfm_estimate, yfm_filter_states, yfm_loglik_grad_batch and yfm_lambda_loss_grad_batch for these kinds (their
   * δ/Φ loss gradient is yfm_neural_loss_grad_batch).
   * yfm_predict's states are 18×n per candidate and a yfm_forecast block has 3 + 18 + N rows. */
  YFM_MODEL_NNS = 16,          /* "NNS" / "3": StaticNeuralModel */
  YFM_MODEL_NNS_ANCHORED = 17, /* "NNS-Anchored" / "20" */
  /* score-driven: YFM_MODEL_SD_NNS | dynamics | YFM_NNS_RW | YFM_NNS_SCALED | YFM_NNS_ANCHORED, dynamics 0 scalar
   * ("1…"), 1 block_diag ("2…"), 2 diag ("3…"); value 3 in the low two bits is not a kind.  Reference codes
   * "8" … "19" are {1,2,3}{SD,RWSD}-NNS then {1,2,3}{SSD,SRWSD}-NNS, "21" … "32" the same with -Anchored:
   *   32 "1SD-NNS"/"8"    36 "1RWSD-NNS"/"9"    33 "2SD-NNS"/"10"   37 "2RWSD-NNS"/"11"   34 "3SD-NNS"/"12"   38 "3RWSD-NNS"/"13"
   *   40 "1SSD-NNS"/"14"  44 "1SRWSD-NNS"/"15"  41 "2SSD-NNS"/"16"  45 "2SRWSD-NNS"/"17"  42 "3SSD-NNS"/"18"  46 "3SRWSD-NNS"/"19"
   *   48 … 54 and 56 … 62: the same with "-Anchored", codes "21" … "26" and "27" … "32" */
  YFM_MODEL_SD_NNS = 32,
  YFM_NNS_RW = 4,        /* random walk γ: no B */
  YFM_NNS_SCALED = 8,    /* scale_grad */
  YFM_NNS_ANCHORED = 16  /* transform_bool = false */
};

/* param_space */
enum yfm_param_space {
  YFM_THETA_UNCONSTRAINED = 0, /* θ as compute_loss receives it (optimization.jl:10-23) */
  YFM_THETA_CONSTRAINED = 1    /* θ_c as set_params! receives it (paramoperations.jl:6-68) */
};

enum yfm_status {
  YFM_OK = 0,
  YFM_EINVAL = -1,      /* bad argument (sizes, kind, pointer) */
  YFM_EHIP = -2,        /* HIP runtime error */
  YFM_ENOPANEL = -3,    /* no panel set on this context */
  YFM_EUNSUPPORTED = -4 /* valid request this build has no kernel for */
};

/* precision — the arithmetic of the TVλ EKF (the fixed-loading models always run their FP64
 * collapsed form, whose filter contracts, with ill-conditioned-loading candidates evaluated in
 * double-double — see yfm_last_batch_deferred)
 *   YFM_PREC_CERTIFIED (default)  TVλ in double-double (~106-bit) arithmetic.  A share of TVλ
 *       candidates amplify any FP64 rounding by 1e10..1e20 over T = 600 steps, so no FP64
 *       evaluation — the reference's own dense path included — is then within 1e-9 of the
 *       exact value of filter.jl:12-80; this mode returns that value to ~1e-13 (every candidate of
 *       a 1,024-candidate config-3 sample within 1.6e-10 of a binary128 restatement, where the
 *       reference's dense FP64 path is up to 1.1e-2 from it).  ≈4× the cost of FP64.
 *   YFM_PREC_FP64  FP64 throughout, the fastest path — the reference's arithmetic class, not a
 *       certified mode: on the rounding-amplifying candidates every FP64 result, the reference's
 *       included, is rounding noise around the exact value (on the 1,024-candidate sample this mode
 *       is closer to it than the reference's dense path at the median, p99 and max — 6.7e-3 vs
 *       1.1e-2 — but either can be the closer one on a given candidate).  Off the configuration
 *       shapes its tail is wider than the reference's: on 72,947 random candidates (N 1..96, starts far
 *       from the data) p99 3.7e-9 vs 6.1e-10, 104 vs 40 above 1e-6 — the capacitance form's
 *       (v'v − u'Wu)/σ² cancels where the dense form does not.  Use YFM_PREC_CERTIFIED for
 *       results that must not depend on rounding. */
enum yfm_precision { YFM_PREC_CERTIFIED = 0, YFM_PREC_FP64 = 1 };

/* Library/ABI introspection. */
int yfm_abi_version(void);
/* Length P of θ for a model kind (kalmanbasemodel.jl:106-112 + dns.jl:15-22). */
int yfm_param_count(int model_kind);
/* State dimension M (3 DNS, 4 TVλ, 5 GNS5; 3 for the λ kinds NS .. SRWSD-NS, P = 13 / 15 / 14 / 15 / 14). */
int yfm_state_dim(int model_kind);
/* Thread-local message for the last failing call on this thread ("" if none). */
const char* yfm_last_error(void);

/* Context lifetime.  Replaces the per-model preallocated buffers of
 * KalmanBaseModel (kalmanbasemodel.jl:46-130): device buffers live in the ctx. */
yfm_ctx* yfm_create(int hip_device);
void yfm_destroy(yfm_ctx* ctx);

/* Select the TVλ arithmetic for subsequent calls on this context (default YFM_PREC_CERTIFIED).
 * The reference has no such switch: its Float64 path is YFM_PREC_FP64's arithmetic class. */
int yfm_set_precision(yfm_ctx* ctx, int precision);
int yfm_get_precision(yfm_ctx* ctx);

/* Page-locked host memory for the host-pointer entry points: θ batches and output buffers
 * allocated here are copied by DMA without a staging pass (the caller keeps the Julia/Python
 * array view; free with yfm_free_host).  NULL on failure (yfm_last_error). */
void* yfm_alloc_host(size_t bytes);
int yfm_free_host(void* p);

/* Upload the yield panel.  Y: N×T column-major (the `data` argument of get_loss,
 * filter.jl:182); maturities: N (KalmanBaseModel.maturities).  Copied; the
 * caller keeps ownership.  NaN columns are allowed (prediction-only steps). */
int yfm_set_panel(yfm_ctx* ctx, const double* Y, int N, int T, const double* maturities);

/* Batched log-likelihood — replaces B calls of
 *   compute_loss(model, data, θ_b)  (optimization.jl:10-23; loglik = -loss) when
 *   param_space = YFM_THETA_UNCONSTRAINED, or
 *   set_params!(model, θ_b); get_loss(model, data)  (filter.jl:182-209)
 *   when param_space = YFM_THETA_CONSTRAINED.
 * theta: P×B column-major.  T_use: NULL (every candidate uses all T columns) or
 * B window lengths, candidate b then evaluates get_loss(model, data[:, 1:T_use[b]])
 * (the expanding-window re-estimation of forecasting.jl:140-176), 1 ≤ T_use[b] ≤ T.
 * loglik_out: B doubles.  Synchronous.
 * For YFM_MODEL_NS .. YFM_MODEL_SRWSD_NS get_loss is src/models/filter.jl:209-243 (a window of one column gives
 * 0.0; the divisor is nobs); a candidate's value is bitwise independent of the batch it is evaluated in. */
int yfm_loglik_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                     const int* T_use, double* loglik_out);

/* Same with DEVICE pointers on the caller's HIP stream (hipStream_t passed as
 * void*, NULL = default stream); asynchronous: returns after enqueueing.  For
 * pipelines that keep Θ resident in HBM (bench.py, RCCL sharding).  A context's
 * device scratch and counters serve one launch at a time: consecutive launches on
 * the same stream are ordered by the stream; a caller that moves to another stream
 * orders the two itself (hipStreamWaitEvent or a synchronisation), as for any HIP
 * work sharing buffers.  The library never touches a previous launch's stream. */
int yfm_loglik_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                            const int* d_T_use, double* d_loglik_out, void* hip_stream);

/* Filtered-state trajectories for parity checks: after every filter! call t
 * (t = 1..T-1), beta and P hold a_{t+1|t}, P_{t+1|t} (filter.jl:125-179).
 * beta_out: M × (T-1) × B, P_out: M × M × (T-1) × B (column-major), loglik_out: B.
 * Meant for small B (the output is O(B·T·M²)).  Synchronous.  Kalman kinds only: the λ kinds have no
 * covariance and return YFM_EUNSUPPORTED (their trajectory is yfm_predict's). */
int yfm_filter_states(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                      const int* T_use, double* beta_out, double* P_out, double* loglik_out);

/* Length L of base.gamma, the observation-driven parameters predict reports as
 * `states` (kalmanbasemodel.jl:58): 1 for DNS (dns.jl:18) and TVλ (tvλdns.jl:19,
 * never set, so zeros), 2 for the GNS5 extension, 1 for the λ kinds (γ_t, mselambda.jl:29). */
int yfm_gamma_dim(int model_kind);

/* Batched predict — replaces, per candidate b,
 *   set_params!(model, θ_b); predict(model, hcat(Y[:, 1:T_b], fill(NaN, N, horizon-1)))
 * (filter.jl:250-282 on the NaN padding of forecasting.jl:141/161/242); horizon = 1
 * is predict(model, Y[:, 1:T_b]).  T_b = T_use[b] (or T when T_use is NULL).
 * Outputs, column-major with ncol = T + horizon - 1 columns per candidate (candidate
 * b's columns beyond T_b + horizon - 1 are NaN):
 *   preds N×ncol×B (preds[:, j] = ŷ for observation j+1), factors M×ncol×B,
 *   states L×ncol×B (L = yfm_gamma_dim), loadings_1 / loadings_2 N×ncol×B (Z[:,2],
 *   Z[:,3]; either may be NULL).  A candidate whose initialize_filter would throw
 *   gets NaN everywhere.  Synchronous.
 * λ kinds: predict of src/models/filter.jl:284-306 — column j holds the prediction, β, γ and Z[:,2], Z[:,3]
 * AFTER the step on observation j; a step that returns −Inf (filter.jl:62-67) gives a −Inf prediction column
 * and leaves the state as the failing call left it. */
int yfm_predict(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B, const int* T_use,
                int horizon, double* preds, double* factors, double* states, double* loadings_1,
                double* loadings_2);

/* Forecast blocks of the rolling-window driver (forecasting.jl:236-250):
 *   res = vcat(factors[:, end-h+1:end], states[:, end-h+1:end], preds[:, end-h+1:end])
 * of the predict call above, h = horizon.  out: (M+L+N) × h × B column-major.  This
 * is the per-task record run_forecast_window_database stores (forecasting.jl:181-184). */
int yfm_forecast(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B, const int* T_use,
                 int horizon, double* out);

/* Batched get_loss_array(model, Y[:, 1:T_b]; K) (filter.jl:211-247): mse_out (T-1)×B,
 * column b holds the T_b - 1 per-step values -‖y_t - ŷ_t‖²/N/K (entry 1 is 0, as in
 * the reference) followed by NaN.  A candidate for which the reference returns the
 * scalar -Inf (a non-finite step) gets -Inf in all its entries; NaN where
 * initialize_filter would throw.  K > 1 passes continue the filter state, as in the
 * reference; K > 1 requires T_use = NULL.  Synchronous.
 * λ kinds: get_loss_array of src/models/filter.jl:245-281 — entry t is −‖y_{t+1} − ŷ_t‖²/N/K and entry 1 is a
 * real value; K = 1 only (K > 1 returns YFM_EUNSUPPORTED). */
int yfm_loss_array(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                   const int* T_use, int K, double* mse_out);

/* Batched estimation — replaces R calls of estimate_steps! (optimization.jl:137-312) for
 * a Kalman model with every parameter in group "1" (kalmanbasemodel.jl:150-159), i.e.
 * block-coordinate Nelder–Mead (Optim.NelderMead(), opt1: `iterations`, `g_tol`;
 * optimization.jl:442-451, :479) with the outer loop max_group_iters / |ΔLL| < tol.
 * Chain r starts from theta0[:, r] (param_space as above; the reference receives
 * constrained all_params and untransforms them) on the window Y[:, 1:T_use[r]] (or all
 * T columns when T_use is NULL).  The R chains' objective evaluations are batched into
 * one device launch per round.  Outputs: theta_c_out P×R = transform_params(best_p)
 * (the reference's returned params), p_out P×R unconstrained optimum (or NULL), init_c_out P×R
 * (or NULL) = transform_params of the sanitised, ×0.95-rescaled start (the reference's returned
 * init_p, optimization.jl:157-184, :298-302), ll_out R
 * (the reference's returned ll), status_out R (or NULL): 0 ok, 1 the reference would
 * throw (NaN outputs), 2 aborted after the first group iteration (parameters kept);
 * n_evals_out (or NULL): objective evaluations performed.  Synchronous.  Kalman kinds only: the λ kinds'
 * parameter groups need other optimisers (optimization.jl:442-479) and return YFM_EUNSUPPORTED. */
int yfm_estimate(yfm_ctx* ctx, int model_kind, int param_space, const double* theta0, int P, int R,
                 const int* T_use, int iterations, double g_tol, int max_group_iters, double tol,
                 double* theta_c_out, double* p_out, double* init_c_out, double* ll_out, int* status_out,
                 long long* n_evals_out);

/* Counters of the last completed batch on this ctx: candidates where the
 * reference would have thrown (NaN outputs) and candidates returning -Inf.
 * For yfm_loglik_batch_device, synchronise the stream first. */
int yfm_last_batch_flags(yfm_ctx* ctx, long long* n_init_throw, long long* n_neg_inf);

/* Candidates of the last completed batch on this ctx that the fixed-loading models (DNS, GNS5)
 * evaluated on the double-double capacitance path instead of the FP64 collapsed form: an
 * ill-conditioned loading Gram matrix (κ₁(Z'Z) ≥ 1e6), a singular one, or fewer maturities than
 * states.  Same filter!/get_loss semantics (filter.jl:125-209); reported for auditing the cost
 * and accuracy split (0 for TVλ).  For yfm_loglik_batch_device, synchronise the stream first. */
int yfm_last_batch_deferred(yfm_ctx* ctx, long long* n_deferred);

/* Wave-steps of the last batch that ran in the DNS / GNS5 kernel's frozen-covariance steady state (64
 * filter steps each: the mean update only at the converged P — DNS with the factors of S = P + R
 * cached, GNS5 refactoring the constant S — DESIGN.md §3.1).  The covariance recursion of filter.jl:158-176 does not depend on the data when the
 * loadings are fixed; a candidate freezes its P once the change per step is at the rounding level, at a
 * step that depends on its own θ only.  YFM_DNS_STEADY=0 in the environment disables it.  0 for the
 * other models, for trajectories and for panels shorter than 80 columns (full recursion there). */
int yfm_last_batch_steady(yfm_ctx* ctx, long long* steady_wave_steps);

/* Batched log-likelihood WITH its gradient — replaces, per candidate, the value and the ForwardDiff
 * gradient that estimate! asks for (optimization.jl:367, TwiceDifferentiable(...; autodiff=:forward))
 * of compute_loss (optimization.jl:10-23), with the sign of get_loss: loglik_out[b] is what
 * yfm_loglik_batch returns and grad_out[:, b] (P×B column-major) = ∂(+loglik)/∂θ_i in the space the
 * caller passed — the unconstrained space includes the derivatives of exp and of from_R_to_11
 * (transformations.jl:2-4, :21-26); the constrained space is the derivative with respect to θ_c itself.
 * The gradient is exact (forward-mode tangents of the full filter recursion, quirks of filter.jl:190-206
 * included: t = 1 not accumulated, the last column unused, a NaN column a prediction-only step whose
 * stale F/v term — and its tangent — is added again).  YFM_MODEL_DNS with N ≤ 64 only: TVλ (served by
 * yfm_tvl_loglik_grad_batch below), GNS5 and
 * larger N return YFM_EUNSUPPORTED.  grad_out[:, b] is NaN in all P entries where loglik_out[b] is −Inf
 * (n_neg_inf) or NaN (n_init_throw), and for the candidates of yfm_last_batch_deferred (their value comes
 * from the double-double path, which carries no tangents): those are counted by
 * yfm_last_batch_grad_unavailable.  yfm_last_batch_flags keeps its meaning.  Synchronous. */
int yfm_loglik_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                          const int* T_use, double* loglik_out, double* grad_out);

/* Same (optimization.jl:367, :10-23) with DEVICE pointers on the caller's HIP stream; asynchronous, with
 * the ordering rules of yfm_loglik_batch_device. */
int yfm_loglik_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                                 const int* d_T_use, double* d_loglik_out, double* d_grad_out, void* hip_stream);

/* Candidates of the last gradient batch on this ctx with a finite-or-not loglik from the double-double
 * path and therefore NaN gradients (optimization.jl:367 has no counterpart: ForwardDiff differentiates
 * the dense path of optimization.jl:10-23 there).  0 after a batch that asked for no gradient.  For
 * yfm_loglik_grad_batch_device, synchronise the stream first. */
int yfm_last_batch_grad_unavailable(yfm_ctx* ctx, long long* n);

/* The TVλ log-likelihood WITH its gradient — the value and the ForwardDiff gradient that estimate! asks for
 * (optimization.jl:367) of compute_loss (optimization.jl:10-23) on the extended Kalman filter of filter.jl:12-80,
 * with the argument lists, the sign, the layout of grad_out (P×B column-major, P = 31), the spaces and the
 * ordering and synchrony rules of yfm_loglik_grad_batch(_device).  YFM_MODEL_TVL only: any other kind returns
 * YFM_EUNSUPPORTED (yfm_loglik_grad_batch still serves DNS and still refuses TVλ).  Every N that yfm_loglik_batch
 * takes for TVλ is accepted.
 *   Value: loglik_out comes from the loglik launch, enqueued first on the same stream under the context's
 * precision (yfm_set_precision; certified double-double by default): it is bitwise what yfm_loglik_batch returns,
 * and yfm_last_batch_flags keeps its meaning.
 *   Gradient: always the FP64 forward-mode tangent recursion of the function the reference computes — the Jacobian
 * column as written at filter.jl:43, t = 1 not accumulated, the last column unused, a NaN column a prediction-only
 * step whose stale F/v term and its tangent are added again — the same bits under either precision setting and
 * whatever batch the candidate sits in.  A window with T_use ≤ 2 gives loglik 0 and an exactly zero gradient.
 *   NaN rule: grad_out[:, b] is NaN in all 31 entries where (1) loglik_out[b] is −Inf or NaN; (2) the value is
 * finite but the tangent recursion's own FP64 value is not, or it meets a negative determinant; (3) any tangent is
 * non-finite (λ overflow, for example).  Cases (2) and (3) are counted by yfm_last_batch_grad_unavailable.
 * Additive: YFM_ABI_VERSION stays 5; a library that has the symbols has the feature. */
int yfm_tvl_loglik_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                              const int* T_use, double* loglik_out, double* grad_out);
int yfm_tvl_loglik_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                     int B, const int* d_T_use, double* d_loglik_out, double* d_grad_out,
                                     void* hip_stream);

/* The λ kinds' loss WITH its gradient with respect to δ and Φ — replaces, per candidate, the value and the
 * gradient that Optim.LBFGS asks for in estimate_steps! when it optimises parameter group "2", the M(M+1) = 12
 * entries of δ and vec Φ (optimization.jl:137-312, :442-479; the groups: msebasemodel.jl:153-162,
 * staticbasemodel.jl:103-112), with the sign of get_loss: loss_out[b] is bitwise what yfm_loglik_batch returns
 * (filter.jl:209-243) and grad_out[:, b] (12×B column-major: δ(3), then vec Φ column-major — the order of θ's last
 * 12 rows) = ∂(+get_loss)/∂θ_i in the space the caller passed; the unconstrained space includes the derivative
 * of from_R_to_11 on the diagonal of Φ (transformations.jl:21-26), everything else there is the identity.  The
 * gradient is exact and needs no tangent recursion: on a data column filter replaces β by an OLS fit and takes
 * the score from it (filter.jl:52-91), so δ and Φ enter only the prediction μ + Φβ (filter.jl:84-88).  A missing
 * first column makes step 1 prediction-only from β₀ = δ (filter.jl:53-59).  The derivatives with respect to the
 * leading parameters (A, B, ω; γ for NS) are not formed here (the reference's defaults optimise those by
 * Nelder–Mead): yfm_lambda_loss_fullgrad_batch below forms all P rows.
 * YFM_MODEL_NS, SD_NS, RWSD_NS, SSD_NS and SRWSD_NS only: the Kalman kinds return YFM_EUNSUPPORTED (their
 * gradient is yfm_loglik_grad_batch).  grad_out[:, b] is NaN in all 12 entries where loss_out[b] is −Inf
 * (n_neg_inf).  A candidate's 13 outputs do not depend on the batch.  yfm_last_batch_flags keeps its meaning.
 * Synchronous. */
int yfm_lambda_loss_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                               const int* T_use, double* loss_out, double* grad_out);

/* Same (optimization.jl:442-479, filter.jl:209-243) with DEVICE pointers on the caller's HIP stream;
 * asynchronous, with the ordering rules of yfm_loglik_batch_device. */
int yfm_lambda_loss_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                      int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                      void* hip_stream);

/* The λ kinds' loss WITH its gradient with respect to EVERY row of θ — the value and the gradient that estimate!'s
 * L-BFGS asks for (optimization.jl:329-410, :367) of compute_loss for these kinds, with the sign of get_loss, and what
 * an L-BFGS group of estimate_steps! that holds leading parameters needs.  The argument, ordering and synchrony rules
 * are those of yfm_lambda_loss_grad_batch(_device); grad_out is P×B column-major in the order of θ.
 *   What it is: the derivative of the function get_loss computes (filter.jl:209-243, K = 1) with respect to every
 * row of θ, in the space the caller passed — what a finite-difference L-BFGS on get_loss converges to.  It is NOT
 * the reference's own dual-number path, which cannot serve as the definition: get_grad_gamma! strips the outer tangent
 * of β (ForwardDiff.value.(beta), filter.jl:175) and set_params! writes into Float arrays.  The leading rows (A, B, ω
 * for SD-NS and SSD-NS; A, ω for RWSD-NS and SRWSD-NS; γ for NS) come from a forward tangent through the score
 * recursion: per direction the scalar γ̇ and, for the scaled kinds, the tangent of the score's second-moment average,
 * with β' = ∂β/∂γ of both OLS fits and the exact score's ∂g/∂γ (second derivatives of the loadings included).  The
 * value path is untouched — the scaled kinds still take their score at the refined β — and the tangent is the exact
 * score's.  The unconstrained space multiplies row A by A and row B by B(1 − B); a missing first column is a
 * prediction-only step, γ₁ = ν + Bγ₀ with its tangent.
 *   Bits: loss_out[b] is bitwise what yfm_loglik_batch returns, and rows P−12 … P−1 of an available gradient are
 * bitwise yfm_lambda_loss_grad_batch's.  A candidate's P + 1 outputs do not depend on the batch it sits in.  A window
 * that compares no column (T_use = 1) gives the loss yfm_loglik_batch gives and an exactly zero gradient.
 *   NaN rule: grad_out[:, b] is NaN in all P rows where (1) loss_out[b] is −Inf (n_neg_inf); (2) the loss is finite
 * but a tangent or a leading accumulator is not finite — a score that is exactly 0 on a scaled kind's first step
 * (the root of its average is 0), λ overflow.  Case (2) is counted by yfm_last_batch_grad_unavailable.
 *   YFM_MODEL_NS, SD_NS, RWSD_NS, SSD_NS and SRWSD_NS with the N range of yfm_loglik_batch for them; every other kind
 * returns YFM_EUNSUPPORTED.  yfm_loglik_grad_batch and yfm_lambda_loss_grad_batch keep their behaviour and refusals.
 * Additive: YFM_ABI_VERSION stays 5; a library that has the symbols has the feature. */
int yfm_lambda_loss_fullgrad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                                   const int* T_use, double* loss_out, double* grad_out);
int yfm_lambda_loss_fullgrad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                          int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                          void* hip_stream);

/* The same for the neural kinds (YFM_MODEL_NNS, NNS_ANCHORED and the 24 score-driven NNS kinds): their parameter
 * group "2" is the same last 12 rows of θ, and δ and Φ enter their filter through the prediction only as well, so
 * the signatures, the layout of grad_out, the spaces, the NaN gradient of a −Inf loss and the batch independence
 * are those of yfm_lambda_loss_grad_batch(_device); loss_out[b] is bitwise what yfm_loglik_batch returns for the
 * kind.  Every other kind returns YFM_EUNSUPPORTED, and so does a panel with fewer than 4 maturities or more than
 * the gradient kernel's maximum (1024, the loss kernel's).  Additive: YFM_ABI_VERSION stays 5, a library that has
 * these two symbols differs from one that has not in nothing else. */
int yfm_neural_loss_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                               const int* T_use, double* loss_out, double* grad_out);
int yfm_neural_loss_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                      int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                      void* hip_stream);

/* The neural kinds' loss WITH its gradient with respect to EVERY row of θ: yfm_lambda_loss_fullgrad_batch(_device) for
 * YFM_MODEL_NNS, NNS_ANCHORED and the 24 score-driven NNS kinds, with its arguments, ordering and synchrony rules;
 * grad_out is P×B column-major in the order of θ (P = 30 for the static kinds, 34 / 42 / 66 for the score-driven kinds
 * with a B, 32 / 36 / 48 for the random-walk kinds).
 *   What it is: the derivative of the function get_loss computes (filter.jl:209-243, K = 1) with respect to every row
 * of θ, in the space the caller passed — what a finite-difference L-BFGS on get_loss converges to.  It is NOT the
 * reference's own dual-number path, which cannot serve as the definition: get_grad_gamma! strips the outer tangent of
 * β (ForwardDiff.value.(beta), filter.jl:175) and set_params! writes into Float arrays.  The leading rows (A, B, ω;
 * A, ω for the random-walk kinds; γ for the static kinds) come from a reverse (adjoint) sweep over the score recursion,
 * whose cost does not depend on the number of rows: a forward sweep records the γ — and, for the scaled kinds, the
 * score's second-moment average — every step enters with, and a backward sweep rebuilds each step from its record
 * and applies the transposes of both OLS fits, of the update and of the score's Jacobian (a Hessian–vector product of
 * the loadings' second derivatives plus the OLS transpose of the β the score is taken at).  The value path is
 * untouched.  The unconstrained space multiplies row A by A and row B by B(1 − B); a missing first column is a
 * prediction-only step, γ₁ = ν + B∘γ₀, with no β adjoint.
 *   Bits: loss_out[b] is bitwise what yfm_loglik_batch returns, and rows P−12 … P−1 of an available gradient are
 * bitwise yfm_neural_loss_grad_batch's.  A candidate's P + 1 outputs do not depend on the batch it sits in, on the
 * lanes per candidate, or on how the launch is split into chunks: the trajectory workspace is capped at 1 GiB (the
 * environment variable YFM_NNS_TRAJ_BYTES overrides the cap in bytes, with a floor of one block's candidates) and a
 * larger batch runs as several chunks of whole blocks on the same stream.  A window that compares no column
 * (T_use = 1) gives the loss yfm_loglik_batch gives and an exactly zero gradient.
 *   NaN rule: grad_out[:, b] is NaN in all P rows where (1) loss_out[b] is −Inf (n_neg_inf); (2) the loss is finite
 * but an adjoint or an accumulator is not finite — a scaled kind's average that is exactly 0 in a component (its
 * root is 0), overflow of a hidden unit.  Case (2) is counted by yfm_last_batch_grad_unavailable.
 *   Every other kind returns YFM_EUNSUPPORTED, and so does a panel with fewer than 4 maturities or more than the two
 * sweeps' maximum, 512 (below the loss kernel's 1024: the backward sweep's LDS record takes the room).
 * yfm_lambda_loss_fullgrad_batch keeps refusing the neural kinds.  Additive: YFM_ABI_VERSION stays 5; a library that
 * has the symbols has the feature. */
int yfm_neural_loss_fullgrad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                                   const int* T_use, double* loss_out, double* grad_out);
int yfm_neural_loss_fullgrad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                          int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                          void* hip_stream);

/* Score series, information matrices and the Hessian of the DNS log-likelihood — what standard errors of a
 * maximum-likelihood estimate are made of.  AN EXTENSION: the reference has no counterpart (estimate! in
 * optimization.jl returns the optimum and its loss, no covariance), so the definitions below are this library's own.
 *   get_loss over nobs = T_use[b] columns is ll = Σ_{k=1}^{nobs−2} ℓ_k, ℓ_k the term added after column k (0-based)
 * is processed; at a NaN column it is the stale term, added again as the reference does (filter.jl:195).
 *   Score series: S[d, k, b] = ∂ℓ_k/∂θ_d for 1 ≤ k ≤ nobs_b − 2 and exactly 0.0 elsewhere; scores_out is
 * P × (T − 1) × B column-major (Julia's S[:, k, b], k 0-based here), θ in the space passed (the unconstrained space
 * through the chain factors of the transform).  Σ_k S[:, k, b] is yfm_loglik_grad_batch's gradient up to the order of
 * the sum.  loglik_out is bitwise yfm_loglik_batch's.
 *   OPG / HAC matrix: Γ_ℓ = Σ_k s_k s_{k−ℓ}' over the pairs that both lie in the accumulated range, and
 * J = Γ_0 + Σ_{ℓ=1}^{lags} (1 − ℓ/(lags+1))(Γ_ℓ + Γ_ℓ') (Bartlett weights; lags = 0: the plain outer product of
 * gradients; lags ≥ nobs − 2 is allowed, the sums are empty).  opg_out is P × P × B column-major, symmetric to the bit.
 *   Hessian: H = ∂²ll/∂θ∂θ' by fourth-order central differences of the EXACT gradient over the realised steps,
 * D_i = (8(g(θ+h e_i) − g(θ−h e_i)) − (g(θ+2h e_i) − g(θ−2h e_i)))/(12h), H = ½(D + D'): 4P perturbed candidates per
 * θ through the loglik and gradient kernels.  step ≤ 0 asks for the default h = YFM_INFO_DEFAULT_STEP.  hess_out is
 * P × P × B column-major, symmetric to the bit.
 *   Unavailable: a candidate has NaN in all of S, J and H where its loglik is −Inf or NaN or where it was evaluated
 * on the double-double path (the deferral list: κ₁(Z'Z) ≥ 1e6), and in all of H also where any of its 4P perturbed
 * points is in that state.  yfm_last_batch_grad_unavailable counts, after yfm_loglik_scores_batch(_device), the
 * deferred candidates (as after yfm_loglik_grad_batch) and, after yfm_loglik_info_batch, the candidates with NaN in H
 * (hess_out NULL: in J); the other yfm_last_batch_* counters then answer for the batch's own loglik launch.
 *   yfm_loglik_info_batch: host pointers; hess_out or opg_out may be NULL to skip that half (not both); loglik_out is
 * bitwise yfm_loglik_batch's and grad_out bitwise yfm_loglik_grad_batch's.  A candidate's outputs do not depend on
 * the batch it sits in.  Beyond the staging that yfm_loglik_grad_batch allocates for the same batch (θ, T_use, loglik,
 * gradient, the work records of the batch's loglik launch), no temporary exceeds 128 MiB: the scores, the perturbed
 * points with the work records of their launches, H and J go chunk by chunk.
 *   YFM_MODEL_DNS with N ≤ 64 only: every other kind, and a larger N, returns YFM_EUNSUPPORTED; lags < 0 and two
 * NULL outputs return YFM_EINVAL.  The _device twin takes device pointers and is asynchronous on hip_stream, with the
 * ordering rules of yfm_loglik_grad_batch_device.  Additive: YFM_ABI_VERSION stays 5; a library that has the symbols
 * has the feature. */
#define YFM_INFO_DEFAULT_STEP 1e-4
int yfm_loglik_scores_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                            const int* T_use, double* loglik_out, double* scores_out);
int yfm_loglik_scores_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                                   const int* d_T_use, double* d_loglik_out, double* d_scores_out, void* hip_stream);
int yfm_loglik_info_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                          const int* T_use, int lags, double step, double* loglik_out, double* grad_out,
                          double* hess_out, double* opg_out);

/* The same three calls for the TVλ model (P = 31): score series, OPG / HAC matrix and Hessian of the extended-Kalman-
 * filter log-likelihood that yfm_tvl_loglik_grad_batch differentiates.  AN EXTENSION, as the DNS calls above are: the
 * reference's estimate! returns no covariance.  The argument lists are those of the DNS namesakes.
 *   Score series: S[d, k, b] = ∂ℓ_k/∂θ_d for 1 ≤ k ≤ nobs_b − 2 and exactly 0.0 elsewhere (column 0, the columns from
 * nobs_b − 1 on, and every column when T_use[b] ≤ 2), ℓ_k the term get_loss adds after column k (at a NaN column the
 * stale term, added again); scores_out is 31 × (T − 1) × B column-major, θ in the space passed.  Σ_k S[:, k, b] is
 * yfm_tvl_loglik_grad_batch's gradient up to the order of the sum.  The series comes from the FP64 tangent recursion:
 * it is the same bits under either yfm_set_precision setting and in whatever batch the candidate sits.
 *   OPG / HAC matrix: J = Γ_0 + Σ_{ℓ=1}^{lags} (1 − ℓ/(lags+1))(Γ_ℓ + Γ_ℓ'), Γ_ℓ = Σ_k s_k s_{k−ℓ}' (Bartlett weights,
 * lags = 0: the plain outer product; lags ≥ nobs − 2 is allowed).  opg_out is 31 × 31 × B, symmetric to the bit.
 *   Hessian: H = ½(D + D'), D_i = (8(g(θ+h e_i) − g(θ−h e_i)) − (g(θ+2h e_i) − g(θ−2h e_i)))/(12h) over the realised
 * steps, g the exact gradient: 4P = 124 perturbed candidates per θ through the TVλ loglik launch at the context's
 * precision and the gradient kernel, the sequence of yfm_tvl_loglik_grad_batch.  step ≤ 0 asks for the default
 * h = YFM_TVL_INFO_DEFAULT_STEP.  hess_out is 31 × 31 × B, symmetric to the bit.
 *   Unavailable: the gradient's rule.  A candidate has NaN in all of S, J and H where its loglik is −Inf or NaN, where
 * the tangent recursion's own FP64 value is not finite or meets a non-positive determinant, or where an entry of its
 * gradient is not finite; and in all of H also where any of its 124 perturbed points has a NaN gradient.
 * yfm_last_batch_grad_unavailable counts, after yfm_tvl_loglik_scores_batch(_device), what it counts after
 * yfm_tvl_loglik_grad_batch and, after yfm_tvl_loglik_info_batch, the candidates with NaN in H (hess_out NULL: in J);
 * the other yfm_last_batch_* counters then answer for the batch's own loglik launch.
 *   loglik_out is bitwise yfm_loglik_batch's and grad_out bitwise yfm_tvl_loglik_grad_batch's.  Beyond the staging that
 * yfm_tvl_loglik_grad_batch allocates for the same batch, no temporary exceeds 128 MiB: the scores, the perturbed
 * points with the work records of their launches, H and J go chunk by chunk, and a candidate's outputs do not depend on
 * how the batch is cut.
 *   YFM_MODEL_TVL only, with every N the TVλ gradient accepts: every other kind returns YFM_EUNSUPPORTED (DNS has the
 * calls above); lags < 0 and two NULL outputs return YFM_EINVAL.  yfm_loglik_scores_batch and yfm_loglik_info_batch
 * keep refusing TVλ.  Additive: YFM_ABI_VERSION stays 5; a library that has the symbols has the feature. */
#define YFM_TVL_INFO_DEFAULT_STEP 1e-5
int yfm_tvl_loglik_scores_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                                const int* T_use, double* loglik_out, double* scores_out);
int yfm_tvl_loglik_scores_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                       int B, const int* d_T_use, double* d_loglik_out, double* d_scores_out,
                                       void* hip_stream);
int yfm_tvl_loglik_info_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                              const int* T_use, int lags, double step, double* loglik_out, double* grad_out,
                              double* hess_out, double* opg_out);

/* The fixed-interval Kalman smoother of the fixed-loading models — β̂_{t|n} = E[β_t | y_1 … y_n], its covariance and the
 * lag-one covariance: level, slope and curvature paths, fitted curves, residuals that are not one-step forecasts, and
 * the moments Σ V_t, Σ C_t of an EM step.  AN EXTENSION: the reference has no counterpart (its predict, filter.jl:250-282,
 * returns the forecasts a_{t+1|t} only), so the definitions below are this library's own.
 *   Model: the one the reference's fixed-loading filter! runs (filter.jl:125-179, initialize_filter filter.jl:1-10):
 * y_t = Zβ_t + ε_t with Var ε = σ²I; β_{t+1} = δ + Φβ_t + η_t with Var η = Q; a_1 = (I − Φ)⁻¹δ and P_1 the unconditional
 * covariance.  A column with any NaN entry is a missing column (the reference's rule any(isnan.(y))).
 *   Window: candidate b has n = T_use[b] columns, or T when T_use is NULL.  All n columns condition the result, column 1
 * and column n included: the exclusion of t = 1 from the log-likelihood and the unused last column of get_loss are
 * properties of the loss, not of the state estimate.  n = 1 is valid: one update, no C.
 *   Definitions: with G = Z'Z and a_t, P_t the predicted moments a_{t|t−1}, P_{t|t−1}, at a data column
 *     B_t = σ²I + G P_t,  s_t = B_t⁻¹(Z'y_t − G a_t) (= Z'F_t⁻¹v_t),  W_t = B_t⁻¹G (= Z'F_t⁻¹Z),  L_t = Φ(I − P_t W_t);
 * at a missing column s_t = 0, W_t = 0, L_t = Φ.  Backward, from r_n = 0 and N_n = 0:
 *     r_{t−1} = s_t + L_t' r_t,   N_{t−1} = W_t + L_t' N_t L_t,
 *     β̂_t = a_t + P_t r_{t−1},   V_t = P_t − P_t N_{t−1} P_t,
 *     C_t = Cov(β_{t+1}, β_t | y_1..n) = (I − P_{t+1} N_t) L_t P_t,  t = 1 … n − 1.
 *   Outputs, column-major, NaN beyond a candidate's window: beta_s M × T × B, slot t − 1 = β̂_t; V_s M × M × T × B,
 * symmetric to the bit; C_s M × M × (T − 1) × B, slot t − 1 = C_t — C_s may be NULL.
 *   Unavailable: all of a candidate's outputs are NaN where initialize_filter would throw; where its log-likelihood
 * over the window is −Inf or NaN; where it sits on the deferral list (κ₁(Z'Z) ≥ 1e6 and the like: an FP64 backward
 * sweep of those is not certified — their forward states remain available through yfm_filter_states); and where any
 * of its outputs is not finite.  yfm_last_batch_grad_unavailable counts these candidates; yfm_last_batch_flags and
 * yfm_last_batch_deferred answer for the batch's forward launch.  A candidate's outputs are bitwise independent of the
 * batch it is in and of its position in it.
 *   yfm_smooth_batch takes host pointers and is synchronous; yfm_smooth_batch_device takes device pointers and only
 * enqueues on hip_stream, with the ordering rules of yfm_loglik_batch_device.  The forward pass is the trajectory
 * launch of yfm_filter_states.  Beyond the batch's own staging (θ, T_use, the logliks, the work records of the forward
 * launch) no device temporary exceeds 128 MiB: the recorded moments go chunk by chunk over candidates, and in the
 * host-pointer call the outputs leave per chunk.  B = 0 succeeds.
 *   YFM_MODEL_DNS and YFM_MODEL_GNS5 with N ≤ 64: a larger N returns YFM_EUNSUPPORTED, and so do YFM_MODEL_TVL (its
 * extended smoother is yfm_tvl_smooth_batch), the λ kinds and the neural kinds (no Kalman filter: nothing to smooth).
 * Additive: YFM_ABI_VERSION stays 5; a library that has the symbols has the feature. */
int yfm_smooth_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                     const int* T_use, double* beta_s, double* V_s, double* C_s);
int yfm_smooth_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                            const int* d_T_use, double* d_beta_s, double* d_V_s, double* d_C_s, void* hip_stream);

/* The extended Kalman smoother of the TVλ model — β̂_{t|n}, V_t, C_t as above with M = 4, and with them the path of the
 * decay parameter given all the data, λ̂_t = 0.01 + exp(β̂_{4,t|n}).  AN EXTENSION, as the fixed-loading smoother is: the
 * reference has no counterpart (its predict, filter.jl:250-282, returns forecasts only).
 *   Model: the one the reference's TVλ filter! runs (filter.jl:12-80, update_factor_loadings! in tvλdns.jl:53-64,
 * initialize_filter filter.jl:1-10), linearised once, at the forward pass's predicted states: nothing is re-linearised
 * or iterated.  At a data column t, with a_t, P_t the predicted moments,
 *     λ_t = 0.01 + exp(a_{4,t}),   Z_t = [1, S(λ_t), C(λ_t), ż_t]  (N × 4; ż_t the Jacobian column as written at
 *     filter.jl:38-46, quirk kept),   v_t = y_t − Z_t[:,1:3]·a_t[1:3],   G_t = Z_t'Z_t,   u_t = Z_t'v_t,
 *     B_t = σ²I + G_t P_t,   s_t = B_t⁻¹u_t,   W_t = B_t⁻¹G_t,   L_t = Φ(I − P_t W_t);
 * a column with any NaN is a missing column: s_t = 0, W_t = 0, L_t = Φ.  Backwards from r_n = 0, N_n = 0 the recursion is
 * exactly that of yfm_smooth_batch:
 *     r_{t−1} = s_t + L_t' r_t,   N_{t−1} = W_t + L_t' N_t L_t,
 *     β̂_t = a_t + P_t r_{t−1},   V_t = P_t − P_t N_{t−1} P_t,   C_t = (I − P_{t+1} N_t) L_t P_t,  t = 1 … n − 1.
 * All n columns of the window condition the result; n = 1 is valid.
 *   Outputs: the layout of yfm_smooth_batch with M = 4 — beta_s 4 × T × B, V_s 4 × 4 × T × B, symmetric to the bit, C_s
 * 4 × 4 × (T − 1) × B, which may be NULL; slots past a window are NaN.
 *   Unavailable: all of a candidate's outputs are NaN, and yfm_last_batch_grad_unavailable counts it, where
 * initialize_filter would throw; where the window's log-likelihood is −Inf or NaN; where a data column's
 * det(σ²I + P_t G_t) is ≤ 0 or not finite, by the rule of yfm_tvl_loglik_grad_batch's kernel — which, like the loss,
 * lets a negative determinant pass at column 1 alone: a non-stationary Φ gives an indefinite P_1, the reference goes on
 * filtering, and the smoothed moments remain the Gaussian conditional's; and where any output inside the window is not
 * finite.  TVλ has no deferral list.
 *   The forward pass is the TVλ trajectory launch of yfm_filter_states at the context's precision (YFM_PREC_CERTIFIED:
 * double-double); the backward sweep is FP64.  Candidates go in chunks: the record (20 doubles × (T − 1) per candidate),
 * each staging buffer and the launch's own scratch stay within 128 MiB each.  The TVλ forward picks its lane count from
 * the batch size, and every chunk's launch takes the whole batch's: a candidate's outputs do not depend on its position
 * in the batch, or on the other candidates of a batch of the same size.  Across batch sizes the recorded bits may differ,
 * and only the parity rule is promised (per array and step, within 1e-9 of a dense FP64 statement of the same smoother,
 * or at least as close to the 40-digit truth as that statement is).
 *   yfm_tvl_smooth_batch takes host pointers and is synchronous; yfm_tvl_smooth_batch_device takes device pointers and
 * only enqueues on hip_stream, with the ordering rules of yfm_loglik_batch_device.  Every N the TVλ log-likelihood takes,
 * both parameter spaces, a per-candidate T_use.  B = 0 succeeds.  Any model_kind but YFM_MODEL_TVL returns
 * YFM_EUNSUPPORTED: DNS and GNS5 have yfm_smooth_batch, the λ and neural kinds are not Kalman filters and have nothing
 * to smooth.  Additive: YFM_ABI_VERSION stays 5; a library that has the symbols has the feature. */
int yfm_tvl_smooth_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                         const int* T_use, double* beta_s, double* V_s, double* C_s);
int yfm_tvl_smooth_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                                const int* d_T_use, double* d_beta_s, double* d_V_s, double* d_C_s, void* hip_stream);

/* One Optim.NelderMead run per chain on a block of coordinates — what estimate_steps! does for a parameter group
 * that uses opt1 (optimization.jl:218-247 with :442-451, :479: NelderMead, `iterations`, g_tol), without the outer
 * group loop, the sanitising or the rescaling around it (:157-184, :249-281), which stay with the caller.  p is
 * P×R column-major, UNCONSTRAINED, in/out: chain r minimises compute_loss (optimization.jl:10-23, = −get_loss) of
 * column r on the window T_use[r] (NULL: the whole panel) over the n_idx distinct coordinates idx[] (0-based rows
 * of θ), the other coordinates held at their values in p; on return those coordinates hold Optim's minimizer and
 * f_out[r] its compute_loss.  The simplex dimension is n_idx.  All model kinds.  The rounds are yfm_estimate's:
 * one batched launch per round and chain group, the speculation tree, each trial point embedded into the chain's
 * full θ in its batch slot; a chain's sequence of simplices is bitwise that of a sequential Optim run on the same
 * objective values.  Where the objective throws (NaN: a Kalman kind's initialize_filter), the chain's column
 * of p is left as it came and f_out[r] is NaN.  n_evals_out (may be NULL): evaluations the chains consumed.
 * Synchronous. */
int yfm_nm_block(yfm_ctx* ctx, int model_kind, double* p, int P, int R, const int* T_use, const int* idx, int n_idx,
                 int iterations, double g_tol, double* f_out, long long* n_evals_out);

#ifdef __cplusplus
}
#endif
#endif /* YFM_H */
