// yfm_internal.hpp — launch interface between the C ABI (yfm_capi.hip) and the kernels.
#pragma once
#include "yfm_flags.hpp"
#include "yfm_tvl_layout.hpp"  // chunk_columns, kTvlGaps, kTvlPowGaps
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/yfm.h"

namespace yfm {

// An environment switch, read at the launch it steers: the variable's text, or `dflt` (which may be null) where
// it is unset.
inline const char* env_or(const char* name, const char* dflt) {
  const char* e = std::getenv(name);
  return e ? e : dflt;
}

// A device allocation that grows on demand and frees itself.  It is destroyed with the device it was
// allocated on current (yfm_destroy sets the context's device before it deletes the context).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
};

// A lane count as a type, and f(Lanes<L>) for the L among Ls that `lanes` names (any other count is refused)
template <int LN>
struct Lanes {
  static constexpr int value = LN;
};
template <int... Ls, class F>
hipError_t with_lanes_of(int lanes, F&& f) {
  hipError_t e = hipErrorInvalidValue;
  (void)((lanes == Ls && ((e = f(Lanes<Ls>{})), true)) || ...);
  return e;
}

struct LaunchArgs {
  const double* theta;  // P×B device
  int P, B, space;
  const double* panel;  // prepared panel (T × ldp)
  const double* raw;    // caller's panel N×T column-major (device copy)
  int T, N, np, ldp;
  const double* mats;   // N device
  const int* T_use;     // B device or nullptr
  double* out;          // B device
  unsigned int* flags;  // this launch's kFlagsPerBank counters (kFlagsPerBank above)
  unsigned int* flags_next = nullptr;  // the other counter bank: zeroed by this launch's first kernel
  double* rec_beta;     // optional trajectories
  double* rec_P;
  double* scratch;      // per-candidate work records (tvl_scratch_bytes, fixedz_scratch_bytes)
  int horizon = 0;      // 0: loglik mode; ≥ 1: trajectory mode (predict / forecast / loss array)
  int rec_len = 0;      // recorded steps per candidate (the last rec_len), stride of rec_beta / rec_P
  int* defer_list = nullptr;   // fixed-loading FP64 kernels → double-double kernel hand-off (B ints)
  int* defer_count = nullptr;  // 1 int, zeroed before the FP64 kernel
  hipStream_t stream;
};

// padded maturity count NP the fixed-loading kernel is instantiated for (-1: none)
int fixedz_np_for(int N);
hipError_t launch_fixedz(int kind, const LaunchArgs& a);
// DNS with N ≤ 32: each filter split over a covariance wave and a mean wave (yfm_split.hip)
bool dns_split_supported(int np);
hipError_t launch_dns_split(const LaunchArgs& a);
// DNS at NP = 30 on 7 MFMA k-steps (both kernels above): 1 unless YFM_DNS_KTRIM=0
int ktrim_enabled();
// per-candidate initial-state records of the per-lane kernel (GNS5: fixedz_init_kernel), bytes
size_t fixedz_scratch_bytes(int kind, int B);
// fixed-loading models with N beyond the per-lane kernel (yfm_group.hip): filter per lane group
int group_max_n(int kind);
int group_lanes_for(int kind, int N);
hipError_t launch_fixedz_group(int kind, const LaunchArgs& a);
// the deferred fixed-loading candidates (ill-conditioned Z'Z) in double-double arithmetic
// (yfm_fixedz_dd.hip): per-candidate dd records of fixedz_dd_scratch_bytes(kind, B) bytes
size_t fixedz_dd_scratch_bytes(int kind, int B);
hipError_t launch_fixedz_dd(int kind, const LaunchArgs& a, double* rec);
// DNS loglik gradient (yfm_grad.hip), enqueued after the loglik launch whose counters a.flags and deferral list
// a.defer_list it reads: ∂loglik/∂θ into grad_out (P×B), NaN where ll[b] is not finite or b was deferred
// (counted in a.flags[5]).  grad_max_n: the largest N of its lane mapping.
int grad_max_n();
hipError_t launch_dns_grad(const LaunchArgs& a, const double* ll, double* grad_out);
// DNS score series, OPG matrix and Hessian pieces (yfm_score.hip).  launch_dns_scores, enqueued like launch_dns_grad
// after the loglik launch of all a.B candidates: S[d, k, b] = ∂ℓ_k/∂θ_d of candidates b0 … b0 + nb − 1 into scores
// (P × (T − 1) × nb column-major, starting at candidate b0), exact zeros outside a window's accumulated columns, NaN
// where ll[b] is not finite or b was deferred (`count`: the deferred counted into a.flags[5]).
hipError_t launch_dns_scores(const LaunchArgs& a, const double* ll, double* scores, int b0, int nb, bool count);
// J_b = Γ₀ + Σ_{ℓ ≤ lags} (1 − ℓ/(lags + 1))(Γ_ℓ + Γ_ℓ') from the scores of nb candidates (T_use, grad: theirs), P × P × nb
// with P = 20 (DNS) or 31 (TVλ); NaN where the candidate's own gradient grad[:, b] is NaN; count (may be null): raised
// by the candidates with a NaN J
hipError_t launch_opg(int P, const double* scores, int T, int nb, const int* T_use, int lags, const double* grad,
                      double* J, unsigned int* count, hipStream_t s);
// the 4P points θ ± h e_i, θ ± 2h e_i of nb candidates (pts: P × 4P nb; pts_T_use: 4P nb, untouched when T_use is
// null) and the realised steps (2P nb); then H = ½(D + D') from their gradients, NaN where one of them or the candidate's
// own gradient grad[:, b] is not finite (such candidates raise *count)
hipError_t launch_hessian_points(const double* theta, int P, int nb, const int* T_use, double h, double* pts,
                                 int* pts_T_use, double* steps, hipStream_t s);
hipError_t launch_hessian_assemble(const double* pts_grad, const double* steps, const double* grad, int P, int nb,
                                   double* H, unsigned int* count, hipStream_t s);
// The backward sweep of the fixed-interval smoother (yfm_smooth.hip; DNS and GNS5, N ≤ smooth_max_n), enqueued after
// the trajectory launch of the a.B candidates at a.theta whose record a.rec_beta / a.rec_P (stride a.rec_len = T − 1),
// counters a.flags and deferral list a.defer_list it reads: β̂ (M × T × B), V (M × M × T × B) and, C_s not null, the
// lag-one covariances (M × M × (T − 1) × B), NaN past a window and in all of a candidate whose ll[b] is not finite,
// that was deferred or that has an output that is not finite (those counted in a.flags[5]).  skip: a.B bytes of work.
int smooth_max_n();
hipError_t launch_smooth(int kind, const LaunchArgs& a, const double* ll, unsigned char* skip, double* beta_s,
                         double* V_s, double* C_s);
// The backward sweep of the TVλ extended smoother (yfm_tvl_smooth.hip; every N the TVλ filter takes), enqueued after
// the TVλ trajectory launch of the a.B candidates at a.theta whose record a.rec_beta / a.rec_P (stride a.rec_len ≥
// T − 1) and counters a.flags it reads: β̂ (4 × T × B), V (4 × 4 × T × B) and, C_s not null, the lag-one covariances
// (4 × 4 × (T − 1) × B), NaN past a window and in all of a candidate whose ll[b] is not finite, whose initial state is
// singular, that has a data column with det(σ²I + P_tG_t) ≤ 0 or an output that is not finite (counted in a.flags[5]).
int tvl_smooth_max_n();
hipError_t launch_tvl_smooth(const LaunchArgs& a, const double* ll, double* beta_s, double* V_s, double* C_s);
// TVλ loglik gradient (yfm_tvl_grad.hip), enqueued after the loglik launch whose counter bank a.flags it adds to:
// ∂loglik/∂θ into grad_out (31×B) from the FP64 tangent recursion over a.raw (NaN flags from a.panel), NaN where
// ll[b] is not finite or the recursion's own value or tangents are not usable (those counted in a.flags[5]).
int tvl_grad_max_n();
hipError_t launch_tvl_grad(const LaunchArgs& a, const double* ll, double* grad_out);
// TVλ score series (yfm_tvl_score.hip), enqueued like launch_tvl_grad after the loglik launch of all a.B candidates:
// S[d, k, b] = ∂ℓ_k/∂θ_d of candidates b0 … b0 + nb − 1 into scores (31 × (T − 1) × nb column-major, starting at
// candidate b0), exact zeros outside a window's accumulated columns, NaN in all of a candidate that launch_tvl_grad
// gives a NaN gradient (those with a finite ll[b] counted in a.flags[5])
hipError_t launch_tvl_scores(const LaunchArgs& a, const double* ll, double* scores, int b0, int nb);
// TVλ EKF kernel (yfm_tvl.hip): lanes per filter for a batch, largest N, launcher.  `share`: launches of this
// size the caller runs concurrently on the device (the estimation driver's chain groups; 1 otherwise)
int tvl_lanes_for(int B, int N, int share = 1);
int tvl_max_n();
size_t tvl_scratch_bytes(int B);
// Maturity jump table for the TVλ exp recurrence (built on the host per lane count L):
// the distinct values d_k of m_{i+L} − m_i and, per maturity i, the index k of its jump.
// K = 0 disables the recurrence (one exp per maturity).
// Power mode (the certified kernel, when the jumps are too many or inexact): every maturity is an exact integer
// multiple k_i·Δ of one step Δ (integer-month grids), so e^{−λm_i} = b^{k_i} with b = e^{−λΔ} — one dd exp per
// step and integer powers of b for the lane starts and the Kp ≤ kTvlPowGaps distinct jump exponents e_q.
struct TvlGaps {
  int K = 0;
  bool exact = false;         // every jump is the exact difference of its two maturities
  const double* d = nullptr;  // device, kTvlGaps
  const int* idx = nullptr;   // device, N
  int Kp = 0;                 // power mode: distinct jump exponents (0: not available)
  double step = 0.0;          // Δ
  const double* e = nullptr;  // device, kTvlPowGaps: the exponents e_q (integers, as doubles)
  const int* pidx = nullptr;  // device, N: each maturity's jump index q
};
hipError_t launch_tvl(const LaunchArgs& a, const TvlGaps& g, int lanes);
// per-candidate FP64 record of the TVλ init kernel (decoded θ + initial state), doubles
constexpr int kRecSigma = 0, kRecDelta = 1, kRecPhi = 5, kRecQ = 21, kRecBeta = 31, kRecP = 35, kRecOk = 45;
constexpr int kRecLen = 48;  // padded to 16-byte multiples
// the same filter in double-double arithmetic (yfm_tvl_dd.hip), YFM_PREC_CERTIFIED: the init
// kernel writes the per-candidate dd records into `rec_dd` (tvl_dd_scratch_bytes(B)); the panel's dd column
// statistics (tvl_dd_colsum_bytes(T)) are made once per panel (yfm_set_panel) or, for a panel of its own
// (get_loss_array's tiled one), by the launch into its scratch (colsum_out).
// tvl_dd_lanes_for picks the lanes per filter (`want` > 0: a requested width, clamped; `share` as tvl_lanes_for)
size_t tvl_dd_scratch_bytes(int B);
size_t tvl_dd_colsum_bytes(int T);
int tvl_dd_lanes_for(int B, int N, int want, int share = 1);
hipError_t launch_tvl_dd_colsum(const double* Y, int N, int T, double* colsum, hipStream_t s);
hipError_t launch_tvl_dd_init(const LaunchArgs& a, double* rec_dd);
hipError_t launch_tvl_dd(const LaunchArgs& a, const double* rec_dd, const double* colsum, const TvlGaps& g, int lanes);
// Static and score-driven λ models (yfm_msed.hip: NS, SD-NS, RWSD-NS, SSD-NS, SRWSD-NS; src/models/filter.jl:52-110).
// msed_kind: the kind is one of them; msed_param_count: P (−1 for another kind); msed_lanes_for: lanes per
// candidate for a batch (4 or 16 — a candidate's value does not depend on it).  launch_msed writes get_loss
// (filter.jl:209-243) into a.out and counts the −Inf candidates in a.flags[1]; it zeroes a.flags_next.
bool msed_kind(int kind);
int msed_param_count(int kind);
int msed_max_n();
int msed_lanes_for(int B);
hipError_t launch_msed(int kind, const LaunchArgs& a, int lanes);
// get_loss into a.out and ∂(get_loss)/∂(δ, vec Φ) — 12 per candidate, in the space a.space — into grad (12×B);
// the loss is launch_msed's bit for bit, the gradient of a −Inf candidate is NaN (counted in a.flags[1] as there).
// With filter.jl:52-91 the γ path does not depend on δ or Φ, so no tangent recursion runs (yfm_msed.hpp).
constexpr int kMsedGrad = 12;
hipError_t launch_msed_grad(int kind, const LaunchArgs& a, int lanes, double* grad);
// The loss with all P derivatives (λ kinds only; grad: P×B column-major device doubles): the loss is launch_msed's and
// the last 12 rows are launch_msed_grad's bit for bit; the leading rows (A, B, ω; γ for NS) come from the tangent of
// the score recursion (yfm_msed.hpp).  NaN in all P rows where the loss is −Inf (a.flags[1]) and where a tangent is
// not finite (a.flags[5]).
hipError_t launch_msed_fullgrad(int kind, const LaunchArgs& a, int lanes, double* grad);
// The same recursion writing its trajectory straight into the caller's (NaN-prefilled) device outputs:
// mode 1 predict (filter.jl:284-306), 2 forecast blocks (forecasting.jl:236-250), 3 get_loss_array (filter.jl:245-281).
struct MsedRecord {
  int mode = 0;
  int horizon = 1;            // predict / forecast
  int ncol = 0;               // predict: T + horizon − 1 columns per candidate; loss array: T − 1
  double* preds = nullptr;    // predict: N×ncol×B; forecast: (3 + 1 + N)×h×B; loss array: ncol×B
  double* factors = nullptr;  // predict: 3×ncol×B
  double* states = nullptr;   // predict: 1×ncol×B
  double* load1 = nullptr;    // predict: N×ncol×B or nullptr
  double* load2 = nullptr;
};
hipError_t launch_msed_record(int kind, const LaunchArgs& a, int lanes, const MsedRecord& r);
// Neural Nelson–Siegel models (yfm_msedn.hip: NNS, NNS-Anchored and the score-driven NNS kinds; the same filter with
// γ ∈ ℝ¹⁸ and the loadings of two tanh networks).  msed_kind and msed_param_count answer for them too, so every
// caller of the λ launchers reaches them: launch_msed and launch_msed_record forward here (r == nullptr: the loss;
// MsedRecord's states are 18×ncol×B and a forecast block has 3 + 18 + N rows).  msedn_min_n ≤ N ≤ msedn_max_n.
bool msedn_kind(int kind);
int msedn_param_count(int kind);
int msedn_min_n();
int msedn_max_n();
hipError_t launch_msedn(int kind, const LaunchArgs& a, int lanes, const MsedRecord* r);
// launch_msed_grad for these kinds (it forwards here): the loss is launch_msedn's bit for bit.
// msedn_min_n ≤ N ≤ msedn_grad_max_n.
int msedn_grad_max_n();
hipError_t launch_msedn_grad(int kind, const LaunchArgs& a, int lanes, double* grad);
// The loss with all P derivatives for these kinds (yfm_msedn_adj.hip; grad: P×B column-major device doubles): a forward
// sweep that is launch_msedn_grad's loop — the loss and the last 12 rows are its bits — and records the γ (and e) every
// step enters with into traj, then an adjoint sweep backwards over those records for the leading rows (A, B, ω; γ for
// the static kinds).  NaN in all P rows where the loss is −Inf (a.flags[1]) and where an adjoint is not finite
// (a.flags[5]).  traj: msedn_fullgrad_traj_bytes(kind, B, T, lanes) bytes (0 for the static kinds: nullptr) — the
// records of one chunk of whole blocks, at most 1 GiB (YFM_NNS_TRAJ_BYTES overrides the cap, floor one block); a
// larger batch runs as several chunks on a.stream.  msedn_min_n ≤ N ≤ msedn_fullgrad_max_n.
int msedn_fullgrad_max_n();
size_t msedn_fullgrad_traj_bytes(int kind, int B, int T, int lanes);
hipError_t launch_msedn_fullgrad(int kind, const LaunchArgs& a, int lanes, double* grad, double* traj);
// Trajectory outputs (yfm_predict.hip) from a recorded state trajectory.
struct PredictArgs {
  int kind, M, L, N, P, B, T;
  int ncol;                  // predict: output columns per candidate (T + horizon − 1)
  int horizon;
  const double* theta;       // P×B device
  const double* mats;        // N device
  const int* T_use;          // B device or nullptr
  const double* rec;         // M × rec_len × B trajectory (yfm_kernels.hip / yfm_tvl.hip)
  int rec_len;
  const unsigned char* init_bad;  // B: initialize_filter threw
  double* preds;             // predict: N×ncol×B; forecast: (M+L+N)×h×B; loss array: (T−1)×B
  double* factors;           // predict: M×ncol×B
  double* states;            // predict: L×ncol×B
  double* load1;             // predict: N×ncol×B or nullptr
  double* load2;
  hipStream_t stream;
};
hipError_t launch_init_bad(const double* ll, int B, unsigned char* bad, hipStream_t s);
hipError_t launch_predict_emit(const PredictArgs& a);
hipError_t launch_forecast_emit(const PredictArgs& a);
hipError_t launch_loss_array(const PredictArgs& a, const double* Y, int T1, int passes, unsigned int* flags);
// Extra per-launch work buffers (flags, deferral list, init records) so launches can be in flight
// on several streams of one context at once (yfm_capi.hip; used by the estimation driver).  A null
// workspace is the context's own.  `share`: launches of similar size the caller keeps in flight at once
// (the TVλ lane choice sizes the device's share of this launch by it): the estimation driver passes its
// chain-group count, every other caller 1.
struct Workspace;
Workspace* workspace_create();
void workspace_destroy(Workspace* w);
int loglik_device_ws(yfm_ctx* ctx, Workspace* ws, int kind, int space, const double* d_theta, int P, int B,
                     const int* d_T_use, double* d_out, hipStream_t s, int share);
// record `msg` as yfm_last_error() for this thread and return `code` (host helpers above the C ABI)
int api_error(int code, const char* msg);
// columns of the context's panel (0 before yfm_set_panel)
int panel_T(const yfm_ctx* ctx);
// a synchronous entry point about to use the context after an asynchronous launch on a caller's stream:
// wait for the device (the caller's stream may be gone, so it is never waited on by handle)
hipError_t settle_foreign_launch(yfm_ctx* ctx);
hipError_t launch_prep_panel(const double* Y, int N, int T, int np, int ldp, double* out, hipStream_t s);

}  // namespace yfm
