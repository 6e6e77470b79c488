// yfm_capi.hip — the C ABI of libyfm_hip.so (declared in include/yfm.h).
//
// Owns device memory per context (the panel, staging buffers for the host-pointer
// entry points, the flag counters) and launches the kernels of yfm_kernels.hip.
// No torch types, no CPU compute fallback: every result comes from a HIP kernel,
// and a missing/failed device is reported as an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/yfm.h"
#include "yfm_internal.hpp"

namespace {

thread_local std::string g_last_error;

int set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define YFM_HIP_CHECK(expr)                                                                      \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) return set_error(YFM_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

int state_dim(int kind) {
  if (yfm::msed_kind(kind)) return 3;  // the λ models' β (msebasemodel.jl:64, staticbasemodel.jl:40)
  return kind == YFM_MODEL_DNS ? 3 : kind == YFM_MODEL_TVL ? 4 : kind == YFM_MODEL_GNS5 ? 5 : -1;
}
int n_lead(int kind) { return kind == YFM_MODEL_DNS ? 1 : kind == YFM_MODEL_TVL ? 0 : 2; }
// L = length of base.gamma (kalmanbasemodel.jl:58): DNS 1 (dns.jl:18), TVλ 1 (tvλdns.jl:19, never set), GNS5 2,
// the λ models 1 (mselambda.jl:29, staticlambda.jl:20)
// the neural kinds 18 (mseneural.jl:29-30)
int gamma_dim(int kind) {
  if (yfm::msedn_kind(kind)) return 18;
  return kind == YFM_MODEL_GNS5 ? 2 : (state_dim(kind) < 0 ? -1 : 1);
}
int param_count(int kind) {
  if (yfm::msed_kind(kind)) return yfm::msed_param_count(kind);
  const int M = state_dim(kind);
  if (M < 0) return -1;
  return n_lead(kind) + 1 + M * (M + 1) / 2 + M + M * M;
}

using yfm::DevBuf;

}  // namespace

// Per-launch device work buffers.  A context owns one; the estimation driver adds one per extra
// concurrent stream (launches in flight on different streams must not share them).
struct yfm::Workspace {
  DevBuf flags;       // 2 banks × kFlagsPerBank unsigned int: n_init_throw, n_neg_inf, deferral list length, n_deferred, steady wave-steps, n_grad_unavailable
  int bank = 0;       // the bank of the last launch (the other one is zeroed by that launch's first kernel)
  bool bank_dirty = false;        // the last launch failed: its zeroing of the other bank may not have been enqueued
  hipStream_t last_stream = nullptr;  // the stream of the last launch (compared, never used: it may be gone)
  DevBuf scratch;     // per-candidate work records (TVλ / GNS5 / two-wave DNS init)
  DevBuf scratch_dd;  // TVλ double-double records (YFM_PREC_CERTIFIED)
  DevBuf defer;       // candidates handed from the FP64 fixed-loading kernels to the dd kernel
  DevBuf scratch_fd;  // their double-double records (yfm_fixedz_dd.hip)
  DevBuf grad;        // gradient staging of the host-pointer gradient calls (yfm_loglik_grad_batch, yfm_lambda_loss_grad_batch)
  DevBuf nns_traj;    // the neural full gradient's trajectory: the forward sweep's records of one chunk of candidates
  // yfm_loglik_scores_batch / yfm_loglik_info_batch: one chunk of candidates at a time, each buffer ≤ kInfoChunkBytes
  DevBuf info_scores;  // the score series of a chunk
  DevBuf info_pts, info_pgrad, info_pmisc;  // a chunk's 4P perturbed θ, their gradients, their logliks / steps / T_use
  DevBuf info_out;     // H or J of a chunk (P × P per candidate), copied out before the next chunk
  DevBuf info_flags;   // the batch's own counter bank kept over the perturbed launches, and the unavailable count
  // yfm_smooth_batch(_device): one chunk of candidates at a time, the record and each output buffer ≤ kInfoChunkBytes
  DevBuf smooth_rec_beta, smooth_rec_P;    // the forward launch's record of a chunk (a_{t+1|t}, P_{t+1|t})
  DevBuf smooth_skip;                      // a chunk's deferred marks
  DevBuf smooth_ll;                        // the device-pointer call's logliks (the host-pointer call uses ctx->out)
  DevBuf smooth_beta, smooth_V, smooth_C;  // the host-pointer call's outputs of a chunk, copied out before the next
  // allocate and zero the two counter banks
  hipError_t init() {
    const size_t nb = 2 * yfm::kFlagsPerBank * sizeof(unsigned int);
    const hipError_t e = flags.ensure(nb);
    return e == hipSuccess ? hipMemset(flags.p, 0, nb) : e;
  }
  unsigned int* bank_ptr(int b) const { return static_cast<unsigned int*>(flags.p) + yfm::kFlagsPerBank * b; }
};

struct yfm_ctx {
  int device = 0;
  int precision = YFM_PREC_CERTIFIED;  // TVλ arithmetic (yfm_set_precision)
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;  // θ uploads of pipelined host-pointer batches (created lazily)
  // panel
  int N = 0, T = 0, np = 0, ldp = 0;
  DevBuf panel, mats, raw;
  DevBuf colsum;  // the panel's dd column statistics (certified TVλ), made by yfm_set_panel
  // staging for host-pointer calls
  DevBuf theta, out, tuse, rec_beta, rec_P;
  yfm::Workspace own;          // the work buffers of every launch that brings no workspace of its own
  DevBuf traj, init_bad;       // trajectory-mode state records, per-candidate init-throw marks
  DevBuf tiled_raw, tiled_panel;  // get_loss_array with K > 1 passes: the panel tiled K times
  // TVλ maturity tables, one per lane count L = 2^l (built lazily, reset by set_panel)
  std::vector<double> mats_host;
  double pow_step = 0.0;  // Δ (0: the maturities are not integer multiples of one step)
  struct TvlTab {
    int K = -1;          // jump table (TvlGaps::K; −1: not built yet)
    bool exact = false;
    DevBuf buf;
    int Kp = 0;          // power-mode table (TvlGaps::Kp), built with the jump table
    DevBuf pow;
  } tvl_tab[7];
};

namespace {

// host-pointer pipelining (yfm_loglik_batch): chunk ≥ 2 per-lane waves per SIMD, ≤ 8 chunks
constexpr int kPipeChunk = 131072;
constexpr int kPipeMaxChunks = 8;

int check_ctx(yfm_ctx* ctx) {
  if (!ctx) return set_error(YFM_EINVAL, "null context");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return set_error(YFM_EHIP, "hipSetDevice(%d): %s", ctx->device, hipGetErrorString(e));
  return YFM_OK;
}

int check_batch(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (state_dim(kind) < 0) return set_error(YFM_EINVAL, "unknown model_kind %d", kind);
  if (space != YFM_THETA_UNCONSTRAINED && space != YFM_THETA_CONSTRAINED)
    return set_error(YFM_EINVAL, "unknown param_space %d", space);
  if (P != param_count(kind))
    return set_error(YFM_EINVAL, "P = %d but model_kind %d has %d parameters", P, kind, param_count(kind));
  if (B < 0) return set_error(YFM_EINVAL, "B = %d < 0", B);
  if (ctx->T <= 0) return set_error(YFM_ENOPANEL, "no panel: call yfm_set_panel first");
  if (yfm::msedn_kind(kind)) {
    if (ctx->N < yfm::msedn_min_n())
      return set_error(YFM_EUNSUPPORTED, "N = %d maturities: the neural kinds' transforms need N >= %d (below it their "
                       "anchor slots alias)", ctx->N, yfm::msedn_min_n());
    if (ctx->N > yfm::msedn_max_n())
      return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the neural-model kernel's %d", ctx->N,
                       yfm::msedn_max_n());
    return YFM_OK;
  }
  if (yfm::msed_kind(kind)) {
    if (ctx->N > yfm::msed_max_n())
      return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the λ-model kernel's %d", ctx->N, yfm::msed_max_n());
    return YFM_OK;
  }
  if (kind == YFM_MODEL_TVL) {
    if (ctx->N > yfm::tvl_max_n())
      return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the TVλ kernel's %d", ctx->N, yfm::tvl_max_n());
    return YFM_OK;
  }
  if (yfm::fixedz_np_for(ctx->N) < 0 && ctx->N > yfm::group_max_n(kind))
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the fixed-loading kernels' %d", ctx->N,
                     yfm::group_max_n(kind));
  return YFM_OK;
}

// Index of v among the distinct values seen so far (exact equality); a new value is appended, and −1
// says that it would be one more than `max`.
int distinct_index(std::vector<double>& seen, double v, int max) {
  int k = 0;
  while (k < (int)seen.size() && seen[k] != v) ++k;
  if (k < (int)seen.size()) return k;
  if (k == max) return -1;
  seen.push_back(v);
  return k;
}

// A maturity table on the device: `slots` doubles (the distinct values, zero-padded), then one index per maturity.
int upload_table(DevBuf& buf, std::vector<double>& vals, int slots, const std::vector<int>& idx) {
  vals.resize(slots, 0.0);
  const size_t vb = sizeof(double) * slots, ib = sizeof(int) * idx.size();
  YFM_HIP_CHECK(buf.ensure(vb + ib));
  char* base = static_cast<char*>(buf.p);
  YFM_HIP_CHECK(hipMemcpy(base, vals.data(), vb, hipMemcpyHostToDevice));
  YFM_HIP_CHECK(hipMemcpy(base + vb, idx.data(), ib, hipMemcpyHostToDevice));
  return YFM_OK;
}

// Jump table of the TVλ exp recurrence for lane count L: distinct m_{i+L} − m_i (exact
// equality) and each maturity's index; K = 0 when there are more than yfm::kTvlGaps.
int build_jump_table(const std::vector<double>& m, int L, yfm_ctx::TvlTab& t) {
  const int N = (int)m.size();
  std::vector<double> d;
  std::vector<int> idx(N, 0);
  bool ok = true, exact = true;
  for (int i = 0; i + L < N && ok; ++i) {
    const double hi = m[i + L], lo = m[i];
    const double gap = hi - lo;
    // TwoSum error of the subtraction: the double-double filter needs the jumps exactly
    const double bb = gap - hi;
    exact = exact && ((hi - (gap - bb)) + (-lo - bb)) == 0.0;
    idx[i] = distinct_index(d, gap, yfm::kTvlGaps);
    ok = idx[i] >= 0;
  }
  if (ok && d.empty()) d.push_back(0.0);  // N ≤ L: every lane has at most one maturity
  const int K = ok ? (int)d.size() : 0;
  if (K > 0)
    if (int r = upload_table(t.buf, d, yfm::kTvlGaps, idx)) return r;
  t.exact = exact;
  t.K = K;
  return YFM_OK;
}

// Δ of the power mode: the gcd of the maturities when each is an integer (exactly, as a double: integer-valued
// and < 2^31), 0 otherwise.
double maturity_step(const std::vector<double>& m) {
  long long gcd = 0;
  for (const double v : m) {
    if (!(v > 0.0 && v < 2147483648.0 && v == std::floor(v))) return 0.0;
    long long a = (long long)v, b = gcd;
    while (b) {
      const long long t = a % b;
      a = b;
      b = t;
    }
    gcd = a;
  }
  return (double)gcd;
}

// Power-mode table for lane count L: the distinct jump exponents (m_{i+L} − m_i)/Δ and each maturity's index;
// Kp = 0 when Δ = 0, an exponent is outside [1, 512) or there are more than yfm::kTvlPowGaps.
int build_pow_table(const std::vector<double>& m, double step, int L, yfm_ctx::TvlTab& t) {
  const int N = (int)m.size();
  t.Kp = 0;
  if (step == 0.0 || N <= L) return YFM_OK;
  std::vector<double> e;
  std::vector<int> pidx(N, 0);
  for (int i = 0; i + L < N; ++i) {
    const double q = (m[i + L] - m[i]) / step;  // exact: integers < 2^31
    if (!(q >= 1.0 && q < 512.0)) return YFM_OK;
    pidx[i] = distinct_index(e, q, yfm::kTvlPowGaps);
    if (pidx[i] < 0) return YFM_OK;
  }
  const int Kp = (int)e.size();
  if (int r = upload_table(t.pow, e, yfm::kTvlPowGaps, pidx)) return r;
  t.Kp = Kp;
  return YFM_OK;
}

// The context's tables for lane count L, built on first use after yfm_set_panel.
int tvl_gaps(yfm_ctx* ctx, int L, yfm::TvlGaps& g) {
  int l = 0;
  while ((1 << l) < L) ++l;
  yfm_ctx::TvlTab& t = ctx->tvl_tab[l];
  if (t.K < 0) {
    if (int r = build_jump_table(ctx->mats_host, L, t)) return r;
    ctx->pow_step = maturity_step(ctx->mats_host);
    if (int r = build_pow_table(ctx->mats_host, ctx->pow_step, L, t)) return r;
  }
  g.K = t.K;
  g.exact = t.exact;
  if (g.K > 0) {
    g.d = static_cast<const double*>(t.buf.p);
    g.idx = reinterpret_cast<const int*>(g.d + yfm::kTvlGaps);
  }
  g.Kp = t.Kp;
  if (g.Kp > 0) {
    g.step = ctx->pow_step;
    g.e = static_cast<const double*>(t.pow.p);
    g.pidx = reinterpret_cast<const int*>(g.e + yfm::kTvlPowGaps);
  }
  if (std::atoi(yfm::env_or("YFM_TVL_EXP", "0")) == 1) g.K = g.Kp = 0;  // diagnostic: force one exp per maturity
  return YFM_OK;
}

// A panel other than the context's (get_loss_array's K-times tiled panel).
struct PanelView {
  const double* raw;
  const double* panel;
  int T;
};

// One filter launch.  A call site sets the fields it means; the rest keep these defaults.
struct Launch {
  int kind = 0, space = 0;
  const double* theta = nullptr;  // P×B device
  int P = 0, B = 0;
  const int* T_use = nullptr;     // B device or nullptr
  double* out = nullptr;          // B device
  double* rec_beta = nullptr;     // optional trajectories
  double* rec_P = nullptr;
  hipStream_t stream = nullptr;
  int horizon = 0;                // as LaunchArgs::horizon
  int rec_len = 0;                // recorded steps per candidate (0 with rec_beta: T − 1)
  const PanelView* panel = nullptr;  // nullptr: the context's panel
  bool continues = false;  // a later chunk of a pipelined batch: accumulates into the previous chunk's counters
  int share = 1;           // launches of this size the caller keeps in flight at once (yfm::loglik_device_ws)
  int lanes_B = 0;         // TVλ: the batch size its lane count is chosen from (0: this launch's B; a chunk of a
                           // larger batch sets the whole batch's, so a candidate's bits do not depend on its chunk)
  const yfm::MsedRecord* msed_rec = nullptr;  // λ models: the trajectory outputs this launch writes (nullptr: the loss)
  double* msed_grad = nullptr;  // λ and neural models: 12×B device, ∂loss/∂(δ, Φ) written with the loss
  double* msed_fullgrad = nullptr;  // λ and neural models: P×B device, ∂loss/∂θ written with the loss
};

// The plain log-likelihood launch, in the argument order of yfm_loglik_batch_device.
Launch loglik_launch(int kind, int space, const double* d_theta, int P, int B, const int* d_T_use, double* d_out,
                     hipStream_t s) {
  Launch q;
  q.kind = kind;
  q.space = space;
  q.theta = d_theta;
  q.P = P;
  q.B = B;
  q.T_use = d_T_use;
  q.out = d_out;
  q.stream = s;
  return q;
}

// What every kernel of the launch q reads of q and of the context: θ, the windows, the panel and the stream.  The
// outputs, counters and work buffers are the caller's to add.
yfm::LaunchArgs base_args(const yfm_ctx* ctx, const Launch& q) {
  yfm::LaunchArgs a{};
  a.theta = q.theta;
  a.P = q.P;
  a.B = q.B;
  a.space = q.space;
  a.panel = static_cast<const double*>(ctx->panel.p);
  a.raw = static_cast<const double*>(ctx->raw.p);
  a.T = ctx->T;
  a.N = ctx->N;
  a.np = ctx->np;
  a.ldp = ctx->ldp;
  a.mats = static_cast<const double*>(ctx->mats.p);
  a.T_use = q.T_use;
  a.stream = q.stream;
  return a;
}

// Enqueue the kernels of one launch on q.stream, with the work buffers of w.
int enqueue(yfm_ctx* ctx, const Launch& q, yfm::Workspace& w) {
  const int B = q.B;
  const hipStream_t s = q.stream;
  const int bank = w.bank ^ (q.continues ? 0 : 1);  // the bank this launch uses
  unsigned int* flags_next = nullptr;
  if (!q.continues) {
    flags_next = w.bank_ptr(bank ^ 1);
  } else {
    YFM_HIP_CHECK(hipMemsetAsync(w.bank_ptr(bank) + 2, 0, sizeof(unsigned int), s));
  }
  if (B == 0) {  // no kernel runs: zero both banks here
    YFM_HIP_CHECK(hipMemsetAsync(w.flags.p, 0, 2 * yfm::kFlagsPerBank * sizeof(unsigned int), s));
    return YFM_OK;
  }
  yfm::LaunchArgs a = base_args(ctx, q);
  a.out = q.out;
  a.flags = w.bank_ptr(bank);
  a.flags_next = flags_next;
  a.rec_beta = q.rec_beta;
  a.rec_P = q.rec_P;
  a.horizon = q.horizon;
  a.rec_len = q.rec_beta ? (q.rec_len > 0 ? q.rec_len : ctx->T - 1) : 0;
  if (q.panel) {
    a.raw = q.panel->raw;
    a.panel = q.panel->panel;
    a.T = q.panel->T;
  }
  hipError_t e;
  if (yfm::msed_kind(q.kind)) {
    const int lanes = yfm::msed_lanes_for(B);
    double* nns_traj = nullptr;
    if (q.msed_fullgrad && yfm::msedn_kind(q.kind)) {
      if (const size_t tb = yfm::msedn_fullgrad_traj_bytes(q.kind, B, a.T, lanes)) {
        YFM_HIP_CHECK(w.nns_traj.ensure(tb));
        nns_traj = static_cast<double*>(w.nns_traj.p);
      }
    }
    e = q.msed_fullgrad && yfm::msedn_kind(q.kind)
            ? yfm::launch_msedn_fullgrad(q.kind, a, lanes, q.msed_fullgrad, nns_traj)
        : q.msed_fullgrad ? yfm::launch_msed_fullgrad(q.kind, a, lanes, q.msed_fullgrad)
        : q.msed_grad  ? yfm::launch_msed_grad(q.kind, a, lanes, q.msed_grad)
        : q.msed_rec ? yfm::launch_msed_record(q.kind, a, lanes, *q.msed_rec)
                     : yfm::launch_msed(q.kind, a, lanes);
  } else if (q.kind == YFM_MODEL_TVL) {
    const int Bl = q.lanes_B > 0 ? q.lanes_B : B;
    int lanes = yfm::tvl_lanes_for(Bl, ctx->N, q.share);
    const char* const ov = yfm::env_or("YFM_TVL_LANES", nullptr);  // tuning override: 1, 2, 4, …, 64
    if (ov) {
      const int l = std::atoi(ov);
      if (l >= 1 && l <= 64 && (l & (l - 1)) == 0) lanes = l;
    }
    yfm::TvlGaps g;
    if (ctx->precision == YFM_PREC_CERTIFIED) {
      lanes = yfm::tvl_dd_lanes_for(Bl, ctx->N, ov ? lanes : 0, q.share);
      // the context's panel has its column statistics already; a panel of the launch's own gets them here
      const bool own_panel = q.panel && q.panel->raw != static_cast<const double*>(ctx->raw.p);
      const size_t rec_bytes = yfm::tvl_dd_scratch_bytes(B);
      YFM_HIP_CHECK(w.scratch_dd.ensure(rec_bytes + (own_panel ? yfm::tvl_dd_colsum_bytes(a.T) : 0)));
      double* rdd = static_cast<double*>(w.scratch_dd.p);
      const double* colsum = static_cast<const double*>(ctx->colsum.p);
      if (own_panel) {
        double* cs = rdd + rec_bytes / sizeof(double);
        YFM_HIP_CHECK(yfm::launch_tvl_dd_colsum(a.raw, a.N, a.T, cs, s));
        colsum = cs;
      }
      if (int r = tvl_gaps(ctx, lanes, g)) return r;
      e = yfm::launch_tvl_dd_init(a, rdd);
      if (e == hipSuccess) e = yfm::launch_tvl_dd(a, rdd, colsum, g, lanes);
    } else {
      YFM_HIP_CHECK(w.scratch.ensure(yfm::tvl_scratch_bytes(B)));
      a.scratch = static_cast<double*>(w.scratch.p);
      if (int r = tvl_gaps(ctx, lanes, g)) return r;
      e = yfm::launch_tvl(a, g, lanes);
    }
  } else {
    // N ≤ 64: one filter per lane (MFMA Z'y); larger N: one filter per lane group.  Either defers
    // the candidates with an ill-conditioned Z'Z, which the double-double kernel then evaluates
    YFM_HIP_CHECK(w.defer.ensure(sizeof(int) * (size_t)B));
    YFM_HIP_CHECK(w.scratch_fd.ensure(yfm::fixedz_dd_scratch_bytes(q.kind, B)));
    a.defer_count = reinterpret_cast<int*>(a.flags + 2);  // zero (a fresh bank, or reset above)
    a.defer_list = static_cast<int*>(w.defer.p);
    if (yfm::fixedz_np_for(ctx->N) > 0) {
      if (const size_t sb = yfm::fixedz_scratch_bytes(q.kind, B)) {
        YFM_HIP_CHECK(w.scratch.ensure(sb));
        a.scratch = static_cast<double*>(w.scratch.p);
      }
      e = yfm::launch_fixedz(q.kind, a);
    } else {
      e = yfm::launch_fixedz_group(q.kind, a);
    }
    if (e == hipSuccess) e = yfm::launch_fixedz_dd(q.kind, a, static_cast<double*>(w.scratch_fd.p));
  }
  if (e != hipSuccess) return set_error(YFM_EHIP, "kernel launch: %s", hipGetErrorString(e));
  return YFM_OK;
}

// Counters [n_init_throw, n_neg_inf, defer_count, n_deferred, steady] in two banks: a launch uses the bank
// its predecessor zeroed (its first kernel zeroes the other one), so no memset is enqueued per call.
// That hand-off only holds when the predecessor's kernels were all enqueued (bank_dirty otherwise) and ran
// on the same stream; after a failed launch or on a stream change this launch zeroes its bank itself, on
// its own stream.  Launches on different streams are ordered by the caller (include/yfm.h: a context's
// scratch serves one launch at a time), so no event is recorded per launch — one was, in an earlier
// round-4 build, and cost 4.7 µs of every config-2 call (profiles/r4/exp1/) — and the library never
// touches the previous launch's stream (the estimator destroys its group streams).  The bank index flips
// only once the launch succeeded.  A pipelined chunk continues its batch's counters and only resets the
// deferral list length.
int launch(yfm_ctx* ctx, const Launch& q, yfm::Workspace* ws = nullptr) {
  yfm::Workspace& w = ws ? *ws : ctx->own;
  // the context's own (synchronous) stream after a launch on a caller's stream: that launch may still run
  if (!ws && q.stream == ctx->stream) YFM_HIP_CHECK(yfm::settle_foreign_launch(ctx));
  if (!q.continues && (w.bank_dirty || q.stream != w.last_stream)) {
    YFM_HIP_CHECK(hipMemsetAsync(w.bank_ptr(w.bank ^ 1), 0, yfm::kFlagsPerBank * sizeof(unsigned int), q.stream));
    w.bank_dirty = false;
  }
  const int r = enqueue(ctx, q, w);
  if (r != YFM_OK) {
    w.bank_dirty = true;
    return r;
  }
  if (!q.continues) {
    w.bank ^= 1;
    w.last_stream = q.stream;
  }
  return YFM_OK;
}

// The gradient entry points' model check: the tangent kernel is built for DNS with N ≤ grad_max_n() only.
int check_grad(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (state_dim(kind) >= 0 && kind != YFM_MODEL_DNS)
    return set_error(YFM_EUNSUPPORTED, "log-likelihood gradients are built for YFM_MODEL_DNS only (model_kind %d)", kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::grad_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the gradient kernel's %d", ctx->N, yfm::grad_max_n());
  return YFM_OK;
}

// The TVλ gradient entry points' model check: the tangent kernel of yfm_tvl_grad.hip, every N the TVλ filter takes.
int check_tvl_grad(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (state_dim(kind) >= 0 && kind != YFM_MODEL_TVL)
    return set_error(YFM_EUNSUPPORTED, "yfm_tvl_loglik_grad_batch is built for YFM_MODEL_TVL only (model_kind %d: use "
                     "yfm_loglik_grad_batch for DNS)", kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::tvl_grad_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the TVλ gradient kernel's %d", ctx->N,
                     yfm::tvl_grad_max_n());
  return YFM_OK;
}

// The λ gradient entry points' model check: the five kinds of yfm_msed.hip only.
int check_lambda_grad(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (yfm::msedn_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "yfm_lambda_loss_grad_batch serves the λ kinds: the neural kinds' delta/Phi loss "
                     "gradient is yfm_neural_loss_grad_batch (model_kind %d)", kind);
  if (state_dim(kind) >= 0 && !yfm::msed_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "the δ/Φ loss gradient is built for the λ kinds only (model_kind %d: use "
                     "yfm_loglik_grad_batch)", kind);
  return check_batch(ctx, kind, space, P, B);
}

// The λ full-gradient entry points' model check: the five kinds of yfm_msed.hip only.
int check_lambda_fullgrad(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (yfm::msedn_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "yfm_lambda_loss_fullgrad_batch serves the λ kinds: the neural kinds have the "
                     "delta/Phi loss gradient of yfm_neural_loss_grad_batch only (model_kind %d)", kind);
  if (state_dim(kind) >= 0 && !yfm::msed_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "the full loss gradient is built for the λ kinds only (model_kind %d: use "
                     "yfm_loglik_grad_batch or yfm_tvl_loglik_grad_batch)", kind);
  return check_batch(ctx, kind, space, P, B);
}

// The neural gradient entry points' model check: the 26 kinds of yfm_msedn.hip only.
int check_neural_grad(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (state_dim(kind) >= 0 && !yfm::msedn_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "yfm_neural_loss_grad_batch is built for the neural kinds only (model_kind %d: "
                     "use yfm_lambda_loss_grad_batch or yfm_loglik_grad_batch)", kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::msedn_grad_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the neural gradient kernel's %d", ctx->N,
                     yfm::msedn_grad_max_n());
  return YFM_OK;
}

// The neural full-gradient entry points' model check: the 26 kinds of yfm_msedn.hip, at the N its two sweeps take.
int check_neural_fullgrad(yfm_ctx* ctx, int kind, int space, int P, int B) {
  if (state_dim(kind) >= 0 && !yfm::msedn_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "yfm_neural_loss_fullgrad_batch is built for the neural kinds only (model_kind "
                     "%d: use yfm_lambda_loss_fullgrad_batch, yfm_loglik_grad_batch or yfm_tvl_loglik_grad_batch)", kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::msedn_fullgrad_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the neural full-gradient kernels' %d", ctx->N,
                     yfm::msedn_fullgrad_max_n());
  return YFM_OK;
}

// What a tangent kernel enqueued after the loglik launch q (on the context's own workspace) reads: that launch's
// inputs, its counter bank and its deferral list.
yfm::LaunchArgs tangent_args(yfm_ctx* ctx, const Launch& q) {
  yfm::Workspace& w = ctx->own;
  yfm::LaunchArgs a = base_args(ctx, q);
  a.flags = w.bank_ptr(w.bank);  // the bank of the loglik launch just enqueued
  a.defer_list = static_cast<int*>(w.defer.p);
  return a;
}

// The loglik launch q on the context's own workspace, then the tangent kernel on the same stream: it reads the
// logliks q.out and (DNS) that launch's deferral list and adds n_grad_unavailable to its counter bank.
int launch_grad(yfm_ctx* ctx, const Launch& q, double* d_grad) {
  if (int r = launch(ctx, q)) return r;
  if (q.B == 0) return YFM_OK;
  yfm::Workspace& w = ctx->own;
  const yfm::LaunchArgs a = tangent_args(ctx, q);
  const hipError_t e = q.kind == YFM_MODEL_TVL ? yfm::launch_tvl_grad(a, q.out, d_grad)
                                               : yfm::launch_dns_grad(a, q.out, d_grad);
  if (e != hipSuccess) {
    w.bank_dirty = true;
    return set_error(YFM_EHIP, "gradient kernel launch: %s", hipGetErrorString(e));
  }
  return YFM_OK;
}

// The launch of a host-pointer call: θ (and T_use) uploaded into the context's staging buffers on its stream,
// the logliks to go to ctx->out.
int stage_inputs(yfm_ctx* ctx, int kind, int space, const double* theta, int P, int B, const int* T_use, Launch& q) {
  const size_t nb = (size_t)(B > 0 ? B : 1);
  YFM_HIP_CHECK(ctx->theta.ensure(sizeof(double) * (size_t)P * nb));
  YFM_HIP_CHECK(ctx->out.ensure(sizeof(double) * nb));
  if (B > 0)
    YFM_HIP_CHECK(hipMemcpyAsync(ctx->theta.p, theta, sizeof(double) * (size_t)P * B, hipMemcpyHostToDevice,
                                 ctx->stream));
  q = loglik_launch(kind, space, static_cast<const double*>(ctx->theta.p), P, B, nullptr,
                    static_cast<double*>(ctx->out.p), ctx->stream);
  if (T_use && B > 0) {
    YFM_HIP_CHECK(ctx->tuse.ensure(sizeof(int) * nb));
    YFM_HIP_CHECK(hipMemcpyAsync(ctx->tuse.p, T_use, sizeof(int) * B, hipMemcpyHostToDevice, ctx->stream));
    q.T_use = static_cast<const int*>(ctx->tuse.p);
  }
  return YFM_OK;
}

// Trajectory mode: run the staged launch q recording the last q.rec_len states of every
// candidate into ctx->traj and mark the candidates whose initialize_filter threw.
int run_trajectory(yfm_ctx* ctx, Launch q) {
  const size_t n = (size_t)q.B * q.rec_len * state_dim(q.kind);
  YFM_HIP_CHECK(ctx->traj.ensure(sizeof(double) * (n > 0 ? n : 1)));
  YFM_HIP_CHECK(ctx->init_bad.ensure((size_t)(q.B > 0 ? q.B : 1)));
  YFM_HIP_CHECK(hipMemsetAsync(ctx->traj.p, 0xff, sizeof(double) * n, ctx->stream));  // NaN fill
  q.rec_beta = static_cast<double*>(ctx->traj.p);
  if (int r = launch(ctx, q)) return r;
  YFM_HIP_CHECK(yfm::launch_init_bad(q.out, q.B, static_cast<unsigned char*>(ctx->init_bad.p), ctx->stream));
  return YFM_OK;
}

// The emit kernels' view of the trajectory that run_trajectory(ctx, q) recorded; `a` brings the output pointers.
yfm::PredictArgs predict_args(yfm_ctx* ctx, const Launch& q, int horizon, yfm::PredictArgs a) {
  a.kind = q.kind;
  a.M = state_dim(q.kind);
  a.L = gamma_dim(q.kind);
  a.N = ctx->N;
  a.P = q.P;
  a.B = q.B;
  a.T = ctx->T;
  a.horizon = horizon;
  a.ncol = ctx->T + horizon - 1;
  a.theta = q.theta;
  a.mats = static_cast<const double*>(ctx->mats.p);
  a.T_use = q.T_use;
  a.rec = static_cast<const double*>(ctx->traj.p);
  a.rec_len = q.rec_len;
  a.init_bad = static_cast<const unsigned char*>(ctx->init_bad.p);
  a.stream = ctx->stream;
  return a;
}

// Record mode of the λ and neural kinds: the kernel writes the trajectory outputs of `o` itself, into the NaN-filled
// block of `bytes` that starts at o.preds.
int launch_record(yfm_ctx* ctx, Launch q, int mode, int horizon, int ncol, const yfm::PredictArgs& o, size_t bytes) {
  YFM_HIP_CHECK(hipMemsetAsync(o.preds, 0xff, bytes, ctx->stream));
  yfm::MsedRecord rec;
  rec.mode = mode;
  rec.horizon = horizon;
  rec.ncol = ncol;
  rec.preds = o.preds;
  rec.factors = o.factors;
  rec.states = o.states;
  rec.load1 = o.load1;
  rec.load2 = o.load2;
  q.msed_rec = &rec;
  return launch(ctx, q);
}

// The counters of the context's last launch (layout: yfm_flags.hpp).
int read_flags(yfm_ctx* ctx, unsigned int (&h)[yfm::kFlagsPerBank]) {
  if (int r = check_ctx(ctx)) return r;
  YFM_HIP_CHECK(hipMemcpy(h, ctx->own.bank_ptr(ctx->own.bank), sizeof(h), hipMemcpyDeviceToHost));
  return YFM_OK;
}

int validate_tuse(const int* T_use, int B, int T) {
  if (!T_use) return YFM_OK;
  for (int b = 0; b < B; ++b)
    if (T_use[b] < 1 || T_use[b] > T)
      return set_error(YFM_EINVAL, "T_use[%d] = %d outside [1, %d]", b, T_use[b], T);
  return YFM_OK;
}

using GradCheck = int (*)(yfm_ctx*, int, int, int, int);

// A gradient call family: its model check, what its value is called in messages, the rows of its gradient and how its
// launch is made.
struct GradFamily {
  GradCheck check;
  const char* value;  // "loglik" or "loss"
  int rows;           // gradient rows per candidate (0: one per row of θ)
  enum { kTangent, kMsedGrad, kMsedFullGrad } how;  // launch_grad, or launch with msed_grad / msed_fullgrad set
};
const GradFamily kDnsGrad{check_grad, "loglik", 0, GradFamily::kTangent};
const GradFamily kTvlGrad{check_tvl_grad, "loglik", 0, GradFamily::kTangent};
const GradFamily kLambdaGrad{check_lambda_grad, "loss", yfm::kMsedGrad, GradFamily::kMsedGrad};
const GradFamily kLambdaFullGrad{check_lambda_fullgrad, "loss", 0, GradFamily::kMsedFullGrad};
const GradFamily kNeuralGrad{check_neural_grad, "loss", yfm::kMsedGrad, GradFamily::kMsedGrad};
const GradFamily kNeuralFullGrad{check_neural_fullgrad, "loss", 0, GradFamily::kMsedFullGrad};

// The launch of family f for q, the gradient to go to d_grad.
int launch_family(yfm_ctx* ctx, const GradFamily& f, Launch q, double* d_grad) {
  if (f.how == GradFamily::kTangent) return launch_grad(ctx, q, d_grad);
  (f.how == GradFamily::kMsedFullGrad ? q.msed_fullgrad : q.msed_grad) = d_grad;
  return launch(ctx, q);
}

// The six host-pointer gradient entry points: one path, each family with its own model check and launch.
int grad_batch(const GradFamily& f, yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
               const int* T_use, double* value_out, double* grad_out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = f.check(ctx, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!theta || !value_out || !grad_out))
    return set_error(YFM_EINVAL, "null theta, %s_out or grad_out", f.value);
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  const size_t rows = f.rows > 0 ? (size_t)f.rows : (size_t)P;
  YFM_HIP_CHECK(ctx->own.grad.ensure(sizeof(double) * rows * (size_t)(B > 0 ? B : 1)));
  double* const d_grad = static_cast<double*>(ctx->own.grad.p);
  if (int r = launch_family(ctx, f, q, d_grad)) return r;
  if (B > 0) {
    YFM_HIP_CHECK(hipMemcpyAsync(value_out, q.out, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
    YFM_HIP_CHECK(hipMemcpyAsync(grad_out, d_grad, sizeof(double) * rows * (size_t)B, hipMemcpyDeviceToHost,
                                 ctx->stream));
  }
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

// Their device-pointer twins: the launch alone, asynchronous on the caller's stream.
int grad_batch_device(const GradFamily& f, yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                      int B, const int* d_T_use, double* d_value_out, double* d_grad_out, void* hip_stream) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = f.check(ctx, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!d_theta || !d_value_out || !d_grad_out))
    return set_error(YFM_EINVAL, "null d_theta, d_%s_out or d_grad_out", f.value);
  return launch_family(ctx, f, loglik_launch(model_kind, param_space, d_theta, P, B, d_T_use, d_value_out,
                                             static_cast<hipStream_t>(hip_stream)), d_grad_out);
}

// The score / information entry points' model check: they run the DNS tangent recursion, so its limits hold.
int check_info(yfm_ctx* ctx, const char* what, int kind, int space, int P, int B) {
  if (state_dim(kind) >= 0 && kind != YFM_MODEL_DNS)
    return set_error(YFM_EUNSUPPORTED, "%s is built for YFM_MODEL_DNS only (model_kind %d): no score series, "
                     "information matrix or Hessian exists for the other kinds", what, kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::grad_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the %d of the tangent kernel that %s runs", ctx->N,
                     yfm::grad_max_n(), what);
  return YFM_OK;
}

// The TVλ score / information entry points' model check: they run the TVλ tangent recursion, every N it takes.
int check_tvl_info(yfm_ctx* ctx, const char* what, int kind, int space, int P, int B) {
  if (state_dim(kind) >= 0 && kind != YFM_MODEL_TVL)
    return set_error(YFM_EUNSUPPORTED, "%s is built for YFM_MODEL_TVL only (model_kind %d): the DNS score series, "
                     "information matrix and Hessian are yfm_loglik_scores_batch and yfm_loglik_info_batch, and none "
                     "exists for the other kinds", what, kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::tvl_grad_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the %d of the tangent kernel that %s runs", ctx->N,
                     yfm::tvl_grad_max_n(), what);
  return YFM_OK;
}

// A score / information call family: its model check, its default Hessian step and the gradient call its messages
// point to.  Its kernels follow the kind (score_launch, launch_grad, launch_opg by P).
struct InfoFamily {
  int (*check)(yfm_ctx*, const char*, int, int, int, int);
  double default_step;
  const char* grad_call;
};
const InfoFamily kDnsInfo{check_info, YFM_INFO_DEFAULT_STEP, "yfm_loglik_grad_batch"};
const InfoFamily kTvlInfo{check_tvl_info, YFM_TVL_INFO_DEFAULT_STEP, "yfm_tvl_loglik_grad_batch"};

// No temporary that the score / information entry points add is larger than this: bigger batches go chunk by chunk.
// (The batch's own staging — θ, T_use, loglik, gradient and the work records of its loglik launch — is what
// yfm_loglik_grad_batch allocates for the same batch.)
constexpr size_t kInfoChunkBytes = (size_t)128 << 20;

int info_chunk(size_t bytes_per_candidate, int B) {
  const size_t n = kInfoChunkBytes / std::max<size_t>(bytes_per_candidate, 1);
  return (int)std::min<size_t>(std::max<size_t>(n, 1), (size_t)std::max(B, 1));
}

// The largest work buffer enqueue() grows for a fixed-loading loglik launch of n candidates (the double-double records
// of the deferral path, the per-lane kernel's init records, the deferral list).
size_t fixedz_launch_bytes(int kind, int n) {
  return std::max({yfm::fixedz_dd_scratch_bytes(kind, n), yfm::fixedz_scratch_bytes(kind, n), sizeof(int) * (size_t)n});
}

// The work records enqueue() grows for a TVλ loglik launch of n candidates under the context's precision.
size_t tvl_launch_bytes(const yfm_ctx* ctx, int n) {
  return ctx->precision == YFM_PREC_CERTIFIED ? yfm::tvl_dd_scratch_bytes(n) : yfm::tvl_scratch_bytes(n);
}

// The score kernel of q's kind for candidates b0 … b0 + nb − 1 of the loglik launch q (`count`: DNS counts the
// deferred into the launch's bank; the TVλ kernel always counts its own unavailable candidates there).
hipError_t score_launch(const yfm::LaunchArgs& a, const Launch& q, double* d_scores, int b0, int nb, bool count) {
  return q.kind == YFM_MODEL_TVL ? yfm::launch_tvl_scores(a, q.out, d_scores, b0, nb)
                                 : yfm::launch_dns_scores(a, q.out, d_scores, b0, nb, count);
}

// The scores of the candidates of the loglik launch q (the last one enqueued on the own workspace), chunk by chunk
// through info_scores; `each(b0, nb, d_scores)` consumes a chunk before the next one overwrites it (same stream).
// `out_per`: bytes per candidate of what `each` itself keeps per chunk.
template <class F>
int for_score_chunks(yfm_ctx* ctx, const Launch& q, bool count, size_t out_per, F&& each) {
  const size_t per = sizeof(double) * (size_t)q.P * (size_t)std::max(ctx->T - 1, 0);
  const int chunk = info_chunk(std::max(per, out_per), q.B);
  YFM_HIP_CHECK(ctx->own.info_scores.ensure(per * chunk));
  double* const d_scores = static_cast<double*>(ctx->own.info_scores.p);
  const yfm::LaunchArgs a = tangent_args(ctx, q);
  for (int b0 = 0; b0 < q.B; b0 += chunk) {
    const int nb = std::min(chunk, q.B - b0);
    const hipError_t e = score_launch(a, q, d_scores, b0, nb, count);
    if (e != hipSuccess) {
      ctx->own.bank_dirty = true;
      return set_error(YFM_EHIP, "score kernel launch: %s", hipGetErrorString(e));
    }
    if (int r = each(b0, nb, d_scores)) return r;
  }
  return YFM_OK;
}

// The chunk `start` shrunk until need(chunk), the bytes a launch of that many candidates allocates, is within
// kInfoChunkBytes (or one candidate is left).
template <class F>
int fit_chunk(int start, F&& need) {
  int chunk = start;
  while (chunk > 1) {
    const size_t nb = need(chunk);
    if (nb <= kInfoChunkBytes) break;
    const int fit = (int)((double)chunk * ((double)kInfoChunkBytes / (double)nb));
    chunk = std::max(1, std::min(chunk - 1, fit));
  }
  return chunk;
}

// Candidates per Hessian chunk: the 4P perturbed θ and their gradients (P doubles per point each), and everything the
// loglik launch of the chunk's 4P·nb points allocates, each within kInfoChunkBytes.
int hessian_chunk(const yfm_ctx* ctx, int kind, int P, int B) {
  const size_t np = 4 * (size_t)P;
  return fit_chunk(info_chunk(sizeof(double) * (size_t)P * np, B), [&](int n) {
    return kind == YFM_MODEL_TVL ? tvl_launch_bytes(ctx, (int)(np * n)) : fixedz_launch_bytes(kind, (int)(np * n));
  });
}

// H of every candidate of the staged launch q, chunk by chunk: the perturbed points, their logliks and gradients (the
// existing launches, on the own workspace), the assembly with the unavailable rule (d_grad: the batch's own gradients;
// d_count: raised per unavailable candidate), and the chunk's H to the host.
int hessian_chunks(yfm_ctx* ctx, const Launch& q, double h, const double* d_grad, unsigned int* d_count,
                   double* hess_out) {
  yfm::Workspace& w = ctx->own;
  const size_t P = (size_t)q.P, np = 4 * P;  // points per candidate
  const int chunk = hessian_chunk(ctx, q.kind, q.P, q.B);
  YFM_HIP_CHECK(w.info_pts.ensure(sizeof(double) * P * np * chunk));
  YFM_HIP_CHECK(w.info_pgrad.ensure(sizeof(double) * P * np * chunk));
  // logliks (np), realised steps (2P), windows (np ints) per candidate
  YFM_HIP_CHECK(w.info_pmisc.ensure((sizeof(double) * (np + 2 * P) + sizeof(int) * np) * chunk));
  YFM_HIP_CHECK(w.info_out.ensure(sizeof(double) * P * P * chunk));
  double* const d_pts = static_cast<double*>(w.info_pts.p);
  double* const d_pgrad = static_cast<double*>(w.info_pgrad.p);
  double* const d_pll = static_cast<double*>(w.info_pmisc.p);
  double* const d_steps = d_pll + np * chunk;
  int* const d_ptu = reinterpret_cast<int*>(d_steps + 2 * P * chunk);
  double* const d_H = static_cast<double*>(w.info_out.p);
  for (int b0 = 0; b0 < q.B; b0 += chunk) {
    const int nb = std::min(chunk, q.B - b0);
    YFM_HIP_CHECK(yfm::launch_hessian_points(q.theta + P * b0, q.P, nb, q.T_use ? q.T_use + b0 : nullptr, h, d_pts,
                                             d_ptu, d_steps, q.stream));
    const Launch qp = loglik_launch(q.kind, q.space, d_pts, q.P, (int)np * nb, q.T_use ? d_ptu : nullptr, d_pll,
                                    q.stream);
    if (int r = launch_grad(ctx, qp, d_pgrad)) return r;
    YFM_HIP_CHECK(yfm::launch_hessian_assemble(d_pgrad, d_steps, d_grad + P * b0, q.P, nb, d_H, d_count, q.stream));
    YFM_HIP_CHECK(hipMemcpyAsync(hess_out + P * P * b0, d_H, sizeof(double) * P * P * nb, hipMemcpyDeviceToHost,
                                 q.stream));
  }
  return YFM_OK;
}

// The score entry points of a family: the loglik launch, then the scores chunk by chunk to the host.
int scores_batch(const InfoFamily& f, const char* what, yfm_ctx* ctx, int model_kind, int param_space,
                 const double* theta, int P, int B, const int* T_use, double* loglik_out, double* scores_out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = f.check(ctx, what, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!theta || !loglik_out || !scores_out))
    return set_error(YFM_EINVAL, "null theta, loglik_out or scores_out");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  if (int r = launch(ctx, q)) return r;
  if (B > 0) {
    YFM_HIP_CHECK(hipMemcpyAsync(loglik_out, q.out, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
    const size_t per = (size_t)P * (size_t)(ctx->T - 1);
    const int rc = for_score_chunks(ctx, q, true, 0, [&](int b0, int nb, const double* d_scores) {
      if (per > 0)
        YFM_HIP_CHECK(hipMemcpyAsync(scores_out + per * b0, d_scores, sizeof(double) * per * nb, hipMemcpyDeviceToHost,
                                     ctx->stream));
      return (int)YFM_OK;
    });
    if (rc != YFM_OK) return rc;
  }
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

// Their device-pointer twin: both launches alone, asynchronous on the caller's stream.
int scores_batch_device(const InfoFamily& f, const char* what, yfm_ctx* ctx, int model_kind, int param_space,
                        const double* d_theta, int P, int B, const int* d_T_use, double* d_loglik_out,
                        double* d_scores_out, void* hip_stream) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = f.check(ctx, what, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!d_theta || !d_loglik_out || !d_scores_out))
    return set_error(YFM_EINVAL, "null d_theta, d_loglik_out or d_scores_out");
  const Launch q = loglik_launch(model_kind, param_space, d_theta, P, B, d_T_use, d_loglik_out,
                                 static_cast<hipStream_t>(hip_stream));
  if (int r = launch(ctx, q)) return r;
  if (B == 0) return YFM_OK;
  const hipError_t e = score_launch(tangent_args(ctx, q), q, d_scores_out, 0, B, true);
  if (e != hipSuccess) {
    ctx->own.bank_dirty = true;
    return set_error(YFM_EHIP, "score kernel launch: %s", hipGetErrorString(e));
  }
  return YFM_OK;
}

// The information entry points of a family: loglik and gradient, J from the score chunks, H from the Hessian chunks.
int info_batch(const InfoFamily& f, const char* what, yfm_ctx* ctx, int model_kind, int param_space, const double* theta,
               int P, int B, const int* T_use, int lags, double step, double* loglik_out, double* grad_out,
               double* hess_out, double* opg_out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = f.check(ctx, what, model_kind, param_space, P, B)) return r;
  if (lags < 0) return set_error(YFM_EINVAL, "lags = %d < 0 (0: the plain outer product of the scores)", lags);
  if (!hess_out && !opg_out)
    return set_error(YFM_EINVAL, "hess_out and opg_out are both null: %s is the call for the loglik and its gradient "
                     "alone", f.grad_call);
  if (!(step == step) || step > 1.79769313486231570815e308)
    return set_error(YFM_EINVAL, "step is not a finite number (<= 0: the default)");
  if (B > 0 && (!theta || !loglik_out || !grad_out)) return set_error(YFM_EINVAL, "null theta, loglik_out or grad_out");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  yfm::Workspace& w = ctx->own;
  const size_t PP = (size_t)P * P;
  YFM_HIP_CHECK(w.grad.ensure(sizeof(double) * (size_t)P * (size_t)(B > 0 ? B : 1)));
  YFM_HIP_CHECK(w.info_flags.ensure(sizeof(unsigned int) * (yfm::kFlagsPerBank + 1)));
  double* const d_grad = static_cast<double*>(w.grad.p);
  unsigned int* const d_saved = static_cast<unsigned int*>(w.info_flags.p);
  unsigned int* const d_count = d_saved + yfm::kFlagsPerBank;  // the candidates with a NaN H (no Hessian: a NaN J)
  YFM_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned int), ctx->stream));
  // the batch's own loglik and gradient, bitwise the gradient call's
  if (int r = launch_grad(ctx, q, d_grad)) return r;
  if (B > 0) {
    YFM_HIP_CHECK(hipMemcpyAsync(loglik_out, q.out, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
    YFM_HIP_CHECK(hipMemcpyAsync(grad_out, d_grad, sizeof(double) * (size_t)P * B, hipMemcpyDeviceToHost, ctx->stream));
    if (opg_out) {  // before any other launch: the scores read this launch's deferral list
      const int rc = for_score_chunks(ctx, q, false, sizeof(double) * PP, [&](int b0, int nb, const double* d_scores) {
        YFM_HIP_CHECK(w.info_out.ensure(sizeof(double) * PP * nb));
        double* const d_J = static_cast<double*>(w.info_out.p);
        YFM_HIP_CHECK(yfm::launch_opg(P, d_scores, ctx->T, nb, q.T_use ? q.T_use + b0 : nullptr, lags,
                                      d_grad + (size_t)P * b0, d_J, hess_out ? nullptr : d_count, ctx->stream));
        YFM_HIP_CHECK(hipMemcpyAsync(opg_out + PP * b0, d_J, sizeof(double) * PP * nb, hipMemcpyDeviceToHost,
                                     ctx->stream));
        return (int)YFM_OK;
      });
      if (rc != YFM_OK) return rc;
    }
    if (hess_out) {
      // the perturbed launches take over the counter banks: the batch's own counters are kept and put back into the
      // bank of the last launch, so yfm_last_batch_flags, _deferred and _steady answer for the batch itself
      YFM_HIP_CHECK(hipMemcpyAsync(d_saved, w.bank_ptr(w.bank), sizeof(unsigned int) * yfm::kFlagsPerBank,
                                   hipMemcpyDeviceToDevice, ctx->stream));
      if (int r = hessian_chunks(ctx, q, step > 0.0 ? step : f.default_step, d_grad, d_count, hess_out))
        return r;
      YFM_HIP_CHECK(hipMemcpyAsync(w.bank_ptr(w.bank), d_saved, sizeof(unsigned int) * yfm::kFlagsPerBank,
                                   hipMemcpyDeviceToDevice, ctx->stream));
    }
    YFM_HIP_CHECK(hipMemcpyAsync(w.bank_ptr(w.bank) + 5, d_count, sizeof(unsigned int), hipMemcpyDeviceToDevice,
                                 ctx->stream));
  }
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

// The smoother entry points' model check: the backward sweep is built for the fixed-loading Kalman models.
int check_smooth(yfm_ctx* ctx, const char* what, int kind, int space, int P, int B) {
  if (kind == YFM_MODEL_TVL)
    return set_error(YFM_EUNSUPPORTED, "%s is built for YFM_MODEL_DNS and YFM_MODEL_GNS5: the TVlambda model's loadings "
                     "move with the state, and its extended smoother is yfm_tvl_smooth_batch (model_kind %d)", what, kind);
  if (yfm::msed_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "%s is built for YFM_MODEL_DNS and YFM_MODEL_GNS5: the %s kinds are not Kalman "
                     "filters and have no state covariance to smooth (model_kind %d)", what,
                     yfm::msedn_kind(kind) ? "neural" : "lambda", kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::smooth_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the %d of the smoother's backward sweep", ctx->N,
                     yfm::smooth_max_n());
  return YFM_OK;
}

// The TVλ extended smoother's model check: yfm_tvl_smooth.hip, every N the TVλ filter takes.
int check_tvl_smooth(yfm_ctx* ctx, const char* what, int kind, int space, int P, int B) {
  if (kind == YFM_MODEL_DNS || kind == YFM_MODEL_GNS5)
    return set_error(YFM_EUNSUPPORTED, "%s is built for YFM_MODEL_TVL only: the fixed-loading models' smoother is "
                     "yfm_smooth_batch (model_kind %d)", what, kind);
  if (yfm::msed_kind(kind))
    return set_error(YFM_EUNSUPPORTED, "%s is built for YFM_MODEL_TVL only: the %s kinds are not Kalman filters, "
                     "there is nothing to smooth (model_kind %d)", what, yfm::msedn_kind(kind) ? "neural" : "lambda",
                     kind);
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  if (ctx->N > yfm::tvl_smooth_max_n())
    return set_error(YFM_EUNSUPPORTED, "N = %d maturities exceeds the %d of the TVλ smoother's backward sweep", ctx->N,
                     yfm::tvl_smooth_max_n());
  return YFM_OK;
}

// Candidates per smoother chunk: the forward record (a and P of T − 1 steps), each output array and everything the
// trajectory launch of the chunk allocates, each within kInfoChunkBytes.
int smooth_chunk(int kind, int M, int T, int B) {
  const size_t rec = sizeof(double) * (size_t)(M + M * M) * (size_t)std::max(T - 1, 1);
  const size_t out = sizeof(double) * (size_t)M * M * (size_t)T;
  return fit_chunk(info_chunk(std::max(rec, out), B), [&](int n) { return fixedz_launch_bytes(kind, n); });
}

// The same for the TVλ extended smoother (M = 4): the record (20 doubles × (T − 1)), each output array and the work
// records of the chunk's TVλ launch under the context's precision, each within kInfoChunkBytes.
int tvl_smooth_chunk(const yfm_ctx* ctx, int T, int B) {
  const size_t rec = sizeof(double) * 20 * (size_t)std::max(T - 1, 1);
  const size_t out = sizeof(double) * 16 * (size_t)T;
  return fit_chunk(info_chunk(std::max(rec, out), B), [&](int n) { return tvl_launch_bytes(ctx, n); });
}

// The smoother over the candidates of q (θ, T_use and the logliks q.out on the device), chunk by chunk on q.stream:
// the trajectory launch of the chunk into the record scratch, then the backward sweep.  h_beta null: the sweep writes
// into the caller's device arrays d_beta, d_V, d_C (whole batch).  Otherwise it writes a chunk's outputs into the
// context's staging buffers, which leave for h_beta, h_V, h_C before the next chunk (want_C: with the lag-one array).
int smooth_chunks(yfm_ctx* ctx, const Launch& q, double* d_beta, double* d_V, double* d_C, double* h_beta, double* h_V,
                  double* h_C, bool want_C) {
  yfm::Workspace& w = ctx->own;
  const int M = state_dim(q.kind), T = ctx->T;
  const size_t nM = (size_t)M * T, nV = (size_t)M * M * T, nC = (size_t)M * M * (size_t)(T - 1);
  const bool tvl = q.kind == YFM_MODEL_TVL;
  const int chunk = tvl ? tvl_smooth_chunk(ctx, T, q.B) : smooth_chunk(q.kind, M, T, q.B);
  const size_t steps = (size_t)std::max(T - 1, 1) * chunk;
  YFM_HIP_CHECK(w.smooth_rec_beta.ensure(sizeof(double) * steps * M));
  YFM_HIP_CHECK(w.smooth_rec_P.ensure(sizeof(double) * steps * M * M));
  YFM_HIP_CHECK(w.smooth_skip.ensure((size_t)chunk));
  if (h_beta) {
    YFM_HIP_CHECK(w.smooth_beta.ensure(sizeof(double) * nM * chunk));
    YFM_HIP_CHECK(w.smooth_V.ensure(sizeof(double) * nV * chunk));
    if (want_C) YFM_HIP_CHECK(w.smooth_C.ensure(sizeof(double) * std::max<size_t>(nC, 1) * chunk));
  }
  for (int b0 = 0; b0 < q.B; b0 += chunk) {
    const int nb = std::min(chunk, q.B - b0);
    Launch qc = q;
    qc.theta = q.theta + (size_t)q.P * b0;
    qc.B = nb;
    qc.T_use = q.T_use ? q.T_use + b0 : nullptr;
    qc.out = q.out + b0;
    qc.continues = b0 > 0;  // one batch: the chunks' counters add up
    qc.lanes_B = q.B;       // TVλ: every chunk's forward launch at the whole batch's lane count
    if (T >= 2) {           // a one-column panel has no recorded step: the sweep takes a_1, P_1 alone
      qc.rec_beta = static_cast<double*>(w.smooth_rec_beta.p);
      qc.rec_P = static_cast<double*>(w.smooth_rec_P.p);
      qc.rec_len = T - 1;
    }
    if (int r = launch(ctx, qc)) return r;
    yfm::LaunchArgs a = tangent_args(ctx, qc);
    a.rec_beta = qc.rec_beta;
    a.rec_P = qc.rec_P;
    a.rec_len = qc.rec_len;
    double* const ob = h_beta ? static_cast<double*>(w.smooth_beta.p) : d_beta + nM * b0;
    double* const oV = h_beta ? static_cast<double*>(w.smooth_V.p) : d_V + nV * b0;
    double* const oC = h_beta ? (want_C ? static_cast<double*>(w.smooth_C.p) : nullptr) : (d_C ? d_C + nC * b0 : nullptr);
    // measurement only (tools/bench_smooth.py, tools/bench_tvl_smooth.py): YFM_SMOOTH_SWEEP=0 leaves the sweep out, so the forward trajectory
    // launch can be timed alone; the outputs are then not written
    if (std::atoi(yfm::env_or("YFM_SMOOTH_SWEEP", "1")) == 0) continue;
    const hipError_t e =
        tvl ? yfm::launch_tvl_smooth(a, qc.out, ob, oV, oC)
            : yfm::launch_smooth(q.kind, a, qc.out, static_cast<unsigned char*>(w.smooth_skip.p), ob, oV, oC);
    if (e != hipSuccess) {
      w.bank_dirty = true;
      return set_error(YFM_EHIP, "smoother kernel launch: %s", hipGetErrorString(e));
    }
    if (h_beta) {
      YFM_HIP_CHECK(hipMemcpyAsync(h_beta + nM * b0, ob, sizeof(double) * nM * nb, hipMemcpyDeviceToHost, q.stream));
      YFM_HIP_CHECK(hipMemcpyAsync(h_V + nV * b0, oV, sizeof(double) * nV * nb, hipMemcpyDeviceToHost, q.stream));
      if (want_C && nC > 0)
        YFM_HIP_CHECK(hipMemcpyAsync(h_C + nC * b0, oC, sizeof(double) * nC * nb, hipMemcpyDeviceToHost, q.stream));
    }
  }
  return YFM_OK;
}

using SmoothCheck = int (*)(yfm_ctx*, const char*, int, int, int, int);

// yfm_smooth_batch and yfm_tvl_smooth_batch: one path, each with its own model check (`what`: the entry point's name)
int smooth_batch(SmoothCheck check, const char* what, yfm_ctx* ctx, int model_kind, int param_space,
                 const double* theta, int P, int B, const int* T_use, double* beta_s, double* V_s, double* C_s) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check(ctx, what, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!theta || !beta_s || !V_s)) return set_error(YFM_EINVAL, "null theta, beta_s or V_s");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  if (B == 0) {
    if (int r = launch(ctx, q)) return r;
  } else if (int r = smooth_chunks(ctx, q, nullptr, nullptr, nullptr, beta_s, V_s, C_s, C_s != nullptr)) {
    return r;
  }
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

int smooth_batch_device(SmoothCheck check, const char* what, yfm_ctx* ctx, int model_kind, int param_space,
                        const double* d_theta, int P, int B, const int* d_T_use, double* d_beta_s, double* d_V_s,
                        double* d_C_s, void* hip_stream) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check(ctx, what, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!d_theta || !d_beta_s || !d_V_s)) return set_error(YFM_EINVAL, "null d_theta, d_beta_s or d_V_s");
  YFM_HIP_CHECK(ctx->own.smooth_ll.ensure(sizeof(double) * (size_t)(B > 0 ? B : 1)));
  const Launch q = loglik_launch(model_kind, param_space, d_theta, P, B, d_T_use,
                                 static_cast<double*>(ctx->own.smooth_ll.p), static_cast<hipStream_t>(hip_stream));
  if (B == 0) return launch(ctx, q);
  return smooth_chunks(ctx, q, d_beta_s, d_V_s, d_C_s, nullptr, nullptr, nullptr, false);
}

}  // namespace

namespace yfm {
int api_error(int code, const char* msg) { return set_error(code, "%s", msg); }
int panel_T(const yfm_ctx* ctx) { return ctx ? ctx->T : 0; }

hipError_t settle_foreign_launch(yfm_ctx* ctx) {
  if (!ctx || !ctx->own.last_stream || ctx->own.last_stream == ctx->stream) return hipSuccess;
  const hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) ctx->own.last_stream = nullptr;  // nothing of the context is in flight any more
  return e;
}
}  // namespace yfm

extern "C" {

int yfm_abi_version(void) { return YFM_ABI_VERSION; }
int yfm_param_count(int model_kind) { return param_count(model_kind); }
int yfm_state_dim(int model_kind) { return state_dim(model_kind); }
const char* yfm_last_error(void) { return g_last_error.c_str(); }

yfm_ctx* yfm_create(int hip_device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_error(YFM_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
    return nullptr;
  }
  if (hip_device < 0 || hip_device >= n) {
    set_error(YFM_EINVAL, "hip_device %d out of range [0, %d)", hip_device, n);
    return nullptr;
  }
  if (hipSetDevice(hip_device) != hipSuccess) {
    set_error(YFM_EHIP, "hipSetDevice(%d) failed", hip_device);
    return nullptr;
  }
  yfm_ctx* ctx = new yfm_ctx();
  ctx->device = hip_device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      ctx->own.init() != hipSuccess) {
    set_error(YFM_EHIP, "context allocation failed on device %d", hip_device);
    yfm_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

void yfm_destroy(yfm_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (hipStream_t s : {ctx->stream, ctx->copy_stream}) {
    if (!s) continue;
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  delete ctx;  // every buffer frees itself
}

void* yfm_alloc_host(size_t bytes) {
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes > 0 ? bytes : 1, hipHostMallocPortable);
  if (e != hipSuccess) {
    set_error(YFM_EHIP, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}

int yfm_free_host(void* p) {
  if (!p) return YFM_OK;
  YFM_HIP_CHECK(hipHostFree(p));
  return YFM_OK;
}

int yfm_set_precision(yfm_ctx* ctx, int precision) {
  if (int r = check_ctx(ctx)) return r;
  if (precision != YFM_PREC_CERTIFIED && precision != YFM_PREC_FP64)
    return set_error(YFM_EINVAL, "unknown precision %d", precision);
  ctx->precision = precision;
  return YFM_OK;
}

int yfm_get_precision(yfm_ctx* ctx) {
  if (!ctx) return set_error(YFM_EINVAL, "null context");
  return ctx->precision;
}

int yfm_set_panel(yfm_ctx* ctx, const double* Y, int N, int T, const double* maturities) {
  if (int r = check_ctx(ctx)) return r;
  YFM_HIP_CHECK(yfm::settle_foreign_launch(ctx));  // a launch on a caller's stream may still read the panel
  if (!Y || !maturities) return set_error(YFM_EINVAL, "null Y or maturities");
  if (N < 1 || T < 1) return set_error(YFM_EINVAL, "N = %d, T = %d must be >= 1", N, T);
  const int np = yfm::fixedz_np_for(N);
  const int npad = np > 0 ? np : ((N + 7) / 8) * 8;
  const int ldp = npad + 4;
  YFM_HIP_CHECK(ctx->raw.ensure(sizeof(double) * (size_t)N * T));
  YFM_HIP_CHECK(ctx->panel.ensure(sizeof(double) * (size_t)ldp * T));
  YFM_HIP_CHECK(ctx->mats.ensure(sizeof(double) * (size_t)N));
  YFM_HIP_CHECK(hipMemcpyAsync(ctx->raw.p, Y, sizeof(double) * (size_t)N * T, hipMemcpyHostToDevice, ctx->stream));
  YFM_HIP_CHECK(hipMemcpyAsync(ctx->mats.p, maturities, sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream));
  YFM_HIP_CHECK(yfm::launch_prep_panel(static_cast<const double*>(ctx->raw.p), N, T, npad, ldp,
                                       static_cast<double*>(ctx->panel.p), ctx->stream));
  YFM_HIP_CHECK(ctx->colsum.ensure(yfm::tvl_dd_colsum_bytes(T)));
  YFM_HIP_CHECK(yfm::launch_tvl_dd_colsum(static_cast<const double*>(ctx->raw.p), N, T,
                                          static_cast<double*>(ctx->colsum.p), ctx->stream));
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->N = N;
  ctx->T = T;
  ctx->mats_host.assign(maturities, maturities + N);
  for (auto& t : ctx->tvl_tab) t.K = -1;
  ctx->np = npad;
  ctx->ldp = ldp;
  return YFM_OK;
}

int yfm_loglik_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                     const int* T_use, double* loglik_out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!theta || !loglik_out)) return set_error(YFM_EINVAL, "null theta or loglik_out");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  // Batches that fill the chip several times over are pipelined: chunk k+1's θ is uploaded on
  // the copy stream while chunk k's filter runs on the context stream (each chunk still holds
  // ≥ 2 waves per SIMD of candidates).  Evaluations are independent, so the logliks are the
  // same bits as one launch; the flags accumulate over the chunks.
  int chunk = B;
  if (model_kind != YFM_MODEL_TVL && B >= 2 * kPipeChunk) {
    chunk = std::max(kPipeChunk, (B + kPipeMaxChunks - 1) / kPipeMaxChunks);
    if (!ctx->copy_stream) YFM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  }
  if (chunk < B) {
    YFM_HIP_CHECK(ctx->theta.ensure(sizeof(double) * (size_t)P * B));
    YFM_HIP_CHECK(ctx->out.ensure(sizeof(double) * B));
    if (T_use) YFM_HIP_CHECK(ctx->tuse.ensure(sizeof(int) * B));
    double* d_th = static_cast<double*>(ctx->theta.p);
    double* d_out = static_cast<double*>(ctx->out.p);
    int* d_tu = T_use ? static_cast<int*>(ctx->tuse.p) : nullptr;
    const int nchunks = (B + chunk - 1) / chunk;
    std::vector<hipEvent_t> ev(nchunks, nullptr);
    int rc = YFM_OK;
    for (int k = 0; k < nchunks && rc == YFM_OK; ++k) {
      const int b0 = k * chunk, nbk = std::min(chunk, B - b0);
      hipError_t e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
      if (e == hipSuccess)
        e = hipMemcpyAsync(d_th + (size_t)P * b0, theta + (size_t)P * b0, sizeof(double) * (size_t)P * nbk,
                           hipMemcpyHostToDevice, ctx->copy_stream);
      if (e == hipSuccess && d_tu)
        e = hipMemcpyAsync(d_tu + b0, T_use + b0, sizeof(int) * nbk, hipMemcpyHostToDevice, ctx->copy_stream);
      if (e == hipSuccess) e = hipEventRecord(ev[k], ctx->copy_stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ev[k], 0);
      if (e != hipSuccess) {
        rc = set_error(YFM_EHIP, "pipelined upload: %s", hipGetErrorString(e));
        break;
      }
      Launch q = loglik_launch(model_kind, param_space, d_th + (size_t)P * b0, P, nbk, d_tu ? d_tu + b0 : nullptr,
                               d_out + b0, ctx->stream);
      q.continues = k > 0;
      rc = launch(ctx, q);
    }
    if (rc == YFM_OK) {
      hipError_t e = hipMemcpyAsync(loglik_out, d_out, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream);
      if (e != hipSuccess) rc = set_error(YFM_EHIP, "hipMemcpyAsync: %s", hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(ctx->copy_stream);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    for (hipEvent_t x : ev)
      if (x) (void)hipEventDestroy(x);
    if (rc == YFM_OK && e != hipSuccess) rc = set_error(YFM_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    return rc;
  }
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  if (int r = launch(ctx, q)) return r;
  if (B > 0)
    YFM_HIP_CHECK(hipMemcpyAsync(loglik_out, q.out, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

int yfm_loglik_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                            const int* d_T_use, double* d_loglik_out, void* hip_stream) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, model_kind, param_space, P, B)) return r;
  if (B > 0 && (!d_theta || !d_loglik_out)) return set_error(YFM_EINVAL, "null d_theta or d_loglik_out");
  return launch(ctx, loglik_launch(model_kind, param_space, d_theta, P, B, d_T_use, d_loglik_out,
                                   static_cast<hipStream_t>(hip_stream)));
}

int yfm_loglik_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                          const int* T_use, double* loglik_out, double* grad_out) {
  return grad_batch(kDnsGrad, ctx, model_kind, param_space, theta, P, B, T_use, loglik_out, grad_out);
}

int yfm_loglik_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                                 const int* d_T_use, double* d_loglik_out, double* d_grad_out, void* hip_stream) {
  return grad_batch_device(kDnsGrad, ctx, model_kind, param_space, d_theta, P, B, d_T_use, d_loglik_out, d_grad_out,
                           hip_stream);
}

int yfm_tvl_loglik_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                              const int* T_use, double* loglik_out, double* grad_out) {
  return grad_batch(kTvlGrad, ctx, model_kind, param_space, theta, P, B, T_use, loglik_out, grad_out);
}

int yfm_tvl_loglik_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                     int B, const int* d_T_use, double* d_loglik_out, double* d_grad_out,
                                     void* hip_stream) {
  return grad_batch_device(kTvlGrad, ctx, model_kind, param_space, d_theta, P, B, d_T_use, d_loglik_out, d_grad_out,
                           hip_stream);
}

int yfm_lambda_loss_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                               const int* T_use, double* loss_out, double* grad_out) {
  return grad_batch(kLambdaGrad, ctx, model_kind, param_space, theta, P, B, T_use, loss_out, grad_out);
}

int yfm_lambda_loss_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                      int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                      void* hip_stream) {
  return grad_batch_device(kLambdaGrad, ctx, model_kind, param_space, d_theta, P, B, d_T_use, d_loss_out, d_grad_out,
                           hip_stream);
}

int yfm_lambda_loss_fullgrad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                                   const int* T_use, double* loss_out, double* grad_out) {
  return grad_batch(kLambdaFullGrad, ctx, model_kind, param_space, theta, P, B, T_use, loss_out, grad_out);
}

int yfm_lambda_loss_fullgrad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                          int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                          void* hip_stream) {
  return grad_batch_device(kLambdaFullGrad, ctx, model_kind, param_space, d_theta, P, B, d_T_use, d_loss_out,
                           d_grad_out, hip_stream);
}

int yfm_neural_loss_grad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                               const int* T_use, double* loss_out, double* grad_out) {
  return grad_batch(kNeuralGrad, ctx, model_kind, param_space, theta, P, B, T_use, loss_out, grad_out);
}

int yfm_neural_loss_grad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                      int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                      void* hip_stream) {
  return grad_batch_device(kNeuralGrad, ctx, model_kind, param_space, d_theta, P, B, d_T_use, d_loss_out, d_grad_out,
                           hip_stream);
}

int yfm_neural_loss_fullgrad_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                                   const int* T_use, double* loss_out, double* grad_out) {
  return grad_batch(kNeuralFullGrad, ctx, model_kind, param_space, theta, P, B, T_use, loss_out, grad_out);
}

int yfm_neural_loss_fullgrad_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                          int B, const int* d_T_use, double* d_loss_out, double* d_grad_out,
                                          void* hip_stream) {
  return grad_batch_device(kNeuralFullGrad, ctx, model_kind, param_space, d_theta, P, B, d_T_use, d_loss_out,
                           d_grad_out, hip_stream);
}

int yfm_last_batch_grad_unavailable(yfm_ctx* ctx, long long* n) {
  unsigned int h[yfm::kFlagsPerBank];
  if (int r = read_flags(ctx, h)) return r;
  if (n) *n = h[5];
  return YFM_OK;
}

int yfm_loglik_scores_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                            const int* T_use, double* loglik_out, double* scores_out) {
  return scores_batch(kDnsInfo, "yfm_loglik_scores_batch", ctx, model_kind, param_space, theta, P, B, T_use, loglik_out,
                      scores_out);
}

int yfm_loglik_scores_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                                   const int* d_T_use, double* d_loglik_out, double* d_scores_out, void* hip_stream) {
  return scores_batch_device(kDnsInfo, "yfm_loglik_scores_batch_device", ctx, model_kind, param_space, d_theta, P, B,
                             d_T_use, d_loglik_out, d_scores_out, hip_stream);
}

int yfm_loglik_info_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                          const int* T_use, int lags, double step, double* loglik_out, double* grad_out,
                          double* hess_out, double* opg_out) {
  return info_batch(kDnsInfo, "yfm_loglik_info_batch", ctx, model_kind, param_space, theta, P, B, T_use, lags, step,
                    loglik_out, grad_out, hess_out, opg_out);
}

int yfm_tvl_loglik_scores_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                                const int* T_use, double* loglik_out, double* scores_out) {
  return scores_batch(kTvlInfo, "yfm_tvl_loglik_scores_batch", ctx, model_kind, param_space, theta, P, B, T_use,
                      loglik_out, scores_out);
}

int yfm_tvl_loglik_scores_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P,
                                       int B, const int* d_T_use, double* d_loglik_out, double* d_scores_out,
                                       void* hip_stream) {
  return scores_batch_device(kTvlInfo, "yfm_tvl_loglik_scores_batch_device", ctx, model_kind, param_space, d_theta, P,
                             B, d_T_use, d_loglik_out, d_scores_out, hip_stream);
}

int yfm_tvl_loglik_info_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                              const int* T_use, int lags, double step, double* loglik_out, double* grad_out,
                              double* hess_out, double* opg_out) {
  return info_batch(kTvlInfo, "yfm_tvl_loglik_info_batch", ctx, model_kind, param_space, theta, P, B, T_use, lags, step,
                    loglik_out, grad_out, hess_out, opg_out);
}

int yfm_smooth_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                     const int* T_use, double* beta_s, double* V_s, double* C_s) {
  return smooth_batch(check_smooth, "yfm_smooth_batch", ctx, model_kind, param_space, theta, P, B, T_use, beta_s, V_s,
                      C_s);
}

int yfm_smooth_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                            const int* d_T_use, double* d_beta_s, double* d_V_s, double* d_C_s, void* hip_stream) {
  return smooth_batch_device(check_smooth, "yfm_smooth_batch_device", ctx, model_kind, param_space, d_theta, P, B,
                             d_T_use, d_beta_s, d_V_s, d_C_s, hip_stream);
}

int yfm_tvl_smooth_batch(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                         const int* T_use, double* beta_s, double* V_s, double* C_s) {
  return smooth_batch(check_tvl_smooth, "yfm_tvl_smooth_batch", ctx, model_kind, param_space, theta, P, B, T_use,
                      beta_s, V_s, C_s);
}

int yfm_tvl_smooth_batch_device(yfm_ctx* ctx, int model_kind, int param_space, const double* d_theta, int P, int B,
                                const int* d_T_use, double* d_beta_s, double* d_V_s, double* d_C_s, void* hip_stream) {
  return smooth_batch_device(check_tvl_smooth, "yfm_tvl_smooth_batch_device", ctx, model_kind, param_space, d_theta,
                             P, B, d_T_use, d_beta_s, d_V_s, d_C_s, hip_stream);
}

int yfm_filter_states(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                      const int* T_use, double* beta_out, double* P_out, double* loglik_out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, model_kind, param_space, P, B)) return r;
  if (yfm::msed_kind(model_kind))
    return set_error(YFM_EUNSUPPORTED, "yfm_filter_states is built for the Kalman kinds only: model_kind %d has no "
                     "covariance trajectory (use yfm_predict)", model_kind);
  if (B > 0 && (!theta || !beta_out || !P_out || !loglik_out)) return set_error(YFM_EINVAL, "null pointer argument");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  if (B == 0 || ctx->T < 2) {
    return yfm_loglik_batch(ctx, model_kind, param_space, theta, P, B, T_use, loglik_out);
  }
  const int M = state_dim(model_kind);
  const size_t steps = (size_t)(ctx->T - 1) * B;
  YFM_HIP_CHECK(ctx->rec_beta.ensure(sizeof(double) * steps * M));
  YFM_HIP_CHECK(ctx->rec_P.ensure(sizeof(double) * steps * M * M));
  YFM_HIP_CHECK(hipMemsetAsync(ctx->rec_beta.p, 0xff, sizeof(double) * steps * M, ctx->stream));  // NaN fill
  YFM_HIP_CHECK(hipMemsetAsync(ctx->rec_P.p, 0xff, sizeof(double) * steps * M * M, ctx->stream));
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  q.rec_beta = static_cast<double*>(ctx->rec_beta.p);
  q.rec_P = static_cast<double*>(ctx->rec_P.p);
  q.rec_len = ctx->T - 1;
  if (int r = launch(ctx, q)) return r;
  YFM_HIP_CHECK(hipMemcpyAsync(loglik_out, q.out, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipMemcpyAsync(beta_out, ctx->rec_beta.p, sizeof(double) * steps * M, hipMemcpyDeviceToHost,
                               ctx->stream));
  YFM_HIP_CHECK(hipMemcpyAsync(P_out, ctx->rec_P.p, sizeof(double) * steps * M * M, hipMemcpyDeviceToHost,
                               ctx->stream));
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

int yfm_last_batch_flags(yfm_ctx* ctx, long long* n_init_throw, long long* n_neg_inf) {
  unsigned int h[yfm::kFlagsPerBank];
  if (int r = read_flags(ctx, h)) return r;
  if (n_init_throw) *n_init_throw = h[0];
  if (n_neg_inf) *n_neg_inf = h[1];
  return YFM_OK;
}

int yfm_last_batch_deferred(yfm_ctx* ctx, long long* n_deferred) {
  unsigned int h[yfm::kFlagsPerBank];
  if (int r = read_flags(ctx, h)) return r;
  if (n_deferred) *n_deferred = h[3];
  return YFM_OK;
}

int yfm_last_batch_steady(yfm_ctx* ctx, long long* steady_wave_steps) {
  unsigned int h[yfm::kFlagsPerBank];
  if (int r = read_flags(ctx, h)) return r;
  if (steady_wave_steps) *steady_wave_steps = h[4];
  return YFM_OK;
}

int yfm_gamma_dim(int model_kind) { return gamma_dim(model_kind); }

int yfm_predict(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B, const int* T_use,
                int horizon, double* preds, double* factors, double* states, double* loadings_1,
                double* loadings_2) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, model_kind, param_space, P, B)) return r;
  if (horizon < 1) return set_error(YFM_EINVAL, "horizon = %d < 1", horizon);
  if (B > 0 && (!theta || !preds || !factors || !states)) return set_error(YFM_EINVAL, "null pointer argument");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  if (B == 0) return YFM_OK;
  const int M = state_dim(model_kind), L = gamma_dim(model_kind), N = ctx->N;
  const size_t ncol = (size_t)ctx->T + horizon - 1;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  q.horizon = horizon;
  // outputs: one device block [preds | load1 | load2 | factors | states]
  const size_t nN = (size_t)N * ncol * B, nM = (size_t)M * ncol * B, nL = (size_t)L * ncol * B;
  YFM_HIP_CHECK(ctx->rec_P.ensure(sizeof(double) * (3 * nN + nM + nL)));
  double* d = static_cast<double*>(ctx->rec_P.p);
  yfm::PredictArgs a{};
  a.preds = d;
  a.load1 = loadings_1 ? d + nN : nullptr;
  a.load2 = loadings_2 ? d + 2 * nN : nullptr;
  a.factors = d + 3 * nN;
  a.states = d + 3 * nN + nM;
  if (yfm::msed_kind(model_kind)) {
    if (int r = launch_record(ctx, q, 1, horizon, (int)ncol, a, sizeof(double) * (3 * nN + nM + nL))) return r;
  } else {
    q.rec_len = ctx->T + horizon;  // every step of the longest candidate
    if (int r = run_trajectory(ctx, q)) return r;
    a = predict_args(ctx, q, horizon, a);
    YFM_HIP_CHECK(yfm::launch_predict_emit(a));
  }
  YFM_HIP_CHECK(hipMemcpyAsync(preds, a.preds, sizeof(double) * nN, hipMemcpyDeviceToHost, ctx->stream));
  if (loadings_1)
    YFM_HIP_CHECK(hipMemcpyAsync(loadings_1, a.load1, sizeof(double) * nN, hipMemcpyDeviceToHost, ctx->stream));
  if (loadings_2)
    YFM_HIP_CHECK(hipMemcpyAsync(loadings_2, a.load2, sizeof(double) * nN, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipMemcpyAsync(factors, a.factors, sizeof(double) * nM, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipMemcpyAsync(states, a.states, sizeof(double) * nL, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

int yfm_forecast(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B, const int* T_use,
                 int horizon, double* out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, model_kind, param_space, P, B)) return r;
  if (horizon < 1) return set_error(YFM_EINVAL, "horizon = %d < 1", horizon);
  if (B > 0 && (!theta || !out)) return set_error(YFM_EINVAL, "null pointer argument");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  if (B == 0) return YFM_OK;
  const int M = state_dim(model_kind), L = gamma_dim(model_kind), N = ctx->N;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  q.horizon = horizon;
  const size_t n = (size_t)(M + L + N) * horizon * B;
  YFM_HIP_CHECK(ctx->rec_P.ensure(sizeof(double) * n));
  yfm::PredictArgs a{};
  a.preds = static_cast<double*>(ctx->rec_P.p);
  if (yfm::msed_kind(model_kind)) {
    if (int r = launch_record(ctx, q, 2, horizon, 0, a, sizeof(double) * n)) return r;
  } else {
    q.rec_len = horizon + 1;
    if (int r = run_trajectory(ctx, q)) return r;
    a = predict_args(ctx, q, horizon, a);
    YFM_HIP_CHECK(yfm::launch_forecast_emit(a));
  }
  YFM_HIP_CHECK(hipMemcpyAsync(out, a.preds, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

int yfm_loss_array(yfm_ctx* ctx, int model_kind, int param_space, const double* theta, int P, int B,
                   const int* T_use, int K, double* mse_out) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, model_kind, param_space, P, B)) return r;
  if (K < 1) return set_error(YFM_EINVAL, "K = %d < 1", K);
  if (K > 1 && T_use) return set_error(YFM_EUNSUPPORTED, "K > 1 passes with per-candidate windows");
  if (B > 0 && (!theta || !mse_out)) return set_error(YFM_EINVAL, "null pointer argument");
  if (int r = validate_tuse(T_use, B, ctx->T)) return r;
  const int T1 = ctx->T - 1;
  if (yfm::msed_kind(model_kind) && K > 1)
    return set_error(YFM_EUNSUPPORTED, "K = %d passes are not built for model_kind %d (K = 1 only)", K, model_kind);
  if (B == 0 || T1 <= 0) return YFM_OK;
  Launch q;
  if (int r = stage_inputs(ctx, model_kind, param_space, theta, P, B, T_use, q)) return r;
  if (yfm::msed_kind(model_kind)) {
    // get_loss_array of filter.jl:245-281: the λ kernel writes the rows itself (NaN beyond each window)
    const size_t nb = sizeof(double) * (size_t)T1 * B;
    YFM_HIP_CHECK(ctx->rec_P.ensure(nb));
    yfm::PredictArgs a{};
    a.preds = static_cast<double*>(ctx->rec_P.p);
    if (int r = launch_record(ctx, q, 3, 1, T1, a, nb)) return r;
    YFM_HIP_CHECK(hipMemcpyAsync(mse_out, a.preds, nb, hipMemcpyDeviceToHost, ctx->stream));
    YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return YFM_OK;
  }
  PanelView pv{static_cast<const double*>(ctx->raw.p), static_cast<const double*>(ctx->panel.p), ctx->T};
  if (K > 1) {
    // the K passes continue the filter state (filter.jl:221-242 never re-initialises):
    // filter the panel [Y[:, 1:T−1] × K, Y[:, T]] once
    const int Tk = K * T1 + 1;
    const size_t colb = sizeof(double) * ctx->N;
    YFM_HIP_CHECK(ctx->tiled_raw.ensure(colb * Tk));
    YFM_HIP_CHECK(ctx->tiled_panel.ensure(sizeof(double) * (size_t)ctx->ldp * Tk));
    char* dst = static_cast<char*>(ctx->tiled_raw.p);
    for (int k = 0; k < K; ++k)
      YFM_HIP_CHECK(hipMemcpyAsync(dst + colb * k * T1, ctx->raw.p, colb * T1, hipMemcpyDeviceToDevice, ctx->stream));
    YFM_HIP_CHECK(hipMemcpyAsync(dst + colb * K * T1, static_cast<char*>(ctx->raw.p) + colb * T1, colb,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    YFM_HIP_CHECK(yfm::launch_prep_panel(static_cast<const double*>(ctx->tiled_raw.p), ctx->N, Tk, ctx->np, ctx->ldp,
                                         static_cast<double*>(ctx->tiled_panel.p), ctx->stream));
    pv = PanelView{static_cast<const double*>(ctx->tiled_raw.p), static_cast<const double*>(ctx->tiled_panel.p), Tk};
  }
  q.rec_len = pv.T - 1;
  q.panel = &pv;
  if (int r = run_trajectory(ctx, q)) return r;
  unsigned int* cur = ctx->own.bank_ptr(ctx->own.bank);
  YFM_HIP_CHECK(hipMemsetAsync(cur, 0, 2 * sizeof(unsigned int), ctx->stream));
  YFM_HIP_CHECK(ctx->rec_P.ensure(sizeof(double) * (size_t)T1 * B));
  yfm::PredictArgs a{};
  a.preds = static_cast<double*>(ctx->rec_P.p);
  a = predict_args(ctx, q, 1, a);
  YFM_HIP_CHECK(yfm::launch_loss_array(a, static_cast<const double*>(ctx->raw.p), T1, K, cur));
  YFM_HIP_CHECK(hipMemcpyAsync(mse_out, a.preds, sizeof(double) * (size_t)T1 * B, hipMemcpyDeviceToHost, ctx->stream));
  YFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return YFM_OK;
}

}  // extern "C"

namespace yfm {

Workspace* workspace_create() {
  auto* w = new Workspace;
  if (w->init() != hipSuccess) {
    delete w;
    return nullptr;
  }
  return w;
}

void workspace_destroy(Workspace* w) { delete w; }

int loglik_device_ws(yfm_ctx* ctx, Workspace* ws, int kind, int space, const double* d_theta, int P, int B,
                     const int* d_T_use, double* d_out, hipStream_t s, int share) {
  if (int r = check_ctx(ctx)) return r;
  if (int r = check_batch(ctx, kind, space, P, B)) return r;
  Launch q = loglik_launch(kind, space, d_theta, P, B, d_T_use, d_out, s);
  q.share = share > 1 ? share : 1;
  return launch(ctx, q, ws);
}

}  // namespace yfm
