// yfm_msed.hip — batched loss, its δ/Φ gradient, its full gradient, per-step loss array, predict and forecast of the static and
// score-driven λ Nelson–Siegel models (NS, SD-NS, RWSD-NS, SSD-NS, SRWSD-NS) for gfx950.  FP64.
//
// Restates, per candidate θ_b (the algebra is in yfm_msed.hpp, which names the model files):
//   get_loss         src/models/filter.jl:209-243
//   get_loss_array   src/models/filter.jl:245-281
//   predict          src/models/filter.jl:284-306
//   forecast blocks  src/forecasting.jl:236-250
//   filter           src/models/filter.jl:52-110
//
// Mapping, the one of yfm_tvl.hip for the same reason — the loadings are recomputed every
// step, so a step is O(N): ONE CANDIDATE PER GROUP OF L LANES, lane j owns the maturities i ≡ j (mod L), the
// statistics are reduced over the group with DPP butterflies (no LDS reduction) and every lane of the group
// runs the same 3×3 work, so the state stays replicated in VGPRs.  L ∈ {4, 16} is chosen per launch from B (one
// candidate per lane was built and dropped: its part of the tree below holds five sets of statistics and spilled).
//
// A candidate's value does not depend on L: the sums are formed over 16 residue classes of the maturity
// index (class c holds i ≡ c mod 16, added in order of i) combined by one fixed tree — class bit 3 first,
// bit 0 last.  A lane forms the part of the tree over its own classes in registers and the group finishes
// it with true xor exchanges in descending order.
//
// One pass per loading evaluation: the first pass of step t, at the loadings step t − 1 predicted with, also
// forms ‖y_t − ŷ_t‖² of get_loss against that prediction (and, in record mode, writes the prediction and the
// loading columns of step t − 1); the second pass, at the updated γ, serves the second OLS.  The static model
// has only the first; the two scaled kinds add a refinement pass at the first loadings (yfm_msed.hpp).
//
// Panel: the caller's raw N×T column-major matrix, staged as yfm_tvl.hip stages it (TC columns in LDS, the
// next chunk prefetched into registers).  The missing-data test is the reference's isnan(y[1]) on the raw
// column, not the prepared panel's any-NaN flag.
#pragma clang fp contract(off)
#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_msed.hpp"
#include "yfm_msed_pass.hpp"

namespace yfm {

namespace {

using namespace msedtree;  // the mapping's constants and the summation tree (yfm_msed_tree.hpp)
using namespace msedpass;  // the staging, the epilogue and the host dispatch (yfm_msed_pass.hpp)

using namespace msed;

// the statistics of one pass
template <bool SCORE>
struct Stats {
  double o[NOLS];
  double d[SCORE ? NSCORE : 1];
  double vv;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < NOLS; ++k) o[k] = 0.0;
#pragma unroll
    for (int k = 0; k < (SCORE ? NSCORE : 1); ++k) d[k] = 0.0;
    vv = 0.0;
  }
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
#pragma unroll
    for (int k = 0; k < NOLS; ++k) o[k] = f(o[k]);
    if constexpr (SCORE) {
#pragma unroll
      for (int k = 0; k < NSCORE; ++k) d[k] = f(d[k]);
    }
    vv = f(vv);
  }
  __device__ __forceinline__ void add(const Stats& a, const Stats& b) {
#pragma unroll
    for (int k = 0; k < NOLS; ++k) o[k] = a.o[k] + b.o[k];
    if constexpr (SCORE) {
#pragma unroll
      for (int k = 0; k < NSCORE; ++k) d[k] = a.d[k] + b.d[k];
    } else {
      d[0] = 0.0;
    }
    vv = a.vv + b.vv;
  }
};

// the statistics of the scaled kinds' refinement pass
struct Refine {
  double r[NREFINE];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < NREFINE; ++k) r[k] = 0.0;
  }
  __device__ __forceinline__ void add(const Refine& a, const Refine& b) {
#pragma unroll
    for (int k = 0; k < NREFINE; ++k) r[k] = a.r[k] + b.r[k];
  }
};

struct MsedOut {
  int mode;          // 0 loss, 1 predict, 2 forecast blocks, 3 loss array
  int horizon;       // predict / forecast: NaN-padding columns + 1
  int ncol;          // predict: columns per candidate (T + horizon − 1); loss array: T − 1
  double* preds;     // predict: N×ncol×B; forecast: (4 + N)×h×B; loss array: ncol×B
  double* factors;   // predict: 3×ncol×B
  double* states;    // predict: 1×ncol×B
  double* load1;     // predict: N×ncol×B or nullptr
  double* load2;
};

template <int L, bool STATIC, bool HASB, bool SCALED, bool RECORD>
__global__ __launch_bounds__(kMsedBlock) void msed_kernel(const double* __restrict__ theta, int P, int B, int space,
                                                           const double* __restrict__ Y, int T, int N, int TC,
                                                           const double* __restrict__ mats,
                                                           const int* __restrict__ T_use, double* __restrict__ out,
                                                           unsigned int* __restrict__ flags,
                                                           unsigned int* __restrict__ flags_next, MsedOut ro) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int KQ = log_classes_per_lane<L>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double2* s_mr = reinterpret_cast<double2*>(smem);  // (m_i, 1/m_i)
  double* s_y = smem + 2 * N;                         // TC columns of N yields
  __shared__ int s_iters_max;

  const int tid = threadIdx.x;
  if (flags_next && blockIdx.x == 0 && tid < kFlagsPerBank) flags_next[tid] = 0u;  // the next launch's counters
  const int j = tid % L;
  const int grp = tid / L;
  const int b = blockIdx.x * GPB + grp;
  const bool live = b < B;
  const int bb = live ? b : (B - 1);
  const int nobs = T_use ? T_use[bb] : T;

  if (tid == 0) s_iters_max = 0;
  for (int i = tid; i < N; i += kMsedBlock) {
    const double m = mats[i];
    s_mr[i] = make_double2(m, 1.0 / m);
  }
  __syncthreads();
  // steps: the filter calls; iteration t runs the first pass on column t — the comparison and the outputs of
  // step t − 1 — and then step t, so there is one iteration more than steps
  const bool traj = RECORD && (ro.mode == 1 || ro.mode == 2);
  const int my_steps = traj ? nobs + ro.horizon - 1 : nobs - 1;
  const int my_iters = my_steps + 1;
  atomicMax(&s_iters_max, live ? my_iters : 0);

  Model mdl;
  State st;
  decode<STATIC, HASB>(theta + (size_t)bb * P, space, mdl);
  init_state(mdl, st);
  const double fN = (double)N;

  double mse = 0.0;
  bool fail = false;       // get_loss / get_loss_array return −Inf
  bool pred_fail = false;  // the last step returned −Inf instead of a prediction

  __syncthreads();
  const int niter = s_iters_max;
  const int CHY = TC * N;

  // ---- panel staging: chunk c (columns cTC .. cTC+TC−1) in LDS, chunk c+1 in registers (yfm_msed_pass.hpp, which
  // says why the two lambdas stay) ----
  double pre[kMsedPre];
  auto load_chunk = [&](int c) { chunk_load(Y, c, CHY, T, N, tid, pre); };
  auto store_chunk = [&]() { chunk_store(s_y, CHY, tid, pre); };
  if (niter > 0) {
    load_chunk(0);
    store_chunk();
    __syncthreads();
    load_chunk(1);
  }

  for (int t = 0; t < niter; ++t) {
    const int tt = t % TC;
    const bool act = live && t < my_iters;
    if (act) {
      const double* col = s_y + tt * N;
      const bool has_col = t < nobs;                     // a data column (the rest is the NaN padding)
      const bool compare = !traj && t >= 1;              // y_t against the prediction of step t − 1 (t < nobs here)
      const bool emit = traj && t >= 1;                  // outputs of step t − 1
      // where the per-maturity outputs of step t − 1 go
      double *e_pred = nullptr, *e_l1 = nullptr, *e_l2 = nullptr;
      if constexpr (RECORD) {
        if (emit && ro.mode == 1) {
          const size_t o = ((size_t)b * ro.ncol + (t - 1)) * N;
          e_pred = ro.preds + o;
          e_l1 = ro.load1 ? ro.load1 + o : nullptr;
          e_l2 = ro.load2 ? ro.load2 + o : nullptr;
        } else if (emit && ro.mode == 2) {
          const int k = (t - 1) - (nobs - 1);
          if (k >= 0) e_pred = ro.preds + ((size_t)b * ro.horizon + k) * (4 + N) + 4;
        }
      }
      // ---- first pass: the loadings at γ ----
      const Lambda la = make_lambda(st.gamma);
      const double ninf = -__builtin_inf();
      Stats<!STATIC> sa;
      auto leaf_a = [&](int c, Stats<!STATIC>& s) {
        s.zero();
        for (int i = c; i < N; i += kMsedClasses) {
          const double2 mr = s_mr[i];
          double z, z2, z3;
          loadings(la, mr.x, mr.y, z, z2, z3);
          const double y = has_col ? col[i] : 0.0;
          accum_ols(s.o, z2, z3, y);
          if constexpr (!STATIC) {
            double d2, d3;
            dloadings(la, mr.x, z, z2, d2, d3);
            accum_score(s.d, z2, z3, d2, d3, y);
          }
          const double pr = fitted(st.beta, z2, z3);
          const double v = y - pr;
          s.vv = mfma(v, v, s.vv);
          if constexpr (RECORD) {
            if (e_pred) e_pred[i] = pred_fail ? ninf : pr;
            if (e_l1) e_l1[i] = z2;
            if (e_l2) e_l2[i] = z3;
          }
        }
      };
      class_tree<KQ>(j, leaf_a, sa);
      sa.each([](double x) { return group_sum_desc<L>(x); });

      if (compare) {
        // v = y_t − ŷ_t; mse −= v'v; a non-finite running sum returns −Inf (filter.jl:226-234, :263-270)
        const double step = pred_fail ? ninf : -sa.vv;
        mse += step;
        fail = fail || !(fabs(mse) <= __DBL_MAX__);
        if constexpr (RECORD) {
          if (ro.mode == 3) {
            fail = fail || !(fabs(step) <= __DBL_MAX__);
            if (j == 0) ro.preds[(size_t)b * ro.ncol + (t - 1)] = step / fN;
          }
        }
      }

      if (t < my_steps) {
        // ---- step t (filter.jl:52-110) ----
        const bool y0nan = !has_col || (col[0] != col[0]);
        pred_fail = false;
        if (y0nan) {
          advance<HASB>(mdl, st);
        } else if (bool ridged = false; !ols(sa.o, fN, st.beta, ridged)) {
          pred_fail = true;
        } else {
          bool ok = true;
          if constexpr (!STATIC) {
            double g;
            if constexpr (SCALED) {
              // ---- refinement pass (yfm_msed.hpp): the residual at β with its rounding errors carried ----
              Refine sr;
              auto leaf_r = [&](int c, Refine& s) {
                s.zero();
                for (int i = c; i < N; i += kMsedClasses) {
                  const double2 mr = s_mr[i];
                  double z, z2, z3, d2, d3;
                  loadings(la, mr.x, mr.y, z, z2, z3);
                  dloadings(la, mr.x, z, z2, d2, d3);
                  accum_refine(s.r, st.beta, z2, z3, d2, d3, col[i]);
                }
              };
              class_tree<KQ>(j, leaf_r, sr);
#pragma unroll
              for (int k = 0; k < NREFINE; ++k) sr.r[k] = group_sum_desc<L>(sr.r[k]);
              g = score_refined(sa.o, fN, ridged, sa.d, sr.r, st.beta);
            } else {
              g = score(sa.d, st.beta);
            }
            update_gamma<SCALED>(mdl, st, g);
            // ---- second pass: the loadings at the updated γ ----
            const Lambda lb = make_lambda(st.gamma);
            Stats<false> sb;
            auto leaf_b = [&](int c, Stats<false>& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) {
                const double2 mr = s_mr[i];
                double z, z2, z3;
                loadings(lb, mr.x, mr.y, z, z2, z3);
                accum_ols(s.o, z2, z3, col[i]);
              }
            };
            class_tree<KQ>(j, leaf_b, sb);
#pragma unroll
            for (int k = 0; k < NOLS; ++k) sb.o[k] = group_sum_desc<L>(sb.o[k]);
            ok = ols(sb.o, fN, st.beta);
          }
          if (ok) {
            advance<HASB>(mdl, st);
          } else {
            pred_fail = true;
          }
        }
        if constexpr (RECORD) {
          // factors and states of column t: β and γ after the step (filter.jl:299-300)
          if (j == 0 && ro.mode == 1) {
            const size_t o = (size_t)b * ro.ncol + t;
#pragma unroll
            for (int k = 0; k < kM; ++k) ro.factors[o * kM + k] = st.beta[k];
            ro.states[o] = st.gamma;
          } else if (j == 0 && ro.mode == 2) {
            const int k = t - (nobs - 1);
            if (k >= 0) {
              double* o = ro.preds + ((size_t)b * ro.horizon + k) * (4 + N);
#pragma unroll
              for (int q = 0; q < kM; ++q) o[q] = st.beta[q];
              o[kM] = st.gamma;
            }
          }
        }
      }
    }
    if (tt == TC - 1) {  // chunk done: its buffer takes the prefetched chunk, prefetch the one after
      __syncthreads();
      store_chunk();
      __syncthreads();
      load_chunk(t / TC + 2);
    }
  }

  if (!live) return;
  if constexpr (RECORD) {
    if (ro.mode == 3) {
      // a non-finite entry makes get_loss_array return the scalar −Inf (filter.jl:268-270): the whole row
      if (fail) {
        for (int k = j; k < nobs - 1; k += L) ro.preds[(size_t)b * ro.ncol + k] = -__builtin_inf();
        if (j == 0) atomicAdd(&flags[1], 1u);
      }
      return;
    }
    if (traj) return;
  }
  if (j != 0) return;
  out[b] = finish_loss(mse, fN, nobs, fail, flags);
}

// The first pass's statistics with Z'v of the comparison (yfm_msed.hpp, ∂loss/∂(δ, Φ)) through the same tree.
template <bool SCORE>
struct GradStats {
  Stats<SCORE> s;
  double zv[kM];
  __device__ __forceinline__ void zero() {
    s.zero();
#pragma unroll
    for (int k = 0; k < kM; ++k) zv[k] = 0.0;
  }
  __device__ __forceinline__ void add(const GradStats& a, const GradStats& b) {
    s.add(a.s, b.s);
#pragma unroll
    for (int k = 0; k < kM; ++k) zv[k] = a.zv[k] + b.zv[k];
  }
};

// get_loss and its gradient with respect to δ and Φ in one pass: msed_kernel's loss mode — the same mapping,
// staging, passes and sums, so the loss is the same bits — whose comparison also forms s = Z'v, from which every
// lane of the group updates the 12 accumulators (replicated like the state: DESIGN.md §3.6).  Writes the loss to
// out[b] and the gradient, in the caller's space, to grad[12·b ..]; NaN where the loss is −Inf.
template <int L, bool STATIC, bool HASB, bool SCALED>
__global__ __launch_bounds__(kMsedBlock) void lambda_grad_kernel(const double* __restrict__ theta, int P, int B,
                                                                  int space, const double* __restrict__ Y, int T,
                                                                  int N, int TC, const double* __restrict__ mats,
                                                                  const int* __restrict__ T_use,
                                                                  double* __restrict__ out, double* __restrict__ grad,
                                                                  unsigned int* __restrict__ flags,
                                                                  unsigned int* __restrict__ flags_next) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int KQ = log_classes_per_lane<L>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double2* s_mr = reinterpret_cast<double2*>(smem);  // (m_i, 1/m_i)
  double* s_y = smem + 2 * N;                         // TC columns of N yields
  __shared__ int s_iters_max;

  const int tid = threadIdx.x;
  if (flags_next && blockIdx.x == 0 && tid < kFlagsPerBank) flags_next[tid] = 0u;  // the next launch's counters
  const int j = tid % L;
  const int grp = tid / L;
  const int b = blockIdx.x * GPB + grp;
  const bool live = b < B;
  const int bb = live ? b : (B - 1);
  const int nobs = T_use ? T_use[bb] : T;

  if (tid == 0) s_iters_max = 0;
  for (int i = tid; i < N; i += kMsedBlock) {
    const double m = mats[i];
    s_mr[i] = make_double2(m, 1.0 / m);
  }
  __syncthreads();
  const int my_steps = nobs - 1;
  const int my_iters = my_steps + 1;  // iteration t: the comparison of step t − 1, then step t
  atomicMax(&s_iters_max, live ? my_iters : 0);

  const double* th = theta + (size_t)bb * P;
  Model mdl;
  State st;
  decode<STATIC, HASB>(th, space, mdl);
  init_state(mdl, st);
  const double fN = (double)N;

  double mse = 0.0;
  bool fail = false;
  bool pred_fail = false;
  Grad g;
  grad_zero(g);
  double bpost[kM] = {0.0, 0.0, 0.0};  // the β step t − 1 predicted from
  bool pred_only = false;              // step t − 1 was prediction-only

  __syncthreads();
  const int niter = s_iters_max;
  const int CHY = TC * N;

  // ---- panel staging, as msed_kernel ----
  double pre[kMsedPre];
  auto load_chunk = [&](int c) { chunk_load(Y, c, CHY, T, N, tid, pre); };
  auto store_chunk = [&]() { chunk_store(s_y, CHY, tid, pre); };
  if (niter > 0) {
    load_chunk(0);
    store_chunk();
    __syncthreads();
    load_chunk(1);
  }

  for (int t = 0; t < niter; ++t) {
    const int tt = t % TC;
    const bool act = live && t < my_iters;
    if (act) {
      const double* col = s_y + tt * N;  // t < nobs: always a data column here
      // ---- first pass: the loadings at γ ----
      const Lambda la = make_lambda(st.gamma);
      GradStats<!STATIC> sa;
      auto leaf_a = [&](int c, GradStats<!STATIC>& s) {
        s.zero();
        for (int i = c; i < N; i += kMsedClasses) {
          const double2 mr = s_mr[i];
          double z, z2, z3;
          loadings(la, mr.x, mr.y, z, z2, z3);
          const double y = col[i];
          accum_ols(s.s.o, z2, z3, y);
          if constexpr (!STATIC) {
            double d2, d3;
            dloadings(la, mr.x, z, z2, d2, d3);
            accum_score(s.s.d, z2, z3, d2, d3, y);
          }
          const double v = y - fitted(st.beta, z2, z3);
          s.s.vv = mfma(v, v, s.s.vv);
          accum_zv(s.zv, z2, z3, v);
        }
      };
      class_tree<KQ>(j, leaf_a, sa);
      sa.s.each([](double x) { return group_sum_desc<L>(x); });
#pragma unroll
      for (int k = 0; k < kM; ++k) sa.zv[k] = group_sum_desc<L>(sa.zv[k]);

      if (t >= 1) {
        // v = y_t − ŷ_t; mse −= v'v; a non-finite running sum returns −Inf (filter.jl:226-234)
        mse += pred_fail ? -__builtin_inf() : -sa.s.vv;
        fail = fail || !(fabs(mse) <= __DBL_MAX__);
        grad_accum(mdl, pred_only, sa.zv, bpost, g);
      }

      if (t < my_steps) {
        // ---- step t (filter.jl:52-110), as msed_kernel ----
        pred_only = col[0] != col[0];
        pred_fail = false;
        if (pred_only) {
          advance<HASB>(mdl, st);
        } else if (bool ridged = false; !ols(sa.s.o, fN, st.beta, ridged)) {
          pred_fail = true;
        } else {
          bool ok = true;
          if constexpr (!STATIC) {
            double sc;
            if constexpr (SCALED) {
              Refine sr;
              auto leaf_r = [&](int c, Refine& s) {
                s.zero();
                for (int i = c; i < N; i += kMsedClasses) {
                  const double2 mr = s_mr[i];
                  double z, z2, z3, d2, d3;
                  loadings(la, mr.x, mr.y, z, z2, z3);
                  dloadings(la, mr.x, z, z2, d2, d3);
                  accum_refine(s.r, st.beta, z2, z3, d2, d3, col[i]);
                }
              };
              class_tree<KQ>(j, leaf_r, sr);
#pragma unroll
              for (int k = 0; k < NREFINE; ++k) sr.r[k] = group_sum_desc<L>(sr.r[k]);
              sc = score_refined(sa.s.o, fN, ridged, sa.s.d, sr.r, st.beta);
            } else {
              sc = score(sa.s.d, st.beta);
            }
            update_gamma<SCALED>(mdl, st, sc);
            // ---- second pass: the loadings at the updated γ ----
            const Lambda lb = make_lambda(st.gamma);
            Stats<false> sb;
            auto leaf_b = [&](int c, Stats<false>& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) {
                const double2 mr = s_mr[i];
                double z, z2, z3;
                loadings(lb, mr.x, mr.y, z, z2, z3);
                accum_ols(s.o, z2, z3, col[i]);
              }
            };
            class_tree<KQ>(j, leaf_b, sb);
#pragma unroll
            for (int k = 0; k < NOLS; ++k) sb.o[k] = group_sum_desc<L>(sb.o[k]);
            ok = ols(sb.o, fN, st.beta);
          }
          if (ok) {
#pragma unroll
            for (int k = 0; k < kM; ++k) bpost[k] = st.beta[k];
            advance<HASB>(mdl, st);
          } else {
            pred_fail = true;
          }
        }
      }
    }
    if (tt == TC - 1) {  // chunk done: its buffer takes the prefetched chunk, prefetch the one after
      __syncthreads();
      store_chunk();
      __syncthreads();
      load_chunk(t / TC + 2);
    }
  }

  if (!live || j != 0) return;
  out[b] = finish_loss(mse, fN, nobs, fail, flags);
  double go[kGrad];
  grad_finish(g, th, P, space, fN, nobs, fail, go);
#pragma unroll
  for (int k = 0; k < kGrad; ++k) grad[(size_t)b * kGrad + k] = go[k];
}

// The statistics of the full gradient's first pass: the δ/Φ gradient's (the same sums through the same tree, the
// score's contractions formed for NS too), D'v of the comparison and the contractions of g' (yfm_msed.hpp accum_tan).
template <bool STATIC>
struct FullStats {
  GradStats<true> g;
  double dv[2];
  double t[STATIC ? 1 : NTAN];
  __device__ __forceinline__ void zero() {
    g.zero();
    dv[0] = dv[1] = 0.0;
#pragma unroll
    for (int k = 0; k < (STATIC ? 1 : NTAN); ++k) t[k] = 0.0;
  }
  __device__ __forceinline__ void add(const FullStats& a, const FullStats& b) {
    g.add(a.g, b.g);
    dv[0] = a.dv[0] + b.dv[0];
    dv[1] = a.dv[1] + b.dv[1];
#pragma unroll
    for (int k = 0; k < (STATIC ? 1 : NTAN); ++k) t[k] = a.t[k] + b.t[k];
  }
};

// the second pass's: the OLS sums and the score's contractions at γ⁺ (β'(γ⁺) needs them)
struct PassB {
  double o[NOLS];
  double d[NSCORE];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < NOLS; ++k) o[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NSCORE; ++k) d[k] = 0.0;
  }
  __device__ __forceinline__ void add(const PassB& a, const PassB& b) {
#pragma unroll
    for (int k = 0; k < NOLS; ++k) o[k] = a.o[k] + b.o[k];
#pragma unroll
    for (int k = 0; k < NSCORE; ++k) d[k] = a.d[k] + b.d[k];
  }
};

// what a candidate of the full-gradient kernel keeps in LDS
template <int K>
struct FullRec {
  Grad g;
  Tangent<K> tn;
  double bpost[kM];
};

// get_loss and its gradient with respect to every row of θ in one pass: lambda_grad_kernel — the same mapping,
// staging, passes, tree and sums, so the loss and the last 12 rows are the same bits — with the tangents of the score
// recursion (yfm_msed.hpp) replicated on every lane of the group like the state.  Writes the loss to
// out[b] and the gradient, in the caller's space, to grad[P·b ..]; NaN in all P rows where the loss is −Inf, and where
// a tangent or a leading accumulator is not finite (counted in flags[5]).
template <int L, bool STATIC, bool HASB, bool SCALED>
__global__ __launch_bounds__(kMsedBlock) void lambda_fullgrad_kernel(const double* __restrict__ theta, int P, int B,
                                                                      int space, const double* __restrict__ Y, int T,
                                                                      int N, int TC, const double* __restrict__ mats,
                                                                      const int* __restrict__ T_use,
                                                                      double* __restrict__ out,
                                                                      double* __restrict__ grad,
                                                                      unsigned int* __restrict__ flags,
                                                                      unsigned int* __restrict__ flags_next) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int KQ = log_classes_per_lane<L>();
  constexpr int K = lead_count<STATIC, HASB>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double2* s_mr = reinterpret_cast<double2*>(smem);  // (m_i, 1/m_i)
  double* s_y = smem + 2 * N;                         // TC columns of N yields
  __shared__ int s_iters_max;
  // the candidate's record: what is touched once per step — the 12 δ/Φ accumulators, the tangents with the leading
  // accumulators and β_post — lives in LDS, not in registers.  Every lane of the group computes the
  // same values and writes them to the same words; a group is part of one wave, so its lanes read and write in step.
  __shared__ FullRec<K> s_rec[GPB];

  const int tid = threadIdx.x;
  if (flags_next && blockIdx.x == 0 && tid < kFlagsPerBank) flags_next[tid] = 0u;  // the next launch's counters
  const int j = tid % L;
  const int grp = tid / L;
  const int b = blockIdx.x * GPB + grp;
  const bool live = b < B;
  const int bb = live ? b : (B - 1);
  const int nobs = T_use ? T_use[bb] : T;

  if (tid == 0) s_iters_max = 0;
  for (int i = tid; i < N; i += kMsedBlock) {
    const double m = mats[i];
    s_mr[i] = make_double2(m, 1.0 / m);
  }
  __syncthreads();
  const int my_steps = nobs - 1;
  const int my_iters = my_steps + 1;  // iteration t: the comparison of step t − 1, then step t
  atomicMax(&s_iters_max, live ? my_iters : 0);

  const double* th = theta + (size_t)bb * P;
  Model mdl;
  State st;
  decode<STATIC, HASB>(th, space, mdl);
  init_state(mdl, st);
  const double fN = (double)N;

  double mse = 0.0;
  bool fail = false;
  bool pred_fail = false;
  Grad& g = s_rec[grp].g;
  Tangent<K>& tn = s_rec[grp].tn;
  double(&bpost)[kM] = s_rec[grp].bpost;  // the β step t − 1 predicted from
  grad_zero(g);
  tangent_init(tn);
#pragma unroll
  for (int k = 0; k < kM; ++k) bpost[k] = 0.0;
  bool pred_only = false;              // step t − 1 was prediction-only

  __syncthreads();
  const int niter = s_iters_max;
  const int CHY = TC * N;

  // ---- panel staging, as msed_kernel ----
  double pre[kMsedPre];
  auto load_chunk = [&](int c) { chunk_load(Y, c, CHY, T, N, tid, pre); };
  auto store_chunk = [&]() { chunk_store(s_y, CHY, tid, pre); };
  if (niter > 0) {
    load_chunk(0);
    store_chunk();
    __syncthreads();
    load_chunk(1);
  }

  for (int t = 0; t < niter; ++t) {
    const int tt = t % TC;
    const bool act = live && t < my_iters;
    if (act) {
      const double* col = s_y + tt * N;  // t < nobs: always a data column here
      // ---- first pass: the loadings at γ ----
      const Lambda la = make_lambda(st.gamma);
      FullStats<STATIC> sa;
      auto leaf_a = [&](int c, FullStats<STATIC>& s) {
        s.zero();
        for (int i = c; i < N; i += kMsedClasses) {
          const double2 mr = s_mr[i];
          double z, z2, z3, d2, d3;
          loadings(la, mr.x, mr.y, z, z2, z3);
          const double y = col[i];
          accum_ols(s.g.s.o, z2, z3, y);
          dloadings(la, mr.x, z, z2, d2, d3);
          accum_score(s.g.s.d, z2, z3, d2, d3, y);
          const double v = y - fitted(st.beta, z2, z3);
          s.g.s.vv = mfma(v, v, s.g.s.vv);
          accum_zv(s.g.zv, z2, z3, v);
          accum_dv(s.dv, d2, d3, v);
          if constexpr (!STATIC) {
            double e2, e3;
            d2loadings(la, mr.x, z, z2, e2, e3);
            accum_tan(s.t, z2, z3, d2, d3, e2, e3, y);
          }
        }
      };
      class_tree<KQ>(j, leaf_a, sa);
      sa.g.s.each([](double x) { return group_sum_desc<L>(x); });
#pragma unroll
      for (int k = 0; k < kM; ++k) sa.g.zv[k] = group_sum_desc<L>(sa.g.zv[k]);
      sa.dv[0] = group_sum_desc<L>(sa.dv[0]);
      sa.dv[1] = group_sum_desc<L>(sa.dv[1]);
      if constexpr (!STATIC) {
#pragma unroll
        for (int k = 0; k < NTAN; ++k) sa.t[k] = group_sum_desc<L>(sa.t[k]);
      }

      if (t >= 1) {
        // v = y_t − ŷ_t; mse −= v'v; a non-finite running sum returns −Inf (filter.jl:226-234)
        mse += pred_fail ? -__builtin_inf() : -sa.g.s.vv;
        fail = fail || !(fabs(mse) <= __DBL_MAX__);
        grad_accum(mdl, pred_only, sa.g.zv, bpost, g);
        lead_accum(sa.g.zv, sa.dv, st.beta, tn);
      }

      if (t < my_steps) {
        // ---- step t (filter.jl:52-110), as msed_kernel, with the tangents (yfm_msed.hpp filter_step_tangent) ----
        pred_only = col[0] != col[0];
        pred_fail = false;
        if (pred_only) {
          advance_tangent_pred_only<HASB>(mdl, st.gamma, tn);
          advance<HASB>(mdl, st);
        } else if (bool ridged = false; !ols(sa.g.s.o, fN, st.beta, ridged)) {
          pred_fail = true;
        } else {
          bool ok = true;
          double bp[kM] = {0.0, 0.0, 0.0}, dv[2];
          ols_tangent(sa.g.s.o, fN, ridged, sa.g.s.d, st.beta, bp, dv);
          if constexpr (!STATIC) {
            double sc;
            if constexpr (SCALED) {
              Refine sr;
              auto leaf_r = [&](int c, Refine& s) {
                s.zero();
                for (int i = c; i < N; i += kMsedClasses) {
                  const double2 mr = s_mr[i];
                  double z, z2, z3, d2, d3;
                  loadings(la, mr.x, mr.y, z, z2, z3);
                  dloadings(la, mr.x, z, z2, d2, d3);
                  accum_refine(s.r, st.beta, z2, z3, d2, d3, col[i]);
                }
              };
              class_tree<KQ>(j, leaf_r, sr);
#pragma unroll
              for (int k = 0; k < NREFINE; ++k) sr.r[k] = group_sum_desc<L>(sr.r[k]);
              sc = score_refined(sa.g.s.o, fN, ridged, sa.g.s.d, sr.r, st.beta);
            } else {
              sc = score(sa.g.s.d, st.beta);
            }
            const double gprime = score_tangent(sa.g.s.d, sa.t, st.beta, bp, dv);
            update_gamma<SCALED>(mdl, st, sc);
            update_gamma_tangent<SCALED>(mdl, st, sc, gprime, tn);
            // ---- second pass: the loadings at the updated γ ----
            const Lambda lb = make_lambda(st.gamma);
            PassB sb;
            auto leaf_b = [&](int c, PassB& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) {
                const double2 mr = s_mr[i];
                double z, z2, z3, d2, d3;
                loadings(lb, mr.x, mr.y, z, z2, z3);
                const double y = col[i];
                accum_ols(s.o, z2, z3, y);
                dloadings(lb, mr.x, z, z2, d2, d3);
                accum_score(s.d, z2, z3, d2, d3, y);
              }
            };
            class_tree<KQ>(j, leaf_b, sb);
#pragma unroll
            for (int k = 0; k < NOLS; ++k) sb.o[k] = group_sum_desc<L>(sb.o[k]);
#pragma unroll
            for (int k = 0; k < NSCORE; ++k) sb.d[k] = group_sum_desc<L>(sb.d[k]);
            ok = ols(sb.o, fN, st.beta, ridged);
            if (ok) ols_tangent(sb.o, fN, ridged, sb.d, st.beta, bp, dv);
          }
          if (ok) {
#pragma unroll
            for (int k = 0; k < kM; ++k) bpost[k] = st.beta[k];
            advance_tangent<HASB>(mdl, st.gamma, bp, tn);
            advance<HASB>(mdl, st);
          } else {
            pred_fail = true;
          }
        }
      }
    }
    if (tt == TC - 1) {  // chunk done: its buffer takes the prefetched chunk, prefetch the one after
      __syncthreads();
      store_chunk();
      __syncthreads();
      load_chunk(t / TC + 2);
    }
  }

  if (!live || j != 0) return;
  out[b] = finish_loss(mse, fN, nobs, fail, flags);
  double go[K + kGrad];
  if (fullgrad_finish<STATIC, HASB>(mdl, tn, g, th, P, space, fN, nobs, fail, go)) atomicAdd(&flags[5], 1u);
#pragma unroll
  for (int k = 0; k < K + kGrad; ++k) grad[(size_t)b * (K + kGrad) + k] = go[k];
}

// ---- host dispatch: one table over the kinds and one launch shape for the three kernels ----
// f(Variant<L, STATIC, HASB, SCALED>) for a λ kind
template <int L, class F>
hipError_t with_kind(int kind, F&& f) {
  switch (kind) {
    case YFM_MODEL_NS: return f(Variant<L, true, false, false>{});
    case YFM_MODEL_SD_NS: return f(Variant<L, false, true, false>{});
    case YFM_MODEL_RWSD_NS: return f(Variant<L, false, false, false>{});
    case YFM_MODEL_SSD_NS: return f(Variant<L, false, true, true>{});
    case YFM_MODEL_SRWSD_NS: return f(Variant<L, false, false, true>{});
  }
  return hipErrorInvalidValue;
}

// launch(Variant, grid, shared-memory bytes, TC) starts the kernel of a kind at a lane count on a's batch and panel
template <class F>
hipError_t launch_with(int kind, const LaunchArgs& a, int lanes, F&& launch) {
  const int TC = chunk_columns(a.N);
  if (TC < 1) return hipErrorInvalidValue;
  const size_t shmem = sizeof(double) * (size_t)(2 * a.N + TC * a.N);
  return with_lanes(lanes, [&](auto ln) {
    return with_kind<decltype(ln)::value>(kind, [&](auto v) {
      launch(v, grid_blocks(a.B, decltype(v)::L), shmem, TC);
      return hipGetLastError();
    });
  });
}

hipError_t launch_any(int kind, const LaunchArgs& a, int lanes, const MsedOut* ro) {
  return launch_with(kind, a, lanes, [&](auto v, dim3 grid, size_t shmem, int TC) {
    using V = decltype(v);
    if (ro) {
      hipLaunchKernelGGL((msed_kernel<V::L, V::STATIC, V::HASB, V::SCALED, true>), grid, dim3(kMsedBlock), shmem,
                         a.stream, a.theta, a.P, a.B, a.space, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out, a.flags,
                         a.flags_next, *ro);
    } else {
      hipLaunchKernelGGL((msed_kernel<V::L, V::STATIC, V::HASB, V::SCALED, false>), grid, dim3(kMsedBlock), shmem,
                         a.stream, a.theta, a.P, a.B, a.space, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out, a.flags,
                         a.flags_next, MsedOut{});
    }
  });
}

}  // namespace

// the neural kinds (yfm_msedn.hip) run the same filter through the same entry points
bool msed_kind(int kind) { return msed::kind_known(kind) || msedn_kind(kind); }

int msed_param_count(int kind) {
  if (msedn_kind(kind)) return msedn_param_count(kind);
  return msed::kind_known(kind) ? msed::kind_params(kind) : -1;
}

int msed_max_n() { return kMsedPre * kMsedBlock - 1; }

int msed_lanes_for(int B) {
  // 16 lanes per candidate until the groups fill two waves per SIMD of the chip's 1,024 (B = 8,192), then 4: the
  // 3×3 work is replicated on every lane of a group, so fewer lanes per candidate is less work as soon as the
  // chip is full either way.
  const char* const ov = env_or("YFM_MSED_LANES", nullptr);  // tuning override: 4, 16
  if (ov) {
    const int l = std::atoi(ov);
    if (l == 4 || l == 16) return l;
  }
  return B <= 8192 ? 16 : 4;
}

hipError_t launch_msed(int kind, const LaunchArgs& a, int lanes) {
  if (msedn_kind(kind)) return launch_msedn(kind, a, lanes, nullptr);
  return launch_any(kind, a, lanes, nullptr);
}

hipError_t launch_msed_grad(int kind, const LaunchArgs& a, int lanes, double* grad) {
  if (msedn_kind(kind)) return launch_msedn_grad(kind, a, lanes, grad);
  return launch_with(kind, a, lanes, [&](auto v, dim3 grid, size_t shmem, int TC) {
    using V = decltype(v);
    hipLaunchKernelGGL((lambda_grad_kernel<V::L, V::STATIC, V::HASB, V::SCALED>), grid, dim3(kMsedBlock), shmem,
                       a.stream, a.theta, a.P, a.B, a.space, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out, grad, a.flags,
                       a.flags_next);
  });
}

hipError_t launch_msed_fullgrad(int kind, const LaunchArgs& a, int lanes, double* grad) {
  if (!msed::kind_known(kind) || a.P != msed::kind_params(kind)) return hipErrorInvalidValue;
  return launch_with(kind, a, lanes, [&](auto v, dim3 grid, size_t shmem, int TC) {
    using V = decltype(v);
    hipLaunchKernelGGL((lambda_fullgrad_kernel<V::L, V::STATIC, V::HASB, V::SCALED>), grid, dim3(kMsedBlock), shmem,
                       a.stream, a.theta, a.P, a.B, a.space, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out, grad, a.flags,
                       a.flags_next);
  });
}

hipError_t launch_msed_record(int kind, const LaunchArgs& a, int lanes, const MsedRecord& r) {
  if (msedn_kind(kind)) return launch_msedn(kind, a, lanes, &r);
  MsedOut ro;
  ro.mode = r.mode;
  ro.horizon = r.horizon;
  ro.ncol = r.ncol;
  ro.preds = r.preds;
  ro.factors = r.factors;
  ro.states = r.states;
  ro.load1 = r.load1;
  ro.load2 = r.load2;
  return launch_any(kind, a, lanes, &ro);
}

}  // namespace yfm
