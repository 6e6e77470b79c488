// yfm_msedn.hip — batched loss, per-step loss array, predict and forecast of the neural Nelson–Siegel models
// (NNS, NNS-Anchored and the 24 score-driven NNS kinds) for gfx950.  FP64.
//
// Restates, per candidate θ_b (the algebra is in yfm_msedn.hpp, which names the model files):
//   get_loss         src/models/filter.jl:209-243
//   get_loss_array   src/models/filter.jl:245-281
//   predict          src/models/filter.jl:284-306
//   forecast blocks  src/forecasting.jl:236-250
//   filter           src/models/filter.jl:52-110
//
// Mapping and staging are the λ kernel's (yfm_msed.hip, yfm_msed_tree.hpp): one candidate per
// group of L ∈ {4, 16} lanes, lane j owns the maturities i ≡ j (mod L), every sum runs through the fixed 16-class
// tree, so a candidate's value does not depend on L or on the batch; the panel is staged through LDS in chunks of TC
// columns.
//
// What differs is the step.  γ (18) and β stay in registers, replicated on every lane of
// the group; A, B and ν (18 each, expanded by the duplicator) and the score's EWMA (18; every lane of the group
// writes the same values) live in LDS, one record per candidate.  The transforms
// need group-wide scalars before any lane has its loadings, so whenever γ changes the group runs `prepare`: every
// lane evaluates the anchor raws itself (12 tanh) and the group sums Q — with, for the kinds that take a score at
// these loadings, the 11 data-free sums of the score.  A step then is
//   pass A   loadings at γ: the 8 OLS statistics, ‖y_t − ŷ_{t−1}‖² and the outputs of step t − 1;  β
//   score    v per maturity at β, the 23 sums;  every lane finishes the 18-vector and updates γ;  prepare
//   pass C   loadings at the updated γ: the 8 OLS statistics;  β;  γ ← ν + B∘γ, β ← μ + Φβ;  prepare (where B)
// — the loadings are evaluated twice per step for the OLS fits, as in §3.6, plus once for the score, whose τ are
// recomputed rather than kept (a lane owns ⌈N/L⌉ maturities, too many to hold).
#pragma clang fp contract(off)
#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_msedn.hpp"
#include "yfm_msed_pass.hpp"

namespace yfm {

namespace {

using namespace msedtree;
using namespace msedpass;
using namespace msedn;

constexpr int kConsts = 4 * kG;  // A, B, ν and the score's EWMA of one candidate in LDS

template <int L, bool STATIC, bool HASB, bool SCALED, bool RECORD>
__global__ __launch_bounds__(kMsedBlock) void msedn_kernel(const double* __restrict__ theta, int P, int B, int space,
                                                            int kind, const double* __restrict__ Y, int T, int N,
                                                            int TC, const double* __restrict__ mats,
                                                            const int* __restrict__ T_use, double* __restrict__ out,
                                                            unsigned int* __restrict__ flags,
                                                            unsigned int* __restrict__ flags_next, MsedRecord ro) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int KQ = log_classes_per_lane<L>();
  constexpr int NREC = kM + kG;  // rows of a forecast block before the predictions
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_m = smem;               // N maturities
  double* s_y = smem + N;           // TC columns of N yields
  double* s_c = s_y + TC * N;       // GPB records [A(18), B(18), ν(18), EWMA(18)]
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
  for (int i = tid; i < N; i += kMsedBlock) s_m[i] = mats[i];
  __syncthreads();
  const bool traj = RECORD && (ro.mode == 1 || ro.mode == 2);
  const int my_steps = traj ? nobs + ro.horizon - 1 : nobs - 1;
  const int my_iters = my_steps + 1;
  atomicMax(&s_iters_max, live ? my_iters : 0);

  // every lane of the group decodes the same θ: the 18-vectors go to the group's record (the same values from
  // every lane), the rest to registers
  double* const cA = s_c + grp * kConsts;
  double* const cB = cA + kG;
  double* const cNu = cB + kG;
  double* const cEw = cNu + kG;
  Model mdl;
  State st;
  {
    double g0[kG];
    decode(theta + (size_t)bb * P, space, kind, mdl, cA, cB, cNu, g0);
#pragma unroll
    for (int k = 0; k < kM; ++k) st.beta[k] = mdl.beta0[k];
#pragma unroll
    for (int k = 0; k < kG; ++k) {
      st.gamma[k] = g0[k];
      cEw[k] = 0.0;
    }
    st.fpow = 1.0;
  }
  const bool anchored = mdl.anchored;
  const Ends ends = {s_m[0], s_m[N - 2], s_m[N - 1]};
  const double fN = (double)N;

  double mse = 0.0;
  bool fail = false;       // get_loss / get_loss_array return −Inf
  bool pred_fail = false;  // the last step returned −Inf instead of a prediction

  __syncthreads();
  const int niter = s_iters_max;
  const int CHY = TC * N;
  if (live) prepare_group<L, !STATIC>(st, anchored, ends, s_m, N, j);

  // ---- panel staging: chunk c (columns cTC .. cTC+TC−1) in LDS.  No register prefetch of the next chunk, unlike
  // the λ kernel: a step here is thousands of instructions, so one exposed load per TC steps costs nothing, and the
  // 16 registers are better spent on the score pass ----
  auto stage_chunk = [&](int c) { chunk_stage(Y, s_y, c, CHY, T, N, tid); };
  if (niter > 0) {
    stage_chunk(0);
    __syncthreads();
  }

  for (int t = 0; t < niter; ++t) {
    const int tt = t % TC;
    const bool act = live && t < my_iters;
    if (act) {
      const double* col = s_y + tt * N;
      const bool has_col = t < nobs;         // a data column (the rest is the NaN padding)
      const bool compare = !traj && t >= 1;  // y_t against the prediction of step t − 1 (t < nobs here)
      const bool emit = traj && t >= 1;      // outputs of step t − 1
      double *e_pred = nullptr, *e_l1 = nullptr, *e_l2 = nullptr;
      if constexpr (RECORD) {
        if (emit && ro.mode == 1) {
          const size_t o = ((size_t)b * ro.ncol + (t - 1)) * N;
          e_pred = ro.preds + o;
          e_l1 = ro.load1 ? ro.load1 + o : nullptr;
          e_l2 = ro.load2 ? ro.load2 + o : nullptr;
        } else if (emit && ro.mode == 2) {
          const int k = (t - 1) - (nobs - 1);
          if (k >= 0) e_pred = ro.preds + ((size_t)b * ro.horizon + k) * (NREC + N) + NREC;
        }
      }
      // ---- pass A: the loadings at γ ----
      const double ninf = -__builtin_inf();
      PassStats sa;
      auto leaf_a = [&](int c, PassStats& s) {
        s.zero();
        for (int i = c; i < N; i += kMsedClasses) {
          double z2, z3;
          Point p;
          loadings(st.gamma, st.sc, i, N, s_m[i], z2, z3, p);
          const double y = has_col ? col[i] : 0.0;
          msed::accum_ols(s.o, z2, z3, y);
          const double pr = msed::fitted(st.beta, z2, z3);
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
#pragma unroll
      for (int k = 0; k < NOLS; ++k) sa.o[k] = group_sum_desc<L>(sa.o[k]);
      sa.vv = group_sum_desc<L>(sa.vv);

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
          advance<HASB>(mdl, cB, cNu, st);
          if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
        } else if (!msed::ols(sa.o, fN, st.beta)) {
          pred_fail = true;
        } else {
          bool ok = true;
          if constexpr (!STATIC) {
            // ---- the score at β: v per maturity, the 23 sums, the 18-vector on every lane ----
            Sums<NSCORE> sc;
            auto leaf_s = [&](int c, Sums<NSCORE>& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) accum_score(s.v, st.gamma, st.sc, st.beta, i, N, s_m[i], col[i]);
            };
            class_tree<KQ>(j, leaf_s, sc);
            sc.template reduce<L>();
            {
              double g[kG];
              finish_score(sc.v, st.aux, st.gamma, st.sc, anchored, ends, g);
              update_gamma<SCALED>(cA, cEw, st, g);
            }
            prepare_group<L, !HASB>(st, anchored, ends, s_m, N, j);
            // ---- pass C: the loadings at the updated γ ----
            Sums<NOLS> sb;
            auto leaf_b = [&](int c, Sums<NOLS>& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) {
                double z2, z3;
                Point p;
                loadings(st.gamma, st.sc, i, N, s_m[i], z2, z3, p);
                msed::accum_ols(s.v, z2, z3, col[i]);
              }
            };
            class_tree<KQ>(j, leaf_b, sb);
            sb.template reduce<L>();
            ok = msed::ols(sb.v, fN, st.beta);
          }
          if (ok) {
            advance<HASB>(mdl, cB, cNu, st);
            if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
          } else {
            pred_fail = true;  // the state stays as the failing call left it: γ updated, β not
            if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
          }
        }
        if constexpr (RECORD) {
          // factors and states of column t: β and γ after the step (filter.jl:299-300)
          if (j == 0 && ro.mode == 1) {
            const size_t o = (size_t)b * ro.ncol + t;
#pragma unroll
            for (int k = 0; k < kM; ++k) ro.factors[o * kM + k] = st.beta[k];
#pragma unroll
            for (int k = 0; k < kG; ++k) ro.states[o * kG + k] = st.gamma[k];
          } else if (j == 0 && ro.mode == 2) {
            const int k = t - (nobs - 1);
            if (k >= 0) {
              double* o = ro.preds + ((size_t)b * ro.horizon + k) * (NREC + N);
#pragma unroll
              for (int q = 0; q < kM; ++q) o[q] = st.beta[q];
#pragma unroll
              for (int q = 0; q < kG; ++q) o[kM + q] = st.gamma[q];
            }
          }
        }
      }
    }
    if (tt == TC - 1) {  // chunk done: its buffer takes the next one
      __syncthreads();
      stage_chunk(t / TC + 1);
      __syncthreads();
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

// get_loss and its gradient with respect to δ and Φ in one pass: msedn_kernel's loss mode — the same mapping, LDS
// record, staging, passes and sums, so the loss is the same bits — whose pass A also forms s = Z'v at the loadings
// the prediction of step t − 1 used, from which every lane of the group updates the 12 accumulators (replicated like
// the state; the algebra is msed::grad_accum / grad_finish).  Writes the loss to out[b] and the
// gradient, in the caller's space, to grad[12·b ..]; NaN where the loss is −Inf.
template <int L, bool STATIC, bool HASB, bool SCALED>
__global__ __launch_bounds__(kMsedBlock) void neural_grad_kernel(const double* __restrict__ theta, int P, int B,
                                                                  int space, int kind, const double* __restrict__ Y,
                                                                  int T, int N, int TC,
                                                                  const double* __restrict__ mats,
                                                                  const int* __restrict__ T_use,
                                                                  double* __restrict__ out, double* __restrict__ grad,
                                                                  unsigned int* __restrict__ flags,
                                                                  unsigned int* __restrict__ flags_next) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int KQ = log_classes_per_lane<L>();
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_m = smem;               // N maturities
  double* s_y = smem + N;           // TC columns of N yields
  double* s_c = s_y + TC * N;       // GPB records [A(18), B(18), ν(18), EWMA(18)]
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
  for (int i = tid; i < N; i += kMsedBlock) s_m[i] = mats[i];
  __syncthreads();
  const int my_steps = nobs - 1;
  const int my_iters = my_steps + 1;  // iteration t: the comparison of step t − 1, then step t
  atomicMax(&s_iters_max, live ? my_iters : 0);

  double* const cA = s_c + grp * kConsts;
  double* const cB = cA + kG;
  double* const cNu = cB + kG;
  double* const cEw = cNu + kG;
  const double* th = theta + (size_t)bb * P;
  Model mdl;
  State st;
  {
    double g0[kG];
    decode(th, space, kind, mdl, cA, cB, cNu, g0);
#pragma unroll
    for (int k = 0; k < kM; ++k) st.beta[k] = mdl.beta0[k];
#pragma unroll
    for (int k = 0; k < kG; ++k) {
      st.gamma[k] = g0[k];
      cEw[k] = 0.0;
    }
    st.fpow = 1.0;
  }
  const bool anchored = mdl.anchored;
  const Ends ends = {s_m[0], s_m[N - 2], s_m[N - 1]};
  const double fN = (double)N;

  double mse = 0.0;
  bool fail = false;
  bool pred_fail = false;
  msed::Grad g;
  msed::grad_zero(g);
  double bpost[kM] = {0.0, 0.0, 0.0};  // the β step t − 1 predicted from
  bool pred_only = false;              // step t − 1 was prediction-only

  __syncthreads();
  const int niter = s_iters_max;
  const int CHY = TC * N;
  if (live) prepare_group<L, !STATIC>(st, anchored, ends, s_m, N, j);

  // ---- panel staging, as msedn_kernel ----
  auto stage_chunk = [&](int c) { chunk_stage(Y, s_y, c, CHY, T, N, tid); };
  if (niter > 0) {
    stage_chunk(0);
    __syncthreads();
  }

  for (int t = 0; t < niter; ++t) {
    const int tt = t % TC;
    const bool act = live && t < my_iters;
    if (act) {
      const double* col = s_y + tt * N;  // t < nobs: always a data column here
      // ---- pass A: the loadings at γ ----
      GradPassStats sa;
      auto leaf_a = [&](int c, GradPassStats& s) {
        s.zero();
        for (int i = c; i < N; i += kMsedClasses) {
          double z2, z3;
          Point p;
          loadings(st.gamma, st.sc, i, N, s_m[i], z2, z3, p);
          const double y = col[i];
          msed::accum_ols(s.s.o, z2, z3, y);
          const double pr = msed::fitted(st.beta, z2, z3);
          const double v = y - pr;
          s.s.vv = mfma(v, v, s.s.vv);
          msed::accum_zv(s.zv, z2, z3, v);
        }
      };
      class_tree<KQ>(j, leaf_a, sa);
#pragma unroll
      for (int k = 0; k < NOLS; ++k) sa.s.o[k] = group_sum_desc<L>(sa.s.o[k]);
      sa.s.vv = group_sum_desc<L>(sa.s.vv);
#pragma unroll
      for (int k = 0; k < kM; ++k) sa.zv[k] = group_sum_desc<L>(sa.zv[k]);

      if (t >= 1) {
        // v = y_t − ŷ_t; mse −= v'v; a non-finite running sum returns −Inf (filter.jl:226-234)
        mse += pred_fail ? -__builtin_inf() : -sa.s.vv;
        fail = fail || !(fabs(mse) <= __DBL_MAX__);
        msed::grad_accum(mdl, pred_only, sa.zv, bpost, g);
      }

      if (t < my_steps) {
        // ---- step t (filter.jl:52-110), as msedn_kernel ----
        pred_only = col[0] != col[0];
        pred_fail = false;
        if (pred_only) {
          advance<HASB>(mdl, cB, cNu, st);
          if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
        } else if (!msed::ols(sa.s.o, fN, st.beta)) {
          pred_fail = true;
        } else {
          bool ok = true;
          if constexpr (!STATIC) {
            // ---- the score at β: v per maturity, the 23 sums, the 18-vector on every lane ----
            Sums<NSCORE> sc;
            auto leaf_s = [&](int c, Sums<NSCORE>& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) accum_score(s.v, st.gamma, st.sc, st.beta, i, N, s_m[i], col[i]);
            };
            class_tree<KQ>(j, leaf_s, sc);
            sc.template reduce<L>();
            {
              double gg[kG];
              finish_score(sc.v, st.aux, st.gamma, st.sc, anchored, ends, gg);
              update_gamma<SCALED>(cA, cEw, st, gg);
            }
            prepare_group<L, !HASB>(st, anchored, ends, s_m, N, j);
            // ---- pass C: the loadings at the updated γ ----
            Sums<NOLS> sb;
            auto leaf_b = [&](int c, Sums<NOLS>& s) {
              s.zero();
              for (int i = c; i < N; i += kMsedClasses) {
                double z2, z3;
                Point p;
                loadings(st.gamma, st.sc, i, N, s_m[i], z2, z3, p);
                msed::accum_ols(s.v, z2, z3, col[i]);
              }
            };
            class_tree<KQ>(j, leaf_b, sb);
            sb.template reduce<L>();
            ok = msed::ols(sb.v, fN, st.beta);
          }
          if (ok) {
#pragma unroll
            for (int k = 0; k < kM; ++k) bpost[k] = st.beta[k];
            advance<HASB>(mdl, cB, cNu, st);
            if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
          } else {
            pred_fail = true;  // the state stays as the failing call left it: γ updated, β not
            if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
          }
        }
      }
    }
    if (tt == TC - 1) {  // chunk done: its buffer takes the next one
      __syncthreads();
      stage_chunk(t / TC + 1);
      __syncthreads();
    }
  }

  if (!live || j != 0) return;
  out[b] = finish_loss(mse, fN, nobs, fail, flags);
  double go[msed::kGrad];
  msed::grad_finish(g, th, P, space, fN, nobs, fail, go);
#pragma unroll
  for (int k = 0; k < msed::kGrad; ++k) grad[(size_t)b * msed::kGrad + k] = go[k];
}

// launch(Variant, grid, shared-memory bytes, TC) starts the kernel of a kind at a lane count on a's batch and panel
template <class F>
hipError_t launch_with(int kind, const LaunchArgs& a, int lanes, F&& launch) {
  const int TC = chunk_columns(a.N);
  if (TC < 1) return hipErrorInvalidValue;
  return with_lanes(lanes, [&](auto ln) {
    constexpr int L = decltype(ln)::value;
    return with_neural_kind<L>(kind, [&](auto v) {
      launch(v, grid_blocks(a.B, L), neural_shmem(L, a.N, TC, kConsts), TC);
      return hipGetLastError();
    });
  });
}

}  // namespace

bool msedn_kind(int kind) { return msedn::kind_known(kind); }

int msedn_param_count(int kind) { return msedn::kind_known(kind) ? msedn::kind_params(kind) : -1; }

int msedn_min_n() { return msedn::kMinN; }

// the panel chunk, the maturities and the 64 constant records of an L = 4 block stay within 64 KiB of LDS
int msedn_max_n() { return 1024; }

// the gradient kernel's block has the loss kernel's LDS layout: the same limit
int msedn_grad_max_n() { return msedn_max_n(); }

hipError_t launch_msedn(int kind, const LaunchArgs& a, int lanes, const MsedRecord* r) {
  if (!msedn::kind_known(kind) || a.N < msedn_min_n() || a.N > msedn_max_n()) return hipErrorInvalidValue;
  return launch_with(kind, a, lanes, [&](auto v, dim3 grid, size_t shmem, int TC) {
    using V = decltype(v);
    if (r) {
      hipLaunchKernelGGL((msedn_kernel<V::L, V::STATIC, V::HASB, V::SCALED, true>), grid, dim3(kMsedBlock), shmem,
                         a.stream, a.theta, a.P, a.B, a.space, kind, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out,
                         a.flags, a.flags_next, *r);
    } else {
      hipLaunchKernelGGL((msedn_kernel<V::L, V::STATIC, V::HASB, V::SCALED, false>), grid, dim3(kMsedBlock), shmem,
                         a.stream, a.theta, a.P, a.B, a.space, kind, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out,
                         a.flags, a.flags_next, MsedRecord{});
    }
  });
}

hipError_t launch_msedn_grad(int kind, const LaunchArgs& a, int lanes, double* grad) {
  if (!msedn::kind_known(kind) || a.N < msedn_min_n() || a.N > msedn_grad_max_n()) return hipErrorInvalidValue;
  return launch_with(kind, a, lanes, [&](auto v, dim3 grid, size_t shmem, int TC) {
    using V = decltype(v);
    hipLaunchKernelGGL((neural_grad_kernel<V::L, V::STATIC, V::HASB, V::SCALED>), grid, dim3(kMsedBlock), shmem,
                       a.stream, a.theta, a.P, a.B, a.space, kind, a.raw, a.T, a.N, TC, a.mats, a.T_use, a.out, grad,
                       a.flags, a.flags_next);
  });
}

}  // namespace yfm
