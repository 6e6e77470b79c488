// yfm_msedn_adj.hip — the loss of the neural Nelson–Siegel models with ∂loss/∂θ over all P rows, for gfx950.  FP64.
//
// Two kernels on one stream (the algebra is yfm_msedn_adj.hpp's):
//   nns_sweep_kernel    the forward sweep: neural_grad_kernel's loop — the same mapping, staging, passes and sums, so the
//                       loss and rows P−12 … P−1 are its bits — which also stores the γ (and, for the scaled kinds, the
//                       e) every step enters with: one contiguous record per candidate and step in HBM, the lanes of
//                       the group writing disjoint components.
//   nns_adjoint_kernel  the backward sweep: per step, from the last compared column to the first, it rebuilds the step
//                       from its record (prepare, OLS, score, update, OLS at γ⁺, γ_next), then runs the five items of
//                       the backward step.  Every 18-vector — γ, γ⁺, γ_next, the score, the direction ḡ, the adjoints γ̄,
//                       ē and the accumulators Ā, B̄, ω̄ — lives in the candidate's LDS record (every lane of the group
//                       writes the same values), so a pass holds only its sums and its scalars in registers.
// The static kinds run both as well: they are the recursion with A = 0 and γ_next = γ, whose backward step is items
// 1 and 2 alone, and they keep no trajectory.
// Mapping and sums are msedn_kernel's: one candidate per group of L lanes (the forward sweep L ∈ {4, 16}, the backward
// sweep 16), every sum through the 16-class tree, so a candidate's P + 1 outputs depend neither on L nor on the batch
// nor on how the launch is chunked.
#pragma clang fp contract(off)
#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_msedn_adj.hpp"
#include "yfm_msed_pass.hpp"

namespace yfm {

namespace {

using namespace msedtree;
using namespace msedpass;
using namespace msedn;

constexpr int kConsts = 4 * kG;  // the forward sweep's record: A, B, ν and the score's EWMA

// the backward sweep's record
enum : int {
  RA = 0,             // A
  RB = RA + kG,       // B
  RW = RB + kG,       // ω
  RADJ = RW + kG,     // γ̄, ē, Ā, B̄, ω̄ (yfm_msedn_adj.hpp: JG …)
  RG = RADJ + NADJ,   // γ the step enters with
  RGP = RG + kG,      // γ⁺
  RGN = RGP + kG,     // γ_next
  RS = RGN + kG,      // the score g
  RD = RS + kG,       // (γ, ḡ) as 18 Duals
  RF1 = RD + 2 * kG,  // the fit at γ: Scal, the data-free sums, the OLS statistics and β₁ (Fit)
  RF2 = RF1 + 30,     // the fit at γ⁺
  RM = RF2 + 30,      // the decoded Model
  NREC = RM + 16
};

// what the backward step keeps of an OLS fit between its passes
struct Fit {
  Scal sc;
  double aux[NAUX];
  double o[NOLS];
  double beta[kM];
};
static_assert(sizeof(Fit) <= 30 * sizeof(double) && sizeof(Model) <= 16 * sizeof(double), "record slots");

template <int NV, int NW>
struct DualSums {
  Dual v[NV];
  double w[NW];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = mk(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0.0;
  }
  __device__ __forceinline__ void add(const DualSums& a, const DualSums& b) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = a.v[k] + b.v[k];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = a.w[k] + b.w[k];
  }
  template <int L>
  __device__ __forceinline__ void reduce() {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = mk(group_sum_desc<L>(v[k].v), group_sum_desc<L>(v[k].d));
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = group_sum_desc<L>(w[k]);
  }
};

// ---- the forward sweep -------------------------------------------------------------------------------------------
// neural_grad_kernel with the trajectory: before step t the group stores the γ (and e) it enters with to
// traj[(b·(T − 1) + t)·STR ..], lane j the components k ≡ j (mod L).  The loss goes to out[b], grad_finish's 12 to rows
// P−12 … P−1 of grad (P×B column-major).
template <int L, bool STATIC, bool HASB, bool SCALED>
__global__ __launch_bounds__(kMsedBlock) void nns_sweep_kernel(const double* __restrict__ theta, int P, int B, int space,
                                                                int kind, const double* __restrict__ Y, int T, int N,
                                                                int TC, const double* __restrict__ mats,
                                                                const int* __restrict__ T_use, double* __restrict__ out,
                                                                double* __restrict__ grad, double* __restrict__ traj,
                                                                unsigned int* __restrict__ flags,
                                                                unsigned int* __restrict__ flags_next) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int KQ = log_classes_per_lane<L>();
  constexpr int STR = STATIC ? 0 : (SCALED ? 2 * kG : kG);
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
        mse += pred_fail ? -__builtin_inf() : -sa.s.vv;
        fail = fail || !(fabs(mse) <= __DBL_MAX__);
        msed::grad_accum(mdl, pred_only, sa.zv, bpost, g);
      }

      if (t < my_steps) {
        // ---- the record of step t: what it enters with ----
        if constexpr (!STATIC) {
          if (t < T - 1) {
            double* const rec = traj + ((size_t)b * (T - 1) + t) * STR;
#pragma unroll
            for (int k = 0; k < kG; ++k)
              if (k % L == j) {
                rec[k] = st.gamma[k];
                if constexpr (SCALED) rec[kG + k] = cEw[k];
              }
          }
        }
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
            pred_fail = true;
            if constexpr (HASB) prepare_group<L, true>(st, anchored, ends, s_m, N, j);
          }
        }
      }
    }
    if (tt == TC - 1) {
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
  for (int k = 0; k < msed::kGrad; ++k) grad[(size_t)b * P + (P - msed::kGrad) + k] = go[k];
}

// ---- the backward sweep's passes, each by the whole group at a γ of the record ---------------------------------------
template <int L>
__device__ __forceinline__ void prepare_at(const double* gam, Scal& sc, double (&aux)[NAUX], bool anchored,
                                           const Ends& e, const double* s_m, int N, int j) {
  anchors(gam, anchored, e, sc);
  Sums<NAUX> sa;
  auto leaf = [&](int c, Sums<NAUX>& s) {
    s.zero();
    for (int i = c; i < N; i += kMsedClasses) accum_aux<true>(s.v, gam, sc, i, N, s_m[i]);
  };
  class_tree<log_classes_per_lane<L>()>(j, leaf, sa);
  sa.template reduce<L>();
#pragma unroll
  for (int k = 0; k < NAUX; ++k) aux[k] = sa.v[k];
  finish_scale(aux[AQ], anchored, sc);
}

template <int L>
__device__ __forceinline__ bool ols_at(const double* gam, const Scal& sc, const double* s_m, const double* col, int N,
                                       int j, double (&o)[NOLS], double (&beta)[kM], bool& ridged) {
  Sums<NOLS> sb;
  auto leaf = [&](int c, Sums<NOLS>& s) {
    s.zero();
    for (int i = c; i < N; i += kMsedClasses) {
      double z2, z3;
      Point p;
      loadings(gam, sc, i, N, s_m[i], z2, z3, p);
      msed::accum_ols(s.v, z2, z3, col[i]);
    }
  };
  class_tree<log_classes_per_lane<L>()>(j, leaf, sb);
  sb.template reduce<L>();
#pragma unroll
  for (int k = 0; k < NOLS; ++k) o[k] = sb.v[k];
  return msed::ols(o, (double)N, beta, ridged);
}

// pull at γ on column col: SCORE: a = 2βv (the score at β; zv = Z'v beside it); else the OLS transpose's for (β, u)
template <int L, bool SCORE>
__device__ __forceinline__ void pull_at(const double* gam, const Scal& sc, const double (&aux)[NAUX], bool anchored,
                                        const Ends& e, const double* s_m, const double* col, int N, int j,
                                        const double (&beta)[kM], const double (&u)[kM], double (&zv)[kM],
                                        double (&out)[kG]) {
  constexpr int NV = NSCORE + (SCORE ? kM : 0);
  Sums<NV> ss;
  auto leaf = [&](int c, Sums<NV>& s) {
    s.zero();
    for (int i = c; i < N; i += kMsedClasses) {
      double z2, z3, a2, a3;
      Point p;
      const double m = s_m[i];
      loadings(gam, sc, i, N, m, z2, z3, p);
      if constexpr (SCORE) {
        const double v = col[i] - msed::fitted(beta, z2, z3);
        s.v[NSCORE] += v;
        s.v[NSCORE + 1] = mfma(z2, v, s.v[NSCORE + 1]);
        s.v[NSCORE + 2] = mfma(z3, v, s.v[NSCORE + 2]);
        a2 = (2.0 * beta[1]) * v;
        a3 = (2.0 * beta[2]) * v;
      } else {
        ols_pull_coef(beta, u, z2, z3, col[i], a2, a3);
      }
      accum_pull(s.v, gam, sc, p, i, N, m, a2, a3);
    }
  };
  class_tree<log_classes_per_lane<L>()>(j, leaf, ss);
  ss.template reduce<L>();
  if constexpr (SCORE) {
#pragma unroll
    for (int k = 0; k < kM; ++k) zv[k] = ss.v[NSCORE + k];
  }
  finish_score(ss.v, aux, gam, sc, anchored, e, out);
}

// the Hessian–vector product of the score along the direction of dg (18 Duals of the record) at β fixed, with
// w = ∂(ḡ·g)/∂β
template <int L>
__device__ __forceinline__ void score_hvp_at(const Dual* dg, bool anchored, const Ends& e, const double* s_m,
                                             const double* col, int N, int j, const double (&beta)[kM],
                                             double (&w)[kM], double (&hv)[kG]) {
  constexpr int KQ = log_classes_per_lane<L>();
  DScal dsc;
  Dual daux[NAUX];
  anchors(dg, anchored, e, dsc);
  {
    DualSums<NAUX, 1> sa;
    auto leaf = [&](int c, DualSums<NAUX, 1>& s) {
      s.zero();
      for (int i = c; i < N; i += kMsedClasses) accum_aux(s.v, dg, dsc, i, N, s_m[i]);
    };
    class_tree<KQ>(j, leaf, sa);
    sa.template reduce<L>();
#pragma unroll
    for (int k = 0; k < NAUX; ++k) daux[k] = sa.v[k];
  }
  finish_scale(daux[AQ], anchored, dsc);
  DualSums<NSCORE, kM> ss;
  auto leaf = [&](int c, DualSums<NSCORE, kM>& s) {
    s.zero();
    for (int i = c; i < N; i += kMsedClasses) accum_score(s.v, s.w, dg, dsc, beta, i, N, s_m[i], col[i]);
  };
  class_tree<KQ>(j, leaf, ss);
  ss.template reduce<L>();
#pragma unroll
  for (int k = 0; k < kM; ++k) w[k] = ss.w[k];
  finish_score(ss.v, daux, dg, dsc, anchored, e, hv);
}

// ---- the backward sweep ------------------------------------------------------------------------------------------
// Reads the loss (out) and rows P−12 … P−1 (grad) the forward sweep left, sweeps the steps nobs − 2 … 0 and writes all
// P rows: NaN where the loss is −Inf, and where an adjoint is not finite (counted in flags[5]).  The panel is staged
// in chunks of TC columns that overlap by one: chunk c holds the columns c(TC − 1) … c(TC − 1) + TC − 1, the steps
// c(TC − 1) … c(TC − 1) + TC − 2 with their next columns.
template <int L, bool STATIC, bool HASB, bool SCALED>
__global__ __launch_bounds__(kMsedBlock) void nns_adjoint_kernel(const double* __restrict__ theta, int P, int B,
                                                                  int space, int kind, const double* __restrict__ Y,
                                                                  int T, int N, int TC,
                                                                  const double* __restrict__ mats,
                                                                  const int* __restrict__ T_use,
                                                                  const double* __restrict__ out,
                                                                  double* __restrict__ grad,
                                                                  const double* __restrict__ traj,
                                                                  unsigned int* __restrict__ flags) {
  constexpr int GPB = kMsedBlock / L;
  constexpr int STR = STATIC ? 0 : (SCALED ? 2 * kG : kG);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_m = smem;               // N maturities
  double* s_y = smem + N;           // TC columns of N yields
  double* s_r = s_y + TC * N;       // GPB records of NREC doubles
  __shared__ int s_steps_max;

  const int tid = threadIdx.x;
  const int j = tid % L;
  const int grp = tid / L;
  const int b = blockIdx.x * GPB + grp;
  const bool live = b < B;
  const int bb = live ? b : (B - 1);
  const int nobs = T_use ? T_use[bb] : T;
  const double ll = out[bb];
  const bool fail = !(ll > -__builtin_inf());  // −Inf (and NaN): no sweep, NaN rows
  // the steps this group sweeps: those the forward sweep recorded
  int my_steps = nobs - 1;
  if (my_steps > T - 1) my_steps = T - 1;
  if (!live || fail) my_steps = 0;

  if (tid == 0) s_steps_max = 0;
  for (int i = tid; i < N; i += kMsedBlock) s_m[i] = mats[i];
  __syncthreads();
  atomicMax(&s_steps_max, my_steps);

  double* const rec = s_r + grp * NREC;
  const double* th = theta + (size_t)bb * P;
  Model& mdl = *reinterpret_cast<Model*>(rec + RM);
  Fit& f1 = *reinterpret_cast<Fit*>(rec + RF1);
  Fit& f2 = *reinterpret_cast<Fit*>(rec + RF2);
  {
    double nu[kG];
    decode(th, space, kind, mdl, rec + RA, rec + RB, nu, rec + RW);
#pragma unroll
    for (int k = 0; k < NADJ; ++k) rec[RADJ + k] = 0.0;
  }
  const bool anchored = mdl.anchored;
  const Ends ends = {s_m[0], s_m[N - 2], s_m[N - 1]};
  const double fN = (double)N;
  double* const adj = rec + RADJ;

  __syncthreads();
  const int nsteps = s_steps_max;
  const int S = TC - 1;  // steps per chunk
  const int CHY = TC * N;
  auto stage_chunk = [&](int c) {
    const size_t base = (size_t)c * S * N;
    const size_t lim = (size_t)T * N;
#pragma unroll
    for (int r = 0; r < kMsedPre; ++r) {
      const int e = r * kMsedBlock + tid;
      const size_t gi = base + e;
      if (e < CHY) s_y[e] = gi < lim ? Y[gi] : 0.0;
    }
  };
  if (nsteps > 0) {
    stage_chunk((nsteps - 1) / S);
    __syncthreads();
  }
  const bool first_missing = nsteps > 0 && Y[0] != Y[0];

  for (int t = nsteps - 1; t >= 0; --t) {
    const int tt = t % S;
    if (t < my_steps) {
      const double* col = s_y + tt * N;
      const double* coln = col + N;
      const bool pred_only = col[0] != col[0];  // t = 0: a later missing column made the loss −Inf
      const double* trec = traj + ((size_t)b * (T - 1) + t) * STR;
      double den = 1.0;
      if constexpr (SCALED) den = 1.0 - forget_pow(t + (first_missing ? 0 : 1));
      // ---- the step again, from its record ----
      if constexpr (STATIC) {
#pragma unroll
        for (int k = 0; k < kG; ++k) rec[RG + k] = rec[RW + k];
      } else {
#pragma unroll
        for (int k = 0; k < kG; ++k) rec[RG + k] = trec[k];
      }
      double bpred[kM];
      bool rd1 = false, rd2 = false, ok = true;
      if (!pred_only) {
        prepare_at<L>(rec + RG, f1.sc, f1.aux, anchored, ends, s_m, N, j);
        ok = ols_at<L>(rec + RG, f1.sc, s_m, col, N, j, f1.o, f1.beta, rd1);
        if constexpr (!STATIC) {
          double zv[kM], gs[kG];
          pull_at<L, true>(rec + RG, f1.sc, f1.aux, anchored, ends, s_m, col, N, j, f1.beta, f1.beta, zv, gs);
#pragma unroll
          for (int k = 0; k < kG; ++k) {
            double gk = gs[k];
            rec[RS + k] = gk;
            if constexpr (SCALED) {
              const double ep = kForget * trec[kG + k] + (1.0 - kForget) * (gk * gk);
              gk = gk / (sqrt(ep / den) + msed::kEps);
            }
            rec[RGP + k] = rec[RG + k] + gk * rec[RA + k];
          }
        } else {
#pragma unroll
          for (int k = 0; k < kG; ++k) rec[RGP + k] = rec[RG + k];
        }
        prepare_at<L>(rec + RGP, f2.sc, f2.aux, anchored, ends, s_m, N, j);
        ok = ols_at<L>(rec + RGP, f2.sc, s_m, col, N, j, f2.o, f2.beta, rd2) && ok;
      } else {
#pragma unroll
        for (int k = 0; k < kM; ++k) f2.beta[k] = mdl.beta0[k];
#pragma unroll
        for (int k = 0; k < kG; ++k) rec[RGP + k] = rec[RG + k];
      }
#pragma unroll
      for (int r = 0; r < kM; ++r) {
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < kM; ++c) a = mfma(mdl.Phi[r][c], f2.beta[c], a);
        bpred[r] = mdl.mu[r] + a;
      }
      // ---- 1. the loss term at γ_next ----
      double zv[kM] = {0.0, 0.0, 0.0};
      {
        double gs[kG];
        if constexpr (HASB) {
#pragma unroll
          for (int k = 0; k < kG; ++k) rec[RGN + k] = (1.0 - rec[RB + k]) * rec[RW + k] + rec[RB + k] * rec[RGP + k];
          Scal scn;
          double auxn[NAUX];
          prepare_at<L>(rec + RGN, scn, auxn, anchored, ends, s_m, N, j);
          pull_at<L, true>(rec + RGN, scn, auxn, anchored, ends, s_m, coln, N, j, bpred, bpred, zv, gs);
        } else {
          if (pred_only) prepare_at<L>(rec + RGP, f2.sc, f2.aux, anchored, ends, s_m, N, j);
          pull_at<L, true>(rec + RGP, f2.sc, f2.aux, anchored, ends, s_m, coln, N, j, bpred, bpred, zv, gs);
        }
#pragma unroll
        for (int k = 0; k < kG; ++k) adj[JG + k] += gs[k];
      }
      if (!ok) adj[JG] = __builtin_nan("");  // a fit of the forward sweep that does not factor here
      if (pred_only) {
#pragma unroll
        for (int k = 0; k < kG; ++k)
          (void)adjoint_update<true, HASB, false>(adj, k, 0.0, rec[RB + k], rec[RW + k], 0.0, 0.0, 0.0, rec[RG + k], 0.0,
                                                  1.0, 1.0);
      } else {
        // ---- 2. the OLS transpose of β₂ at γ⁺; 3., 4. the accumulators and the update's adjoint ----
        double w[kM], u[kM] = {0.0, 0.0, 0.0};
        beta_adjoint(mdl, zv, w);
        (void)ols_solve(f2.o, fN, rd2, w, u);
        {
          double p2[kG];
          pull_at<L, false>(rec + RGP, f2.sc, f2.aux, anchored, ends, s_m, col, N, j, f2.beta, u, zv, p2);
          Dual* const dg = reinterpret_cast<Dual*>(rec + RD);
#pragma unroll
          for (int k = 0; k < kG; ++k) {
            const double gk = STATIC ? 0.0 : rec[RS + k];
            double ep = 0.0, sden = 1.0, gt = gk;
            if constexpr (SCALED) {
              ep = kForget * trec[kG + k] + (1.0 - kForget) * (gk * gk);
              sden = sqrt(ep / den) + msed::kEps;
              gt = gk / sden;
            }
            const double gb = adjoint_update<STATIC, HASB, SCALED>(adj, k, rec[RA + k], rec[RB + k], rec[RW + k], p2[k],
                                                                   gk, gt, rec[RGP + k], ep, sden, den);
            if constexpr (!STATIC) dg[k] = mk(rec[RG + k], gb);
          }
        }
        if constexpr (!STATIC) {
          // ---- 5. the score's adjoint ----
          double w1[kM];
          {
            double hv[kG];
            score_hvp_at<L>(reinterpret_cast<const Dual*>(rec + RD), anchored, ends, s_m, col, N, j, f1.beta, w1, hv);
#pragma unroll
            for (int k = 0; k < kG; ++k) adj[JG + k] += hv[k];
          }
          (void)ols_solve(f1.o, fN, rd1, w1, u);
          double p1[kG];
          pull_at<L, false>(rec + RG, f1.sc, f1.aux, anchored, ends, s_m, col, N, j, f1.beta, u, zv, p1);
#pragma unroll
          for (int k = 0; k < kG; ++k) adj[JG + k] += p1[k];
        }
      }
    }
    if (tt == 0 && t > 0) {  // chunk done: its buffer takes the one before
      __syncthreads();
      stage_chunk((t - 1) / S);
      __syncthreads();
    }
  }

  if (!live) return;
#pragma unroll
  for (int k = 0; k < kG; ++k) adj[JW + k] += adj[JG + k];
  if (j != 0) return;
  double tail[msed::kGrad];
#pragma unroll
  for (int k = 0; k < msed::kGrad; ++k) tail[k] = grad[(size_t)b * P + (P - msed::kGrad) + k];
  // straight into the candidate's column of grad: fullgrad_finish indexes its output by the kind's row layout
  if (fullgrad_finish(adj, rec + RA, rec + RB, tail, kind, space, fN, nobs, fail, grad + (size_t)b * P))
    atomicAdd(&flags[5], 1u);
}

struct ChunkArgs {
  const double* theta;
  const int* T_use;
  double* out;
  double* grad;
  int B;
  unsigned int* flags_next;
};

// The backward sweep always runs 16 lanes per candidate, whatever the forward sweep ran: at L = 4 a lane's part of the
// tree holds three partial sets of the Hessian–vector pass's 49 sums, which no register budget takes without scratch,
// and a candidate's outputs do not depend on L.
constexpr int kAdjLanes = 16;

// the forward sweep of chunk c at `lanes` lanes, then its backward sweep
hipError_t launch_pair(int kind, const LaunchArgs& a, const ChunkArgs& c, int lanes, int TC, double* traj) {
  return with_lanes(lanes, [&](auto ln) {
    constexpr int L = decltype(ln)::value;
    return with_neural_kind<L>(kind, [&](auto v) {
      using V = decltype(v);
      hipLaunchKernelGGL((nns_sweep_kernel<L, V::STATIC, V::HASB, V::SCALED>), grid_blocks(c.B, L), dim3(kMsedBlock),
                         neural_shmem(L, a.N, TC, kConsts), a.stream, c.theta, a.P, c.B, a.space, kind, a.raw, a.T, a.N,
                         TC, a.mats, c.T_use, c.out, c.grad, traj, a.flags, c.flags_next);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((nns_adjoint_kernel<kAdjLanes, V::STATIC, V::HASB, V::SCALED>), grid_blocks(c.B, kAdjLanes),
                         dim3(kMsedBlock), neural_shmem(kAdjLanes, a.N, TC, NREC), a.stream, c.theta, a.P, c.B, a.space,
                         kind, a.raw, a.T, a.N, TC, a.mats, c.T_use, c.out, c.grad, traj, a.flags);
      return hipGetLastError();
    });
  });
}

// bytes of trajectory one candidate takes on a panel of T columns
size_t traj_bytes_per_candidate(int kind, int T) {
  if (kind_static(kind) || T < 2) return 0;
  return sizeof(double) * (size_t)traj_stride(kind) * (size_t)(T - 1);
}

// candidates per chunk: whole blocks within the cap (YFM_NNS_TRAJ_BYTES, else 1 GiB), one block at the least
int chunk_candidates(int kind, int B, int T, int lanes) {
  const size_t per = traj_bytes_per_candidate(kind, T);
  if (per == 0) return B;
  size_t cap = (size_t)1 << 30;
  if (const char* const ov = env_or("YFM_NNS_TRAJ_BYTES", nullptr)) {
    const long long v = std::atoll(ov);
    if (v >= 0) cap = (size_t)v;
  }
  const int gpb = kMsedBlock / lanes;
  size_t n = (cap / per) / gpb * gpb;
  if (n < (size_t)gpb) n = gpb;
  return n < (size_t)B ? (int)n : B;
}

}  // namespace

int msedn_fullgrad_max_n() { return 512; }

size_t msedn_fullgrad_traj_bytes(int kind, int B, int T, int lanes) {
  if (!msedn::kind_known(kind) || B < 1 || (lanes != 4 && lanes != 16)) return 0;
  return traj_bytes_per_candidate(kind, T) * (size_t)chunk_candidates(kind, B, T, lanes);
}

hipError_t launch_msedn_fullgrad(int kind, const LaunchArgs& a, int lanes, double* grad, double* traj) {
  if (!msedn::kind_known(kind) || a.N < msedn_min_n() || a.N > msedn_fullgrad_max_n()) return hipErrorInvalidValue;
  if (lanes != 4 && lanes != 16) return hipErrorInvalidValue;
  const int TC = chunk_columns(a.N);
  if (TC < 2) return hipErrorInvalidValue;  // the backward sweep's chunks overlap by a column
  if (traj_bytes_per_candidate(kind, a.T) > 0 && !traj) return hipErrorInvalidValue;
  const int nb = chunk_candidates(kind, a.B, a.T, lanes);
  for (int b0 = 0; b0 < a.B; b0 += nb) {
    ChunkArgs c;
    c.theta = a.theta + (size_t)b0 * a.P;
    c.T_use = a.T_use ? a.T_use + b0 : nullptr;
    c.out = a.out + b0;
    c.grad = grad + (size_t)b0 * a.P;
    c.B = a.B - b0 < nb ? a.B - b0 : nb;
    c.flags_next = b0 == 0 ? a.flags_next : nullptr;
    const hipError_t e = launch_pair(kind, a, c, lanes, TC, traj);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace yfm
