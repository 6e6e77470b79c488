// yfm_tvl_score.hip — the score series of the TVλ extended-Kalman-filter log-likelihood for gfx950 (MI355X)
// (include/yfm.h yfm_tvl_loglik_scores_batch, yfm_tvl_loglik_info_batch).  An extension: the reference's estimate!
// returns no covariance.
//
// tvl_score_kernel: tvl_grad_kernel's recursion (yfm_tvl_grad.hip: one candidate per group of 32 lanes, one direction
// per lane, the functions of yfm_tvl_grad.hpp, the same fences) that stores, after every step, its direction's share of
// the term get_loss adds there — S[d, k, b] = ∂ℓ_k/∂θ_d, tvlgrad::score_value — instead of only summing it.  The 31
// live lanes of a group write 248 consecutive bytes per step; lane 15 is the padding direction and writes nothing.
// The columns outside a candidate's accumulated range 1 … nobs − 2 are written as exact zeros by the same lanes, so
// the array needs no memset.  What the gradient kernel learns only at the end — its own value or a tangent is not
// usable — makes the group write its columns again, as NaN (rare), and raises flags[5] as the gradient kernel does.
//
// A sibling of tvl_grad_kernel, not a second instantiation of one body: that kernel sits at 256 VGPRs with nothing to
// spare, and its code object is not to move.  Everything the store needs — the candidate, the address, dconst, the
// chain factor — is formed at the store from the block index, a fresh lane index and LDS, so nothing more is carried
// across the step loop than there.
#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_tvl_grad_map.hpp"

namespace yfm {

// L lanes per candidate, ND directions per lane.  Y, prep: as in tvl_grad_kernel.  scores: P × (T − 1) × B
// column-major.  Dynamic LDS: N × (m, 1/m), then per group 100 doubles and a Model.
template <int L, int ND>
__global__ __launch_bounds__(kTvlGradBlock) void tvl_score_kernel(const double* __restrict__ theta, int P, int B,
                                                                  int space, const double* __restrict__ Y,
                                                                  const double* __restrict__ prep, int ldp, int np,
                                                                  int T, int N, const double* __restrict__ mats,
                                                                  const int* __restrict__ T_use,
                                                                  const double* __restrict__ ll,
                                                                  double* __restrict__ scores,
                                                                  unsigned int* __restrict__ n_unavailable) {
  namespace g = tvlgrad;
  static_assert(L == 32 && ND == 1, "one direction per lane: a step's 31 scores are one contiguous store");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  double2* s_mr = reinterpret_cast<double2*>(smem);  // (m_i, 1/m_i)
  double* s_linv = smem + 2 * N;                     // per group: the 10×10 inverse Lyapunov operator
  constexpr int GPB = kTvlGradBlock / L;
  g::Model* smodel0 = reinterpret_cast<g::Model*>(s_linv + 100 * GPB);  // per group: the decoded θ
  g::Model* smodel = smodel0 + tid / L;
  const int j = tid % L;
  const int b = (int)(((size_t)blockIdx.x * kTvlGradBlock + tid) / L);
  const bool live = b < B;
  const int bb = live ? b : B - 1;  // a group past B mirrors the last candidate and writes nothing
  const int nobs = min(max(T_use ? T_use[bb] : T, 1), T);
  const double* th = theta + (size_t)bb * P;
  const double llb = ll[bb];
  const bool avail = llb - llb == 0.0;  // finite: −Inf and NaN logliks have no scores

  for (int i = tid; i < N; i += kTvlGradBlock) {
    const double m = mats[i];
    s_mr[i] = make_double2(m, 1.0 / m);
  }
  __syncthreads();

  // the decoded parameters and the inverse Lyapunov operator in LDS, one copy per group (tvl_grad_kernel)
  {
    g::Model mreg;
    g::decode(th, space, mreg);
    if (j == 0) *smodel = mreg;
    wave_lds_sync();
  }
  const g::Model& m = *smodel;  // before the step loop; inside it, `mk` below
  double* Linv = s_linv + (tid / L) * 100;
  for (int c = j; c < 10; c += L) {
    double colv[10];
    g::lyapunov_inverse_column(m.Phi, c, colv);
#pragma unroll
    for (int r = 0; r < 10; ++r) Linv[r * 10 + c] = colv[r];
  }
  wave_lds_sync();
  g::State s;
  g::Tangent t[ND];
  g::seed(g::slot_direction(L, 0, j), t[0]);
  g::init_state<ND>(m, Linv, s, t);

  double l_minm = __builtin_inf();  // this lane's smallest maturity (the λ-overflow test of step_consts)
  for (int i = j; i < N; i += L) l_minm = fmin(l_minm, s_mr[i].x);

  // filter! over columns 0 .. nobs − 2 (filter.jl:190); the group's lanes share nobs
  for (int k = 0; k + 1 < nobs; ++k) {
    const bool nan_col = prep[(size_t)k * ldp + np + 2] != 0.0;
    const bool acc = k >= 1;  // Julia t > 1 (filter.jl:194)
    // the fences of tvl_grad_kernel: the parameters and the seeds are formed where a step uses them
    int goff = (tid / L) * (int)sizeof(g::Model);
    asm volatile("" : "+v"(goff));
    const g::Model& mk = *reinterpret_cast<const g::Model*>(reinterpret_cast<const char*>(smodel0) + goff);
    {
      int d = t[0].d;
      asm volatile("" : "+v"(d));
      t[0].d = d;
    }
    const double* col = Y + (size_t)k * N;
    g::StepConst kc;
    g::step_consts(s.beta, l_minm, kc);
    g::Moments mo;
    g::moments_zero(mo);
#pragma unroll 1
    for (int i = fresh_group_lane<L>(); i < N; i += L) {
      const double2 mr = s_mr[i];
      g::accum(kc, s.beta, mr.x, mr.y, exp(-(kc.lam * mr.x)), col[i], mo);
    }
#pragma unroll
    for (int q = 0; q < g::NSTAT; ++q) {
      mo.s[q] = group_sum<L>(mo.s[q]);
      mo.j3[q] = group_sum<L>(mo.j3[q]);
    }
#pragma unroll
    for (int q = 0; q < g::NJ; ++q) {
      mo.j1[q] = group_sum<L>(mo.j1[q]);
      mo.j2[q] = group_sum<L>(mo.j2[q]);
    }
    g::Step u;
    g::primal_update(mk, s, mo, N, u);
    g::Filtered f;
    g::filtered_state(mk, s, u, nan_col, f);
    g::tangent_step<tvl_slot_mask<L, 0>()>(mk, s, u, mo, N, f, nan_col, t[0], acc);
    g::primal_step(mk, u, f, nan_col, s, acc);

    // this step's term of this lane's direction: column k of the candidate's scores.  The candidate, its θ and the
    // address are formed here, behind a fence of their own, from the block index and the thread index.
    {
      int tf = tid;
      asm volatile("" : "+v"(tf));
      const int bs = (int)(((size_t)blockIdx.x * kTvlGradBlock + tf) / L);
      const int d = t[0].d;
      if (bs < B && d < g::kNP) {
        const double v = g::score_value(mk, t[0], N, acc) * g::chain_factor(theta + (size_t)bs * P, space, d) + 0.0;
        scores[((size_t)bs * (T - 1) + k) * P + d] = avail ? v : __builtin_nan("");
      }
    }
  }

  // this lane's gradient entry; the candidate's scores are kept only when every one of them is finite (the
  // gradient kernel's rule)
  const int je = fresh_group_lane<L>();
  const int d = g::slot_direction(L, 0, je);
  const double gv = g::grad_value(m, t[0], N, nobs) * g::chain_factor(theta + (size_t)bb * P, space, d) + 0.0;
  const bool fin = d >= g::kNP || g::finite(gv);
  const bool own_ok = g::primal_ok(m, s, N, nobs) && group_sum<L>(fin ? 0.0 : 1.0) == 0.0;
  if (!live) return;
  const int ncol = T - 1;
  double* const out = scores + (size_t)b * P * ncol;
  const bool keep = avail && own_ok;
  if (je == 0 && avail && !own_ok) atomicAdd(n_unavailable, 1u);
  if (d >= g::kNP) return;
  // the columns past the window: exact zeros; all of them NaN for a candidate without scores
  const double fill = keep ? 0.0 : __builtin_nan("");
  for (int k = keep ? max(nobs - 1, 0) : 0; k < ncol; ++k) out[(size_t)k * P + d] = fill;
}

namespace {
constexpr int kTvlScoreLanes = 32, kTvlScoreDirs = 1;
}

hipError_t launch_tvl_scores(const LaunchArgs& a, const double* ll, double* scores, int b0, int nb) {
  if (nb <= 0 || a.T < 2) return hipSuccess;
  if (a.N > tvl_grad_max_n() || a.N < 1 || a.P != tvlgrad::kNP || !a.raw || !a.panel) return hipErrorInvalidValue;
  constexpr int per_block = kTvlGradBlock / kTvlScoreLanes;
  const int grid = (nb + per_block - 1) / per_block;
  const size_t shmem = sizeof(double) * (2 * (size_t)a.N + 100 * per_block) + sizeof(tvlgrad::Model) * per_block;
  hipLaunchKernelGGL((tvl_score_kernel<kTvlScoreLanes, kTvlScoreDirs>), dim3(grid), dim3(kTvlGradBlock), shmem,
                     a.stream, a.theta + (size_t)b0 * a.P, a.P, nb, a.space, a.raw, a.panel, a.ldp, a.np, a.T, a.N,
                     a.mats, a.T_use ? a.T_use + b0 : nullptr, ll + b0, scores, a.flags + 5);
  return hipGetLastError();
}

}  // namespace yfm
