// yfm_tvl_grad.hip — batched gradient of the TVλ extended-Kalman-filter log-likelihood for gfx950 (MI355X): the
// filter and its forward-mode tangents propagated together (yfm_tvl_grad.hpp carries the algebra and the reference
// lines).
//
// What it replaces: the ForwardDiff gradient of compute_loss that estimate! asks for
// (src/optimization.jl:367, TwiceDifferentiable(...; autodiff=:forward), through optimization.jl:10-23) on a
// TVλDNSModel (filter.jl:12-80).
//
// Mapping: ONE CANDIDATE PER GROUP OF L LANES, ND directions per lane (L·ND = 32 slots for the 31 parameters; one
// is zero-seeded padding); L = 32, ND = 1 is what is built.  Lane j of a group owns the maturities i ≡ j (mod L), as in tvl_loglik_kernel: per
// step it forms its share of the 14 statistics and of their 24 state derivatives (one exp per maturity; the panel
// column is read through the cache), and the group reduces the 38 sums with DPP butterflies (group_sum).  Every lane
// then repeats the 4×4 primal update and carries its own directions, so the recursion needs no other cross-lane
// traffic.  The 15 directions before Φ fill the first ⌈15/L⌉ slots, Φ's 16 the others (slot_direction), so the seed kinds a slot
// can carry are few and compile-time (tvl_slot_mask); the seed
// values differ per lane, so the wave does not diverge.  There is one mapping, whatever the batch: a candidate's
// gradient does not depend on the launch it sits in.
//
// The logliks come from the existing launch (yfm_capi.hip runs it first, on the same stream, under the context's
// precision); a candidate whose loglik is −Inf or NaN gets NaN gradients here.  A candidate whose loglik is finite
// but whose FP64 recursion here is not usable (its own value not finite, a negative determinant, a non-finite
// tangent) gets NaN gradients too and is counted in flags[5] (yfm_last_batch_grad_unavailable).
#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_tvl_grad_map.hpp"

namespace yfm {

// L lanes per candidate, ND directions per lane.  Y: the caller's raw N×T panel (column-major); prep: the prepared
// panel, read for its per-column NaN flags only (offset np + 2, stride ldp).  Dynamic LDS: N × (m, 1/m), then per
// group 100 doubles and a Model.
template <int L, int ND>
__global__ __launch_bounds__(kTvlGradBlock) void tvl_grad_kernel(const double* __restrict__ theta, int P, int B, int space,
                                                                 const double* __restrict__ Y,
                                                                 const double* __restrict__ prep, int ldp, int np, int T,
                                                                 int N, const double* __restrict__ mats,
                                                                 const int* __restrict__ T_use,
                                                                 const double* __restrict__ ll,
                                                                 double* __restrict__ grad_out,
                                                                 unsigned int* __restrict__ n_unavailable) {
  namespace g = tvlgrad;
  static_assert(L >= 32 ? ND == 1 : (ND - g::slots_before_phi(L)) * L >= 16, "a slot for every parameter");
  static_assert(L <= 32, "a group's butterflies stay inside its own rows: groups finish their windows independently");
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

  for (int i = tid; i < N; i += kTvlGradBlock) {
    const double m = mats[i];
    s_mr[i] = make_double2(m, 1.0 / m);
  }
  __syncthreads();

  // The decoded parameters live in LDS, one copy per group: they are the same in every lane, each use is a
  // broadcast read, and a U direction reads its row of U by address.  In registers next to the tangents the kernel
  // spilled.  (The fences inside the step loop keep the reads where they are used.)
  {
    g::Model mreg;
    g::decode(th, space, mreg);
    if (j == 0) *smodel = mreg;
    wave_lds_sync();
  }
  const g::Model& m = *smodel;  // before the step loop; inside it, `mk` below
  // the inverse of the initial state's Lyapunov operator, a column per lane (10 columns), shared through LDS
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
  for_slots<ND>([&](auto sl) { g::seed(g::slot_direction(L, sl(), j), t[sl()]); });
  g::init_state<ND>(m, Linv, s, t);

  double l_minm = __builtin_inf();  // this lane's smallest maturity (the λ-overflow test of step_consts)
  for (int i = j; i < N; i += L) l_minm = fmin(l_minm, s_mr[i].x);

  // filter! over columns 0 .. nobs − 2 (filter.jl:190); the group's lanes share nobs
  for (int k = 0; k + 1 < nobs; ++k) {
    const bool nan_col = prep[(size_t)k * ldp + np + 2] != 0.0;
    const bool acc = k >= 1;  // Julia t > 1 (filter.jl:194)
    // Loop-invariant values the compiler would otherwise hoist into registers for the whole loop — the parameters
    // (54 doubles) and each direction's seeds (pure functions of its index) — are made to look step-dependent: the
    // group's LDS offset and the direction indices pass through an empty asm, so the reads and the selects are
    // formed where a step uses them.  With them resident the kernel spilled to scratch.
    int goff = (tid / L) * (int)sizeof(g::Model);
    asm volatile("" : "+v"(goff));
    const g::Model& mk = *reinterpret_cast<const g::Model*>(reinterpret_cast<const char*>(smodel0) + goff);
#pragma unroll
    for (int sl = 0; sl < ND; ++sl) {
      int d = t[sl].d;
      asm volatile("" : "+v"(d));
      t[sl].d = d;
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
    // one path for both kinds of column (yfm_tvl_grad.hpp: selects keep the prediction on a NaN column)
    g::Step u;
    g::primal_update(mk, s, mo, N, u);
    g::Filtered f;
    g::filtered_state(mk, s, u, nan_col, f);
    for_slots<ND>(
        [&](auto sl) { g::tangent_step<tvl_slot_mask<L, sl()>()>(mk, s, u, mo, N, f, nan_col, t[sl()], acc); });
    g::primal_step(mk, u, f, nan_col, s, acc);
  }

  // this lane's gradient entries; the candidate's are kept only when every one of them is finite
  const int je = fresh_group_lane<L>();
  double gv[ND];
  bool fin = true;
#pragma unroll
  for (int sl = 0; sl < ND; ++sl) {
    const int d = g::slot_direction(L, sl, je);
    gv[sl] = g::grad_value(m, t[sl], N, nobs) * g::chain_factor(theta + (size_t)bb * P, space, d) + 0.0;
    fin = fin && (d >= g::kNP || g::finite(gv[sl]));
  }
  const bool own_ok = g::primal_ok(m, s, N, nobs) && group_sum<L>(fin ? 0.0 : 1.0) == 0.0;
  if (!live) return;
  const double llb = ll[b];
  const bool ll_fin = llb - llb == 0.0;  // finite: −Inf and NaN logliks have no gradient
#pragma unroll
  for (int sl = 0; sl < ND; ++sl) {
    const int d = g::slot_direction(L, sl, je);
    if (d < g::kNP) grad_out[(size_t)b * P + d] = (ll_fin && own_ok) ? gv[sl] : __builtin_nan("");
  }
  if (je == 0 && ll_fin && !own_ok) atomicAdd(n_unavailable, 1u);
}

int tvl_grad_max_n() { return tvl_max_n(); }

// The mapping in use: 32 lanes, one direction each (256 VGPR + 212 AGPR, no scratch).  The others the issue names
// do not fit the register file: built with -DYFM_TVL_GRAD_LANES=16 -DYFM_TVL_GRAD_DIRS=2 the kernel spills 57 VGPRs
// (232 B of scratch per lane), with 8 and 4 421 (1,512 B), so there was nothing to time against.
#ifndef YFM_TVL_GRAD_LANES
#define YFM_TVL_GRAD_LANES 32
#define YFM_TVL_GRAD_DIRS 1
#endif
namespace {
constexpr int kTvlGradLanes = YFM_TVL_GRAD_LANES, kTvlGradDirs = YFM_TVL_GRAD_DIRS;
}

hipError_t launch_tvl_grad(const LaunchArgs& a, const double* ll, double* grad_out) {
  if (a.B <= 0) return hipSuccess;
  if (a.N > tvl_grad_max_n() || a.N < 1 || a.P != tvlgrad::kNP || !a.raw || !a.panel) return hipErrorInvalidValue;
  constexpr int per_block = kTvlGradBlock / kTvlGradLanes;
  const int grid = (a.B + per_block - 1) / per_block;
  const size_t shmem = sizeof(double) * (2 * (size_t)a.N + 100 * per_block) +
                       sizeof(tvlgrad::Model) * per_block;
  hipLaunchKernelGGL((tvl_grad_kernel<kTvlGradLanes, kTvlGradDirs>), dim3(grid), dim3(kTvlGradBlock), shmem, a.stream,
                     a.theta, a.P, a.B, a.space, a.raw, a.panel, a.ldp, a.np, a.T, a.N, a.mats, a.T_use, ll, grad_out,
                     a.flags + 5);
  return hipGetLastError();
}

}  // namespace yfm
