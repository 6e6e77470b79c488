// yfm_grad.hip — batched gradient of the DNS log-likelihood for gfx950 (MI355X): the filter and its
// forward-mode tangents propagated together (yfm_grad.hpp carries the algebra and the reference lines).
//
// What it replaces: the ForwardDiff gradient of compute_loss that estimate! asks for
// (src/optimization.jl:367, TwiceDifferentiable(...; autodiff=:forward), through optimization.jl:10-23).
//
// Mapping: ONE CANDIDATE PER GROUP OF 8 LANES, 3 directions per lane (24 slots for the 20 parameters; the
// last four are zero-seeded padding).  Every lane repeats the 3×3 primal step and carries its own
// directions, so the recursion needs no cross-lane traffic.  Direction d = 8·slot + lane: slot 0 holds
// γ, σ² and the six U entries (seeds dR, dz̃, dσ², dQ), slot 1 the three δ and Φ₁₁ … Φ₂₂ (dδ, dΦ), slot 2
// the rest of Φ (slot_mask) — the seed kinds a slot can carry are compile-time, the seed values differ per lane, so the
// wave does not diverge.  The four panel contractions per step (Z'ỹ and (∂Z/∂γ)'ỹ) are split over the
// group's lanes — lane j owns the maturities i ≡ j (mod 8), at most 8 (N ≤ 64), loadings in VGPRs — and
// reduced with DPP butterflies (group_sum), as yfm_group.hip does.  Each lane writes its own rows of grad.
//
// The logliks come from the existing launch (yfm_capi.hip runs it first, on the same stream); a candidate whose
// loglik is −Inf or NaN gets NaN gradients here, and grad_unavailable_kernel then does the same for the
// candidates of that launch's deferral list (ill-conditioned Z'Z: their value comes from the double-double
// kernel, which has no tangents).
#include <algorithm>

#include "yfm_device.hpp"
#include "yfm_grad.hpp"
#include "yfm_grad_map.hpp"
#include "yfm_internal.hpp"

namespace yfm {

// L lanes per candidate, ND directions per lane
template <int L, int ND>
__global__ __launch_bounds__(kGradBlock) void dns_grad_kernel(const double* __restrict__ theta, int P, int B, int space,
                                                              const double* __restrict__ panel, int ldp, int np, int T,
                                                              int N, const double* __restrict__ mats,
                                                              const int* __restrict__ T_use,
                                                              const double* __restrict__ ll, double* __restrict__ grad_out) {
  namespace g = grad;
  static_assert(L * ND >= g::kNP, "a slot for every parameter");
  constexpr int kGradMPL = kGradMaxN / L;  // maturities per lane
  constexpr int kGradSlots = ND;
  const int tid = threadIdx.x;
  const int j = tid % L;
  const int b = (int)(((size_t)blockIdx.x * kGradBlock + tid) / L);
  const bool live = b < B;
  const int bb = live ? b : B - 1;  // a group past B mirrors the last candidate and writes nothing
  const int nobs = min(max(T_use ? T_use[bb] : T, 1), T);
  const double* th = theta + (size_t)bb * P;

  g::Common c;
  g::decode(th, space, c.m);

  // this lane's loadings and their γ-derivatives; Z'Z and its derivative by group reduction
  double Zl[kGradMPL][4];
  double gs[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, dgs[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kGradMPL; ++k) {
    const int i = j + k * L;
    const bool own = i < N;
    const double m = mats[own ? i : 0];
    double z1, z2, d1, d2;
    g::loadings(c.m.gam, m, z1, z2, d1, d2);
    Zl[k][0] = own ? z1 : 0.0;
    Zl[k][1] = own ? z2 : 0.0;
    Zl[k][2] = own ? d1 : 0.0;
    Zl[k][3] = own ? d2 : 0.0;
    g::gram_add(Zl[k][0], Zl[k][1], Zl[k][2], Zl[k][3], gs, dgs);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    gs[k] = group_sum<L>(gs[k]);
    dgs[k] = group_sum<L>(dgs[k]);
  }
  g::setup_common(c, gs, dgs, N);

  g::State s;
  g::Tangent t[kGradSlots];
  for_slots<ND>([&](auto sl) { g::seed<slot_mask<L, sl()>()>(c.m, sl() * L + j, t[sl()]); });
  g::init_state<kGradSlots>(c, s, t);

  // filter! over columns 0 .. nobs − 2 (filter.jl:190); the group's lanes share nobs
  for (int k = 0; k + 1 < nobs; ++k) {
    const double* col = panel + (size_t)k * ldp;
    double zc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < kGradMPL; ++q) {
      const int i = j + q * L;
      const double y = (i < N) ? col[i] : 0.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) zc[e] = fma(Zl[q][e], y, zc[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) zc[e] = group_sum<L>(zc[e]);
    const double ybar = col[np], ytt = col[np + 1];
    const bool nan_col = col[np + 2] != 0.0;
    const bool acc = k >= 1;  // Julia t > 1 (filter.jl:194)
    if (nan_col) {
      for_slots<ND>([&](auto sl) { g::tangent_nan_step<slot_mask<L, sl()>()>(c, s, t[sl()], acc); });
      g::primal_nan_step(c.m, s, acc);
    } else {
      const double z[2] = {zc[0], zc[1]}, dz[2] = {zc[2], zc[3]};
      g::Step u;
      double det, q;
      g::primal_update(c, s, z, dz, ybar, ytt, u, det, q);
      for_slots<ND>([&](auto sl) { g::tangent_data_step<slot_mask<L, sl()>()>(c, s, u, t[sl()], acc); });
      g::primal_predict(c.m, u.bf, u.Pf, s);
    }
  }

  if (!live) return;
  const double llb = ll[b];
  const bool avail = llb - llb == 0.0;  // finite: −Inf and NaN logliks have no gradient
#pragma unroll
  for (int sl = 0; sl < kGradSlots; ++sl) {
    const int d = sl * L + j;
    if (d < g::kNP) {
      const double v = g::grad_value(c, t[sl], nobs) * g::chain_factor(th, space, d) + 0.0;
      grad_out[(size_t)b * P + d] = avail ? v : __builtin_nan("");
    }
  }
}

// NaN gradients for the candidates of the loglik launch's deferral list, and their count into the
// launch's counter bank (flags[5], yfm_last_batch_grad_unavailable)
__global__ void grad_unavailable_kernel(const int* __restrict__ defer_list, const unsigned int* __restrict__ flags,
                                        int P, int B, double* __restrict__ grad_out, unsigned int* __restrict__ n_out) {
  const unsigned int nd = min(flags[2], (unsigned int)B);
  const size_t n = (size_t)nd * P;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const int bdef = defer_list[e / P];
    if (bdef >= 0 && bdef < B) grad_out[(size_t)bdef * P + e % P] = __builtin_nan("");
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = nd;
}

int grad_max_n() { return kGradMaxN; }

// the mapping in use (yfm_grad_map.hpp)
namespace {
constexpr int kGradLanes = YFM_GRAD_LANES, kGradDirs = YFM_GRAD_DIRS;
}

hipError_t launch_dns_grad(const LaunchArgs& a, const double* ll, double* grad_out) {
  if (a.B <= 0) return hipSuccess;
  if (a.N > grad_max_n() || a.P != grad::kNP || !a.defer_list) return hipErrorInvalidValue;
  constexpr int per_block = kGradBlock / kGradLanes;
  const int grid = (a.B + per_block - 1) / per_block;
  hipLaunchKernelGGL((dns_grad_kernel<kGradLanes, kGradDirs>), dim3(grid), dim3(kGradBlock), 0, a.stream, a.theta, a.P, a.B, a.space, a.panel,
                     a.ldp, a.np, a.T, a.N, a.mats, a.T_use, ll, grad_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int g2 = (int)std::min<size_t>(((size_t)a.B * a.P + 255) / 256, 256);
  hipLaunchKernelGGL(grad_unavailable_kernel, dim3(g2), dim3(256), 0, a.stream, a.defer_list, a.flags, a.P, a.B,
                     grad_out, a.flags + 5);
  return hipGetLastError();
}

}  // namespace yfm
