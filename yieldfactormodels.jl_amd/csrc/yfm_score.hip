// yfm_score.hip — what a maximum-likelihood estimate of the DNS model needs beyond θ̂ (gfx950, MI355X): the score
// series, the OPG / HAC information matrix and the Hessian of the log-likelihood (include/yfm.h
// yfm_loglik_scores_batch, yfm_loglik_info_batch).  An extension: the reference's estimate! returns no covariance.
//
// dns_score_kernel: dns_grad_kernel's recursion (yfm_grad.hip: one candidate per group of 8 lanes, 3 directions per
// lane, the functions of yfm_grad.hpp) that stores, after every step, each direction's share of the term get_loss adds
// there — S[d, k, b] = ∂ℓ_k/∂θ_d, grad::score_value — instead of only summing it.  The columns outside a candidate's
// accumulated range 1 … nobs − 2 are written as exact zeros by the same lanes, so the array needs no memset.
//
// opg_kernel (DNS, P = 20) and opg31_kernel (TVλ, P = 31; its scores come from yfm_tvl_score.hip), one body opg_body<P>:
// J_b = Γ₀ + Σ_ℓ w_ℓ (Γ_ℓ + Γ_ℓ'), Γ_ℓ = Σ_k s_k s_{k−ℓ}', one wave per candidate on
// v_mfma_f64_16x16x4_f64.  P is padded to 32: the tiles (0,0), (0,1), (1,1) are accumulated and the upper triangle
// is mirrored on the way out.  Operand layout (yfm_fixedz_mfma.hpp): A[i][k] in lane 16k + i, B[k][j] in lane 16k + j,
// D[(l >> 4) + 4q][l & 15] in element q of lane l.  A k-step is four time steps; the A fragment of tile r is S[16r +
// (l & 15), 4kk + (l >> 4)], and the B fragment of tile c has the same form, so at lag 0 the fragments serve both sides.
// At lag ℓ the shifted fragments S[·, 4kk + (l >> 4) − ℓ] are scaled by the Bartlett weight and enter once as B (Γ_ℓ)
// and once as A (Γ_ℓ').  Rows ≥ P and columns outside 0 … n − 1 are masked to zero.
//
// Hessian: fourth-order central differences of the exact gradient.  hessian_points_kernel writes the 4P perturbed θ of
// every candidate and the realised steps; the loglik launch and the kind's gradient kernel evaluate them (yfm_capi.hip);
// hessian_assemble_kernel forms D and ½(D + D'), NaN where any perturbed gradient or the candidate's own is unavailable.
#include <algorithm>

#include "yfm_device.hpp"
#include "yfm_grad.hpp"
#include "yfm_grad_map.hpp"
#include "yfm_internal.hpp"
#include "yfm_tvl_grad.hpp"

namespace yfm {

typedef double yfm_score_double4 __attribute__((ext_vector_type(4)));

// L lanes per candidate, ND directions per lane; scores: P × ncol × B column-major, ncol = T − 1
template <int L, int ND>
__global__ __launch_bounds__(kGradBlock) void dns_score_kernel(const double* __restrict__ theta, int P, int B, int space,
                                                               const double* __restrict__ panel, int ldp, int np, int T,
                                                               int N, const double* __restrict__ mats,
                                                               const int* __restrict__ T_use,
                                                               const double* __restrict__ ll,
                                                               double* __restrict__ scores) {
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
  const int ncol = T - 1;
  double* const out = scores + (size_t)bb * P * ncol;
  const double llb = ll[bb];
  const bool avail = llb - llb == 0.0;  // finite: −Inf and NaN logliks have no scores

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
    // this step's term, per direction: column k of the candidate's scores (each lane its own rows)
    if (live) {
#pragma unroll
      for (int sl = 0; sl < kGradSlots; ++sl) {
        const int d = sl * L + j;
        if (d < g::kNP) {
          const double v = g::score_value(c, t[sl], acc) * g::chain_factor(th, space, d) + 0.0;
          out[(size_t)k * P + d] = avail ? v : __builtin_nan("");
        }
      }
    }
  }

  if (!live) return;
  // the columns past the window: exact zeros (NaN for a candidate without scores)
  const double fill = avail ? 0.0 : __builtin_nan("");
  for (int k = max(nobs - 1, 0); k < ncol; ++k) {
#pragma unroll
    for (int sl = 0; sl < kGradSlots; ++sl) {
      const int d = sl * L + j;
      if (d < g::kNP) out[(size_t)k * P + d] = fill;
    }
  }
}

// NaN scores for the candidates b0 … b0 + nb − 1 of the loglik launch's deferral list (`scores` starts at candidate
// b0), and — count_out not null — the list's length into the launch's counter bank (flags[5])
__global__ void score_unavailable_kernel(const int* __restrict__ defer_list, const unsigned int* __restrict__ flags,
                                         int B, int b0, int nb, size_t per, double* __restrict__ scores,
                                         unsigned int* __restrict__ count_out) {
  const unsigned int nd = min(flags[2], (unsigned int)B);
  for (unsigned int i = blockIdx.y; i < nd; i += gridDim.y) {
    const int bdef = defer_list[i] - b0;
    if (bdef < 0 || bdef >= nb) continue;
    double* const o = scores + (size_t)bdef * per;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < per; e += (size_t)gridDim.x * blockDim.x)
      o[e] = __builtin_nan("");
  }
  if (count_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *count_out = nd;
}

namespace {

constexpr int kOpgWaves = 4;  // candidates (waves) per block

// the fragment of row tile r at k-step kk, shifted back by `lag` columns: S[16r + (lane & 15), 4kk + (lane >> 4) − lag],
// zero for a padding row and outside columns 0 … n − 1
template <int kOpgP>
__device__ __forceinline__ double opg_frag(const double* __restrict__ S, int n, int r, int kk, int lag, int lane) {
  const int row = 16 * r + (lane & 15);
  const int col = 4 * kk + (lane >> 4) - lag;
  const bool ok = row < kOpgP && col >= 0 && col < n;
  return ok ? S[(size_t)col * kOpgP + row] : 0.0;
}

// The body of both OPG kernels, 16 < kOpgP ≤ 32 rows padded to two 16-row tiles.  scores: kOpgP × ncol × B; grad:
// kOpgP × B, the candidates' own gradients; J: kOpgP × kOpgP × B.  One wave per candidate.  A candidate without a
// gradient (NaN there) gets NaN in all of J, whatever its window; `count` (may be null) is raised by the candidates
// with a NaN J.
template <int kOpgP>
__device__ __forceinline__ void opg_body(const double* __restrict__ scores, int ncol, int T, int B,
                                         const int* __restrict__ T_use, int lags, const double* __restrict__ grad,
                                         double* __restrict__ J, unsigned int* __restrict__ count) {
  static_assert(kOpgP > 16 && kOpgP <= 32, "two row tiles");
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kOpgWaves + (threadIdx.x >> 6);
  if (b >= B) return;  // the whole wave
  const int nobs = min(max(T_use ? T_use[b] : T, 1), T);
  const int n = min(max(nobs - 1, 0), ncol);  // columns 0 … nobs − 2 can hold a term (column 0 is zero)
  const double* S = scores + (size_t)b * kOpgP * ncol;
  const int nk = (n + 3) / 4;
  yfm_score_double4 a00 = {0.0, 0.0, 0.0, 0.0}, a01 = a00, a11 = a00;
  for (int kk = 0; kk < nk; ++kk) {
    const double f0 = opg_frag<kOpgP>(S, n, 0, kk, 0, lane), f1 = opg_frag<kOpgP>(S, n, 1, kk, 0, lane);
    a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, f0, a00, 0, 0, 0);
    a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, f1, a01, 0, 0, 0);
    a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(f1, f1, a11, 0, 0, 0);
  }
  // Γ_ℓ pairs column k ≥ ℓ + 1 with column k − ℓ ≥ 1: none once ℓ ≥ n − 1
  const int lmax = min(lags, n - 2);
  for (int lag = 1; lag <= lmax; ++lag) {
    const double w = 1.0 - (double)lag / ((double)lags + 1.0);
    for (int kk = lag / 4; kk < nk; ++kk) {
      const double f0 = opg_frag<kOpgP>(S, n, 0, kk, 0, lane), f1 = opg_frag<kOpgP>(S, n, 1, kk, 0, lane);
      const double g0 = w * opg_frag<kOpgP>(S, n, 0, kk, lag, lane), g1 = w * opg_frag<kOpgP>(S, n, 1, kk, lag, lane);
      a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, g0, a00, 0, 0, 0);  // w Γ_ℓ
      a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(g0, f0, a00, 0, 0, 0);  // w Γ_ℓ'
      a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(f0, g1, a01, 0, 0, 0);
      a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(g0, f1, a01, 0, 0, 0);
      a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(f1, g1, a11, 0, 0, 0);
      a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(g1, f1, a11, 0, 0, 0);
    }
  }
  const double gb = grad[(size_t)b * kOpgP];
  if (!(gb - gb == 0.0)) {
    const double nan = __builtin_nan("");
    a00 = a01 = a11 = yfm_score_double4{nan, nan, nan, nan};
  }
  if (count && lane == 0 && a00[0] != a00[0]) atomicAdd(count, 1u);  // J[0, 0]
  // the upper triangle (i ≤ j) of each tile, written to both sides: J is symmetric to the last bit
  double* const Jb = J + (size_t)b * kOpgP * kOpgP;
  const int cj = lane & 15;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ri = (lane >> 4) + 4 * q;
    if (ri <= cj) {  // tile (0,0): rows and columns 0 … 15
      Jb[(size_t)cj * kOpgP + ri] = a00[q];
      Jb[(size_t)ri * kOpgP + cj] = a00[q];
    }
    if (cj < kOpgP - 16) {  // tile (0,1): rows 0 … 15, columns 16 … kOpgP − 1
      Jb[(size_t)(16 + cj) * kOpgP + ri] = a01[q];
      Jb[(size_t)ri * kOpgP + 16 + cj] = a01[q];
    }
    if (ri <= cj && cj < kOpgP - 16) {  // tile (1,1): rows and columns 16 … kOpgP − 1
      Jb[(size_t)(16 + cj) * kOpgP + 16 + ri] = a11[q];
      Jb[(size_t)(16 + ri) * kOpgP + 16 + cj] = a11[q];
    }
  }
}

}  // namespace

// DNS: 20 rows (rows 20 … 31 of the second tile are padding)
__global__ __launch_bounds__(64 * kOpgWaves) void opg_kernel(const double* __restrict__ scores, int ncol, int T, int B,
                                                             const int* __restrict__ T_use, int lags,
                                                             const double* __restrict__ grad, double* __restrict__ J,
                                                             unsigned int* __restrict__ count) {
  opg_body<grad::kNP>(scores, ncol, T, B, T_use, lags, grad, J, count);
}

// TVλ: 31 rows (row 31 is padding); tile (1,1) holds 15 live rows
__global__ __launch_bounds__(64 * kOpgWaves) void opg31_kernel(const double* __restrict__ scores, int ncol, int T, int B,
                                                               const int* __restrict__ T_use, int lags,
                                                               const double* __restrict__ grad, double* __restrict__ J,
                                                               unsigned int* __restrict__ count) {
  opg_body<tvlgrad::kNP>(scores, ncol, T, B, T_use, lags, grad, J, count);
}

// The perturbed points of candidates 0 … B − 1: point 4(P b + i) + s is θ_b moved along e_i by +h, −h, +2h, −2h
// (s = 0 … 3); steps[2(P b + i) + {0, 1}] the realised differences up − dn of the h and the 2h pair.
__global__ void hessian_points_kernel(const double* __restrict__ theta, int P, int B, const int* __restrict__ T_use,
                                      double h, double* __restrict__ pts, int* __restrict__ pts_T_use,
                                      double* __restrict__ steps) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)B * P) return;
  const int b = (int)(e / P), i = (int)(e % P);
  const double* th = theta + (size_t)b * P;
  const double x = th[i];
  const double mv[4] = {x + h, x - h, x + 2.0 * h, x - 2.0 * h};
  for (int s = 0; s < 4; ++s) {
    double* o = pts + (4 * e + s) * P;
    for (int d = 0; d < P; ++d) o[d] = d == i ? mv[s] : th[d];
    if (pts_T_use) pts_T_use[4 * e + s] = T_use[b];
  }
  steps[2 * e] = mv[0] - mv[1];
  steps[2 * e + 1] = mv[2] - mv[3];
}

// H_b = ½(D + D'), row i of D the Richardson combination (4 c_h − c_2h)/3 of the central differences c of the gradient
// over the realised steps (with exact steps h and 2h: (8(g₊ − g₋) − (g₊₊ − g₋₋))/(12h)).  One block per candidate;
// all of H_b is NaN when any of the 4P perturbed gradients or the candidate's own (grad: P × B) is not finite, and
// such a candidate raises *count.
__global__ __launch_bounds__(256) void hessian_assemble_kernel(const double* __restrict__ pts_grad,
                                                               const double* __restrict__ steps,
                                                               const double* __restrict__ grad, int P, int B,
                                                               double* __restrict__ H, unsigned int* __restrict__ count) {
  const int b = blockIdx.x;
  const double* G = pts_grad + (size_t)b * 4 * P * P;  // [i][s][d]
  const double g0 = grad[(size_t)b * P];
  int bad = !(g0 - g0 == 0.0);
  for (int e = threadIdx.x; e < 4 * P * P; e += blockDim.x) {
    const double v = G[e];
    bad |= !(v - v == 0.0);
  }
  bad = __syncthreads_or(bad);
  if (bad && threadIdx.x == 0) atomicAdd(count, 1u);
  double* const Hb = H + (size_t)b * P * P;
  const double* st = steps + (size_t)b * 2 * P;
  for (int e = threadIdx.x; e < P * P; e += blockDim.x) {
    const int i = e / P, j = e % P;
    if (i > j) continue;
    auto D = [&](int r, int c) {  // ∂g_c/∂θ_r
      const double* Gr = G + (size_t)r * 4 * P;
      const double c1 = (Gr[c] - Gr[P + c]) / st[2 * r];
      const double c2 = (Gr[2 * P + c] - Gr[3 * P + c]) / st[2 * r + 1];
      return (4.0 * c1 - c2) / 3.0;
    };
    const double v = bad ? __builtin_nan("") : 0.5 * (D(i, j) + D(j, i));
    Hb[(size_t)j * P + i] = v;
    Hb[(size_t)i * P + j] = v;
  }
}

namespace {
constexpr int kScoreLanes = YFM_GRAD_LANES, kScoreDirs = YFM_GRAD_DIRS;
}

hipError_t launch_dns_scores(const LaunchArgs& a, const double* ll, double* scores, int b0, int nb, bool count) {
  if (nb <= 0 || a.T < 2) return hipSuccess;
  if (a.N > grad_max_n() || a.P != grad::kNP || !a.defer_list) return hipErrorInvalidValue;
  constexpr int per_block = kGradBlock / kScoreLanes;
  const int grid = (nb + per_block - 1) / per_block;
  hipLaunchKernelGGL((dns_score_kernel<kScoreLanes, kScoreDirs>), dim3(grid), dim3(kGradBlock), 0, a.stream,
                     a.theta + (size_t)b0 * a.P, a.P, nb, a.space, a.panel, a.ldp, a.np, a.T, a.N, a.mats,
                     a.T_use ? a.T_use + b0 : nullptr, ll + b0, scores);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t per = (size_t)a.P * (a.T - 1);
  const int gx = (int)std::min<size_t>((per + 255) / 256, 64);
  const int gy = std::min(a.B, 1024);
  hipLaunchKernelGGL(score_unavailable_kernel, dim3(gx, gy), dim3(256), 0, a.stream, a.defer_list, a.flags, a.B, b0, nb,
                     per, scores, count ? a.flags + 5 : nullptr);
  return hipGetLastError();
}

hipError_t launch_opg(int P, const double* scores, int T, int nb, const int* T_use, int lags, const double* grad,
                      double* J, unsigned int* count, hipStream_t s) {
  if (nb <= 0) return hipSuccess;
  if (P != grad::kNP && P != tvlgrad::kNP) return hipErrorInvalidValue;
  hipLaunchKernelGGL(P == grad::kNP ? opg_kernel : opg31_kernel, dim3((nb + kOpgWaves - 1) / kOpgWaves), dim3(64 * kOpgWaves), 0, s, scores, T - 1, T,
                     nb, T_use, lags, grad, J, count);
  return hipGetLastError();
}

hipError_t launch_hessian_points(const double* theta, int P, int nb, const int* T_use, double h, double* pts,
                                 int* pts_T_use, double* steps, hipStream_t s) {
  if (nb <= 0) return hipSuccess;
  const size_t n = (size_t)nb * P;
  hipLaunchKernelGGL(hessian_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, theta, P, nb, T_use, h,
                     pts, T_use ? pts_T_use : nullptr, steps);
  return hipGetLastError();
}

hipError_t launch_hessian_assemble(const double* pts_grad, const double* steps, const double* grad, int P, int nb,
                                   double* H, unsigned int* count, hipStream_t s) {
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(hessian_assemble_kernel, dim3(nb), dim3(256), 0, s, pts_grad, steps, grad, P, nb, H, count);
  return hipGetLastError();
}

}  // namespace yfm
