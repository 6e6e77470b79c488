// yfm_smooth.hip — the backward sweep of the fixed-interval Kalman smoother (gfx950, MI355X) for the fixed-loading
// models DNS (M = 3) and GNS5 (M = 5): β̂_t = E[β_t | y_1..n], V_t and the lag-one covariance C_t (include/yfm.h
// yfm_smooth_batch).  An extension: the reference's predict returns the forecasts a_{t+1|t} only.
//
// The forward pass is the trajectory launch of yfm_filter_states: its record holds a_2 … a_n and P_2 … P_n, the
// predicted moments the sweep needs; a_1 and P_1 are formed here (yfm_smooth.hpp init_mean, InitCov).
//
// smooth_kernel: one wave per candidate, the chunked sweep of yfm_smooth_sweep.hpp (its phases 1 to 3 below), the
// algebra of yfm_smooth.hpp.  What is this kernel's own:
//   phase 1: Z'y_t over the N maturities (Z from LDS, broadcast), the solve with B_t, then s_t, W_t, L_t, P_{t|t}; of
//     a_{t|t} only u_t = Z'y_t − σ²s_t (a_t at a missing column) is formed, and kept across the chain;
//   phase 3: a_{t|t} = G⁻¹u_t (G⁻¹ from LDS), taken there because the chain's registers are free.
// Unavailable, beside an output that is not finite: a loglik that is not finite (−Inf, or NaN where initialize_filter
// throws) and a candidate on the deferral list (`skip`).
#include <algorithm>
#include <type_traits>

#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_smooth_sweep.hpp"

namespace yfm {

using smooth::fill_nan;
using smooth::kSmoothChunk;

// theta: P × nb; ll: nb logliks of the forward launch; skip: nb marks (deferred candidates); rec_beta / rec_P: the
// forward record, M (× M) × rec_len × nb, slot t − 2 = a_t, P_t; outputs M × T × nb, M × M × T × nb, M × M × (T − 1) × nb
template <int M>
__global__ __launch_bounds__(64) void smooth_kernel(const double* __restrict__ theta, int P, int nb, int space,
                                                    const double* __restrict__ raw, int N, int T,
                                                    const double* __restrict__ mats, const int* __restrict__ T_use,
                                                    const double* __restrict__ ll,
                                                    const unsigned char* __restrict__ skip,
                                                    const double* __restrict__ rec_beta,
                                                    const double* __restrict__ rec_P, int rec_len,
                                                    double* __restrict__ beta_s, double* __restrict__ V_s,
                                                    double* __restrict__ C_s, unsigned int* __restrict__ flags) {
  namespace sm = smooth;
  __shared__ double zs[64 * M];                               // Z, row i at zs[i M …]
  __shared__ double init_lds[sm::InitCov<M>::kDoubles];       // the P_1 system
  __shared__ double ops[sm::smooth_ops<M>() * kSmoothChunk];  // the sweep's s, W, L
  __shared__ double gis[M * M];                               // G⁻¹, row-major

  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= nb) return;
  const int n = min(max(T_use ? T_use[b] : T, 1), T);
  double* const bo = beta_s + (size_t)b * M * T;
  double* const Vo = V_s + (size_t)b * M * M * T;
  double* const Co = C_s ? C_s + (size_t)b * M * M * (size_t)max(T - 1, 0) : nullptr;
  const double llb = ll[b];
  if (!(llb - llb == 0.0) || skip[b]) {  // the whole wave
    fill_nan<M>(bo, Vo, Co, 0, T, lane);
    if (lane == 0) atomicAdd(flags + 5, 1u);
    return;
  }

  sm::Model<M> m;
  sm::decode<M>(theta + (size_t)b * P, space, m);
  {
    double z[M];
    sm::loading_row<M>(m, mats[min(lane, N - 1)], z);
#pragma unroll
    for (int k = 0; k < M; ++k) zs[lane * M + k] = lane < N ? z[k] : 0.0;
  }
  wave_lds_sync();
  double G[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) G[i][j] = 0.0;
  for (int i = 0; i < N; ++i) {
    double z[M];
#pragma unroll
    for (int k = 0; k < M; ++k) z[k] = zs[i * M + k];
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
      for (int k = j; k < M; ++k) G[j][k] = fma(z[j], z[k], G[j][k]);
  }
#pragma unroll
  for (int j = 0; j < M; ++j)
#pragma unroll
    for (int k = j + 1; k < M; ++k) G[k][j] = G[j][k];

  {  // G⁻¹ for the filtered mean: wave-uniform, formed once and read from LDS as broadcasts
    double Ginv[M * M];
    sm::gram_inverse<M>(G, Ginv);
#pragma unroll
    for (int k = 0; k < M * M; ++k)
      if (lane == 0) gis[k] = Ginv[k];
  }
  wave_lds_sync();

  double a1[M], P1[M][M];
  bool ok = sm::init_mean<M>(m, a1);
  ok = sm::InitCov<M>::solve(m, init_lds, lane, 64, [] { wave_lds_sync(); }, P1) && ok;

  double r[M], Nm[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    r[i] = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) Nm[i][j] = 0.0;
  }

  const size_t rb = (size_t)b * (size_t)rec_len;
  for (int c = (n - 1) / kSmoothChunk; c >= 0; --c) {
    const int t0 = kSmoothChunk * c + 1;  // the chunk's first column (1-based)
    const int t = t0 + lane;
    const bool act = t <= n;
    const int tt = act ? t : n;  // an idle lane repeats the window's last column and stores nothing
    // 1. this column's operands
    double a[M], Pm[M][M];
    if (tt == 1) {
#pragma unroll
      for (int i = 0; i < M; ++i) {
        a[i] = a1[i];
#pragma unroll
        for (int j = 0; j < M; ++j) Pm[i][j] = P1[i][j];
      }
    } else {
      sm::record_moments<M>(rec_beta, rec_P, rb + (size_t)(tt - 2), a, Pm);
    }
    double zy[M];
#pragma unroll
    for (int k = 0; k < M; ++k) zy[k] = 0.0;
    bool missing = false;
    const double* ycol = raw + (size_t)(tt - 1) * N;
    for (int i = 0; i < N; ++i) {
      const double y = ycol[i];
      missing = missing || (y != y);
#pragma unroll
      for (int k = 0; k < M; ++k) zy[k] = fma(zs[i * M + k], y, zy[k]);
    }
    sm::StepOps<M> o;
    sm::step_operands_core<M>(m, G, a, Pm, zy, missing, o);
    sm::store_operands<M>(ops, lane, o);
    // a_{t|t} waits for phase 3, where the chain's registers are free: a (missing column) or G a_{t|t} until then
    double af[M];
#pragma unroll
    for (int i = 0; i < M; ++i) af[i] = missing ? a[i] : o.u[i];
    wave_lds_sync();
    // 2. the chain over the chunk's columns, last to first; this lane keeps r_t, N_t of its own column
    double rt[M], Nt[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      rt[i] = 0.0;
#pragma unroll
      for (int j = 0; j < M; ++j) Nt[i][j] = 0.0;
    }
    for (int j = min(n - t0, kSmoothChunk - 1); j >= 0; --j) {
      const bool mine = j == lane;
      double s[M], W[M][M], L[M][M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        rt[i] = mine ? r[i] : rt[i];
        s[i] = ops[kSmoothChunk * i + j];
#pragma unroll
        for (int k = 0; k < M; ++k) {
          Nt[i][k] = mine ? Nm[i][k] : Nt[i][k];
          W[i][k] = ops[kSmoothChunk * (M + i * M + k) + j];
          L[i][k] = ops[kSmoothChunk * (M + M * M + i * M + k) + j];
        }
      }
      sm::chain_step<M>(s, W, L, r, Nm);
    }
    wave_lds_sync();  // the next chunk overwrites the operands
    // 3. this column's outputs
    const bool lag = act && t < n;
    double Pn[M][M];
    {
      const double* pp = rec_P + (rb + (size_t)(lag ? t - 1 : 0)) * M * M;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) Pn[i][j] = lag ? pp[j * M + i] : 0.0;
    }
    {  // af holds a_t (missing column) or u_t = G a_{t|t} since phase 1
      double ga[M];
#pragma unroll
      for (int i = 0; i < M; ++i) ga[i] = af[i];
      sm::filtered_mean<M>(gis, ga, ga, missing, af);
    }
    double bs[M], V[M][M], C[M][M];
    const bool fin = sm::step_outputs<M>(m, af, o.Pf, rt, Nt, lag, Pn, bs, V, C);
    ok = ok && (fin || !act);
    if (act) {
#pragma unroll
      for (int i = 0; i < M; ++i) {
        bo[(size_t)(t - 1) * M + i] = bs[i];
#pragma unroll
        for (int j = 0; j < M; ++j) Vo[((size_t)(t - 1) * M + j) * M + i] = V[i][j];
      }
      if (Co && lag) {
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
          for (int j = 0; j < M; ++j) Co[((size_t)(t - 1) * M + j) * M + i] = C[i][j];
      }
    }
  }
  // an output that is not finite anywhere makes the candidate unavailable: all of it NaN
  const bool bad = sm::raise_unavailable(ok, lane, flags);
  fill_nan<M>(bo, Vo, Co, bad ? 0 : n, T, lane);
}

// skip[b] = 1 for the candidates of the forward launch's deferral list (skip is zeroed before)
__global__ void smooth_mark_deferred_kernel(const int* __restrict__ defer_list, const unsigned int* __restrict__ flags,
                                            int nb, unsigned char* __restrict__ skip) {
  const unsigned int nd = min(flags[2], (unsigned int)nb);
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += gridDim.x * blockDim.x) {
    const int b = defer_list[i];
    if (b >= 0 && b < nb) skip[b] = 1;
  }
}

int smooth_max_n() { return 64; }

hipError_t launch_smooth(int kind, const LaunchArgs& a, const double* ll, unsigned char* skip, double* beta_s,
                         double* V_s, double* C_s) {
  if (a.B <= 0) return hipSuccess;
  if (a.N < 1 || a.N > smooth_max_n() || !a.defer_list || (a.T > 1 && (!a.rec_beta || !a.rec_P)))
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(skip, 0, (size_t)a.B, a.stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(smooth_mark_deferred_kernel, dim3(std::min((a.B + 255) / 256, 64)), dim3(256), 0, a.stream,
                     a.defer_list, a.flags, a.B, skip);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  auto launch = [&](auto m) {
    hipLaunchKernelGGL(smooth_kernel<decltype(m)::value>, dim3(a.B), dim3(64), 0, a.stream, a.theta, a.P, a.B, a.space,
                       a.raw, a.N, a.T, a.mats, a.T_use, ll, skip, a.rec_beta, a.rec_P, a.rec_len, beta_s, V_s, C_s,
                       a.flags);
    return hipGetLastError();
  };
  if (kind == YFM_MODEL_GNS5) return launch(std::integral_constant<int, 5>{});
  if (kind == YFM_MODEL_DNS) return launch(std::integral_constant<int, 3>{});
  return hipErrorInvalidValue;
}

}  // namespace yfm
