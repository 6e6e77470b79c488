// yfm_smooth.hip — the backward sweep of the fixed-interval Kalman smoother (gfx950, MI355X) for the fixed-loading
// models DNS (M = 3) and GNS5 (M = 5): β̂_t = E[β_t | y_1..n], V_t and the lag-one covariance C_t (include/yfm.h
// yfm_smooth_batch).  An extension: the reference's predict returns the forecasts a_{t+1|t} only.
//
// The forward pass is the trajectory launch of yfm_filter_states: its record holds a_2 … a_n and P_2 … P_n, the
// predicted moments the sweep needs; a_1 and P_1 are formed here (yfm_smooth.hpp init_mean, InitCov).
//
// smooth_kernel: one wave per candidate, the algebra of yfm_smooth.hpp.  The window is cut into chunks of 64 columns
// (chunk c holds columns 64c + 1 … 64c + 64, whatever the window's end, so a column's lane and chunk do not depend on
// n) that are taken from the last to the first.  Per chunk
//   1. lane ℓ forms the operands of its column t = 64c + 1 + ℓ — Z'y_t over the N maturities (Z from LDS, broadcast),
//      the solve with B_t, then s_t, W_t, L_t, a_{t|t}, P_{t|t} — from the recorded moments and the data alone, all 64
//      columns at once, every load issued before the recursion, and writes s_t, W_t, L_t to LDS (operand-major, so
//      the stores are conflict-free and the chain's reads are broadcasts);
//   2. every lane runs the short serial chain r_{t−1} = s_t + L_t'r_t, N_{t−1} = W_t + L_t'N_tL_t over the chunk's
//      columns on wave-uniform values (r and N stay in registers across chunks) and keeps r_t, N_t of its own column
//      as the chain passes it;
//   3. lane ℓ forms a_{t|t} = G⁻¹u_t (G⁻¹ from LDS; u_t = Z'y_t − σ²s_t kept from phase 1), then β̂_t, V_t and C_t of its
//      column, and stores them.
// Slots past a candidate's window are written as NaN by the same wave, and all of an unavailable candidate's slots:
// a loglik that is not finite (−Inf, or NaN where initialize_filter throws), a candidate on the deferral list (`skip`),
// an output that is not finite.  Those candidates raise flags[5].  No memset of the outputs is needed.
#include <algorithm>

#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_smooth.hpp"

namespace yfm {

namespace {

constexpr int kSmoothChunk = 64;  // columns per chunk: one per lane

template <int M>
constexpr int smooth_ops() {
  return M + 2 * M * M;  // s, W, L per column
}

template <int M>
__device__ __forceinline__ void fill_nan(double* __restrict__ beta_s, double* __restrict__ V_s, double* __restrict__ C_s,
                                         int t_from, int T, int lane) {
  const double nan = __builtin_nan("");
  // slots t_from … T − 1 of β̂ and V (0-based), slots max(t_from − 1, 0) … T − 2 of C
  for (size_t e = (size_t)t_from * M + lane; e < (size_t)T * M; e += 64) beta_s[e] = nan;
  for (size_t e = (size_t)t_from * M * M + lane; e < (size_t)T * M * M; e += 64) V_s[e] = nan;
  if (C_s)
    for (size_t e = (size_t)max(t_from - 1, 0) * M * M + lane; e < (size_t)max(T - 1, 0) * M * M; e += 64) C_s[e] = nan;
}

}  // namespace

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
  constexpr int kOps = smooth_ops<M>();
  __shared__ double zs[64 * M];                       // Z, row i at zs[i M …]
  __shared__ double init_lds[sm::InitCov<M>::kDoubles];  // the P_1 system
  __shared__ double ops[kOps * kSmoothChunk];          // operand k of column j at ops[64 k + j]
  __shared__ double gis[M * M];                        // G⁻¹, row-major

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
      const double* pa = rec_beta + (rb + (size_t)(tt - 2)) * M;
      const double* pp = rec_P + (rb + (size_t)(tt - 2)) * M * M;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        a[i] = pa[i];
#pragma unroll
        for (int j = 0; j < M; ++j) Pm[i][j] = pp[j * M + i];
      }
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
    double af[M], Pf[M][M];
    {
      sm::StepOps<M> o;
      sm::step_operands_core<M>(m, G, a, Pm, zy, missing, o);
#pragma unroll
      for (int i = 0; i < M; ++i) {
        ops[kSmoothChunk * i + lane] = o.s[i];
#pragma unroll
        for (int j = 0; j < M; ++j) {
          Pf[i][j] = o.Pf[i][j];
          ops[kSmoothChunk * (M + i * M + j) + lane] = o.W[i][j];
          ops[kSmoothChunk * (M + M * M + i * M + j) + lane] = o.L[i][j];
        }
      }
      // a_{t|t} waits for phase 3, where the chain's registers are free: a (missing column) or G a_{t|t} until then
#pragma unroll
      for (int i = 0; i < M; ++i) af[i] = missing ? a[i] : o.u[i];
    }
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
    const bool fin = sm::step_outputs<M>(m, af, Pf, rt, Nt, lag, Pn, bs, V, C);
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
  const bool bad = __ballot(!ok) != 0ull;
  if (bad) {
    __threadfence();
    if (lane == 0) atomicAdd(flags + 5, 1u);
  }
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
  if (kind == YFM_MODEL_GNS5) {
    hipLaunchKernelGGL(smooth_kernel<5>, dim3(a.B), dim3(64), 0, a.stream, a.theta, a.P, a.B, a.space, a.raw, a.N, a.T,
                       a.mats, a.T_use, ll, skip, a.rec_beta, a.rec_P, a.rec_len, beta_s, V_s, C_s, a.flags);
  } else if (kind == YFM_MODEL_DNS) {
    hipLaunchKernelGGL(smooth_kernel<3>, dim3(a.B), dim3(64), 0, a.stream, a.theta, a.P, a.B, a.space, a.raw, a.N, a.T,
                       a.mats, a.T_use, ll, skip, a.rec_beta, a.rec_P, a.rec_len, beta_s, V_s, C_s, a.flags);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace yfm
