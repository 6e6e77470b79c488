// yfm_tvl_smooth.hip — the backward sweep of the TVλ model's extended Kalman smoother (gfx950, MI355X): β̂_t = E[β_t |
// y_1..n], V_t, the lag-one covariance C_t (include/yfm.h yfm_tvl_smooth_batch) of the model linearised once, at the
// forward pass's predicted states.  An extension: the reference's predict returns the forecasts a_{t+1|t} only.
//
// The forward pass is the TVλ trajectory launch of yfm_filter_states under the context's precision: its record holds
// a_2 … a_n and P_2 … P_n; a_1 and P_1 are formed here (yfm_smooth.hpp init_mean, InitCov<4>).
//
// tvl_smooth_kernel: one wave per candidate, the chunked sweep of yfm_smooth_sweep.hpp (its phases 1 to 3 below) at
// M = 4, the algebra of yfm_tvl_smooth.hpp.  What is this kernel's own is phase 1: from a_t, P_t of its column lane ℓ
// forms the loadings' constants at λ_t = 0.01 + e^{a₄,t} with the forward's function (tvlgrad::step_consts, its
// λ-overflow branch tested on the smallest maturity), runs the maturity loop — one exp per maturity, (m, 1/m) broadcast
// from LDS, the panel column read through the cache — for G_t, u_t and the missing flag, then the 4×4 update in its
// symmetric form for s_t, W_t, L_t, a_{t|t}, P_{t|t}.
// Unavailable, beside an output that is not finite: a loglik that is not finite, a singular initial state, a data
// column whose det(σ²I + P_tG_t) is not usable (tvlsmooth::det_usable: the gradient kernel's rule).
#include "yfm_device.hpp"
#include "yfm_internal.hpp"
#include "yfm_smooth_sweep.hpp"
#include "yfm_tvl_smooth.hpp"

namespace yfm {

using smooth::fill_nan;
using smooth::kSmoothChunk;

// theta: 31 × nb; ll: nb logliks of the forward launch; rec_beta / rec_P: the forward record, 4 (× 4) × rec_len × nb,
// slot t − 2 = a_t, P_t; outputs 4 × T × nb, 4 × 4 × T × nb, 4 × 4 × (T − 1) × nb.  Dynamic LDS: N × (m, 1/m).
__global__ __launch_bounds__(64) void tvl_smooth_kernel(const double* __restrict__ theta, int P, int nb, int space,
                                                        const double* __restrict__ raw, int N, int T,
                                                        const double* __restrict__ mats, const int* __restrict__ T_use,
                                                        const double* __restrict__ ll,
                                                        const double* __restrict__ rec_beta,
                                                        const double* __restrict__ rec_P, int rec_len,
                                                        double* __restrict__ beta_s, double* __restrict__ V_s,
                                                        double* __restrict__ C_s, unsigned int* __restrict__ flags) {
  namespace sm = smooth;
  namespace ts = tvlsmooth;
  namespace tg = tvlgrad;
  constexpr int M = 4;
  extern __shared__ __attribute__((aligned(16))) double tvl_smooth_dyn[];
  double2* const s_mr = reinterpret_cast<double2*>(tvl_smooth_dyn);  // (m_i, 1/m_i)
  __shared__ double init_lds[sm::InitCov<M>::kDoubles];               // the P_1 system
  __shared__ double ops[sm::smooth_ops<M>() * kSmoothChunk];          // the sweep's s, W, L

  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= nb) return;
  const int n = min(max(T_use ? T_use[b] : T, 1), T);
  double* const bo = beta_s + (size_t)b * M * T;
  double* const Vo = V_s + (size_t)b * M * M * T;
  double* const Co = C_s ? C_s + (size_t)b * M * M * (size_t)max(T - 1, 0) : nullptr;
  const double llb = ll[b];
  if (!(llb - llb == 0.0)) {  // the whole wave
    fill_nan<M>(bo, Vo, Co, 0, T, lane);
    if (lane == 0) atomicAdd(flags + 5, 1u);
    return;
  }

  double minm = __builtin_inf();
  for (int i = lane; i < N; i += 64) {
    const double mi = mats[i];
    s_mr[i] = make_double2(mi, 1.0 / mi);
    minm = fmin(minm, mi);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) minm = fmin(minm, __shfl_xor(minm, off, 64));
  wave_lds_sync();

  tg::Model gm;
  sm::Model<M> m;
  ts::decode(theta + (size_t)b * P, space, gm, m);
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
    sm::StepOps<M> o;
    {
      tg::StepConst kc;
      tg::step_consts(a, minm, kc);
      tg::Moments mo;
      ts::stats_zero(mo);
      bool missing = false;
      const double* ycol = raw + (size_t)(tt - 1) * N;
#pragma unroll 2
      for (int i = 0; i < N; ++i) {
        const double2 mr = s_mr[i];
        const double y = ycol[i];
        missing = missing || (y != y);
        ts::accum(kc, a, mr.x, mr.y, exp(-(kc.lam * mr.x)), y, mo);
      }
      const double det = ts::column_operands(gm, m, a, Pm, mo, N, missing, o);
      ok = ok && ts::det_usable(det, missing, tt);
    }
    sm::store_operands<M>(ops, lane, o);
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
    double bs[M], V[M][M], C[M][M];
    const bool fin = sm::step_outputs<M>(m, o.af, o.Pf, rt, Nt, lag, Pn, bs, V, C);
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
  // a column without a usable determinant or an output that is not finite makes the candidate unavailable
  const bool bad = sm::raise_unavailable(ok, lane, flags);
  fill_nan<M>(bo, Vo, Co, bad ? 0 : n, T, lane);
}

int tvl_smooth_max_n() { return tvl_max_n(); }

hipError_t launch_tvl_smooth(const LaunchArgs& a, const double* ll, double* beta_s, double* V_s, double* C_s) {
  if (a.B <= 0) return hipSuccess;
  if (a.N < 1 || a.N > tvl_smooth_max_n() || a.P != tvlgrad::kNP || !a.raw || !ll || !beta_s || !V_s ||
      (a.T > 1 && (!a.rec_beta || !a.rec_P || a.rec_len < a.T - 1)))
    return hipErrorInvalidValue;
  const size_t shmem = sizeof(double) * 2 * (size_t)a.N;
  hipLaunchKernelGGL(tvl_smooth_kernel, dim3(a.B), dim3(64), shmem, a.stream, a.theta, a.P, a.B, a.space, a.raw, a.N,
                     a.T, a.mats, a.T_use, ll, a.rec_beta, a.rec_P, a.rec_len, beta_s, V_s, C_s, a.flags);
  return hipGetLastError();
}

}  // namespace yfm
