// yfm_smooth_sweep.hpp — the chunked backward sweep of smooth_kernel<M> (yfm_smooth.hip: DNS, GNS5) and
// tvl_smooth_kernel (yfm_tvl_smooth.hip: TVλ, M = 4): the mapping, stated once, and the pieces of it that both kernels
// call.  Device code only.
//
// One wave per candidate.  The forward record holds a_2 … a_n and P_2 … P_n (M (× M) × rec_len × nb, slot t − 2 = a_t,
// P_t); a_1, P_1 come from the kernel (yfm_smooth.hpp init_mean, InitCov).  The window is cut into chunks of 64 columns
// (chunk c holds columns 64c + 1 … 64c + 64, whatever the window's end, so a column's lane and chunk do not depend on
// n) that are taken from the last to the first.  Per chunk
//   1. lane ℓ takes a_t, P_t of its column t = 64c + 1 + ℓ (a_1, P_1 or record_moments) and forms that column's
//      operands s_t, W_t, L_t and its filtered moments from them and the data alone — the kernel's own algebra, all 64
//      columns at once, every load issued before the recursion; s_t, W_t, L_t go to LDS operand-major (store_operands),
//      so the stores are conflict-free and the chain's reads are broadcasts;
//   2. every lane runs the short serial chain r_{t−1} = s_t + L_t'r_t, N_{t−1} = W_t + L_t'N_tL_t (chain_step) over the
//      chunk's columns on wave-uniform values (r and N stay in registers across chunks) and keeps r_t, N_t of its own
//      column as the chain passes it;
//   3. lane ℓ forms β̂_t, V_t and C_t of its column (step_outputs) and stores them.
// Slots past a candidate's window are written as NaN by the same wave, and all of an unavailable candidate's slots
// (fill_nan); such a candidate raises flags[5] (raise_unavailable).  No memset of the outputs is needed.
//
// Phase 2, the load of P_{t+1}, the column's stores and the zeroing of r, N are one text in both kernels and stay
// there: as functions they change the kernels' instruction streams (the rows "smoother sweep").
#pragma once
#include "yfm_device.hpp"
#include "yfm_smooth.hpp"

namespace yfm {
namespace smooth {

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

// a, P of a slot of the forward record (slot = b · rec_len + t − 2 for a_t, P_t), P transposed
template <int M>
__device__ __forceinline__ void record_moments(const double* rec_beta, const double* rec_P, size_t slot,
                                               double (&a)[M], double (&Pm)[M][M]) {
  const double* pa = rec_beta + slot * M;
  const double* pp = rec_P + slot * M * M;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    a[i] = pa[i];
#pragma unroll
    for (int j = 0; j < M; ++j) Pm[i][j] = pp[j * M + i];
  }
}

// s, W, L of this lane's column to LDS: operand k of column j at ops[64 k + j]
template <int M>
__device__ __forceinline__ void store_operands(double* ops, int lane, const StepOps<M>& o) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    ops[kSmoothChunk * i + lane] = o.s[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      ops[kSmoothChunk * (M + i * M + j) + lane] = o.W[i][j];
      ops[kSmoothChunk * (M + M * M + i * M + j) + lane] = o.L[i][j];
    }
  }
}

// After the last chunk: a lane that is not ok makes the candidate unavailable.  Returns that, the candidate counted.
__device__ __forceinline__ bool raise_unavailable(bool ok, int lane, unsigned int* flags) {
  const bool bad = __ballot(!ok) != 0ull;
  if (bad) {
    __threadfence();
    if (lane == 0) atomicAdd(flags + 5, 1u);
  }
  return bad;
}

}  // namespace smooth
}  // namespace yfm
