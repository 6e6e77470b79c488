// yfm_tvl_layout.hpp — the dynamic LDS of the two TVλ loglik kernels, stated once per kernel: the kernel walks the
// struct's regions and its launcher passes the struct's bytes(), so the two cannot disagree (a mismatch would be an
// out-of-bounds LDS write).  Also the columns-per-chunk rule of the launchers that stage panel chunks through registers.
// Plain integers, for the device, the host and tests/tvl_layout_host_check.cpp (the former chains and byte counts).
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YFM_LAYOUT_HD __host__ __device__ __forceinline__
#else
#define YFM_LAYOUT_HD inline
#endif

namespace yfm {

// columns per panel chunk: a block's prefetch registers hold pre_times_block doubles, a column takes `stride`; at
// most 32, and 0 where not even one fits (the launchers refuse)
inline int chunk_columns(int pre_times_block, int stride) {
  if (stride < 1) return 0;
  const int TC = pre_times_block / stride;
  return TC > 32 ? 32 : TC;
}

// jump tables of the TVλ exp recurrence (TvlGaps, yfm_internal.hpp)
constexpr int kTvlGaps = 8;
constexpr int kTvlPowGaps = 16;

// tvl_loglik_kernel<L, ·> (yfm_tvl.hip): the regions in address order from smem, lengths in doubles (gi: ints);
// GPB = 256 / L filters per block.  Lengths are methods, not members a constructor fills: evaluated where the kernel
// uses them they are the expressions it had inline, and its assembly is unchanged.
struct TvlSmem {
  int N, TC, GPB, L;
  YFM_LAYOUT_HD int mr() const { return 2 * N; }                    // (m_i, 1/m_i), N double2
  YFM_LAYOUT_HD int nan() const { return TC; }                      // TC NaN flags of the staged chunk
  YFM_LAYOUT_HD int y() const { return TC * N; }                    // TC columns of N yields (column-major, stride N)
  YFM_LAYOUT_HD int w() const { return GPB * kTvlGaps; }            // per group: e^{-λ d_k}, k < K (≤ kTvlGaps)
  YFM_LAYOUT_HD int xch() const { return L >= 4 ? GPB * 16 : 0; }   // per group: 4×4 exchange block (L ≥ 4)
  YFM_LAYOUT_HD int gi() const { return N; }                        // per maturity: gap index of the jump i → i + L (int)
  YFM_LAYOUT_HD size_t bytes() const { return 8 * (size_t)(mr() + nan() + y() + w() + xch()) + 4 * (size_t)gi(); }
};

// per-candidate dd record: σ², δ, Φ, Q — the read-only part staged in LDS per group (doubles)
constexpr int kDPar = 58;
// per-group jump factors e^{−λ d_k} in LDS: 17 dd (272 B) apart, so the 16 groups of a wave reading their own table
// hit disjoint banks (a power-of-two stride is a 4-way conflict)
constexpr int kDdJumps = kTvlPowGaps > kTvlGaps ? kTvlPowGaps : kTvlGaps;
constexpr int kDdWStride = kDdJumps + 1;
// per-group 4×4 dd exchange blocks 17 dd apart: at 16 dd (256 B = 64 banks) the 16 groups of a wave exchanging the
// same entry all hit the same banks — a 16-way conflict on every transpose
constexpr int kXchStride = 4 * 4 + 1;
constexpr int kSumDd = 2;  // dd column sums per staged column

// tvl_dd_loglik_kernel<L, ·, ·> (yfm_tvl_dd.hip): the regions in address order, lengths in doubles (w, xch: dd = two
// doubles; gi: ints); walked like TvlSmem.  The first two hold two tables each, split by the kernel at N and at TC.
struct TvlDdSmem {
  int N, TC, GPB, L;
  YFM_LAYOUT_HD int mats() const { return 3 * N; }                  // m_i (N), then 1/m_i (N dd)
  YFM_LAYOUT_HD int cols() const { return (1 + 2 * kSumDd) * TC; }  // per staged column: NaN flag (TC), then Σy, Σy² (dd)
  YFM_LAYOUT_HD int ymax() const { return TC; }                     // per staged column: max_i |y_i|
  YFM_LAYOUT_HD int y() const { return TC * N; }                    // TC columns of N yields
  YFM_LAYOUT_HD int par() const { return GPB * kDPar; }             // per group: σ², δ, Φ, Q
  YFM_LAYOUT_HD int w() const { return GPB * kDdWStride; }          // per group: e^{-λ d_k}, k < K (dd)
  YFM_LAYOUT_HD int xch() const { return GPB * kXchStride; }        // per group: 4×4 exchange block (dd)
  YFM_LAYOUT_HD int gi() const { return N; }                        // per maturity: its jump's index (int)
  YFM_LAYOUT_HD size_t bytes() const {
    return 8 * (size_t)(mats() + cols() + ymax() + y() + par() + 2 * w() + 2 * xch()) + 4 * (size_t)gi();
  }
};

}  // namespace yfm
