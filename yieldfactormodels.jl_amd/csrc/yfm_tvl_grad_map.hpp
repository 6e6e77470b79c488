// yfm_tvl_grad_map.hpp — the lane mapping that the TVλ tangent kernels share (yfm_tvl_grad.hip, yfm_tvl_score.hip):
// one candidate per group of L lanes, ND directions per lane (tvlgrad::slot_direction).  Device only.
#pragma once
#include "yfm_grad_map.hpp"  // for_slots
#include "yfm_tvl_grad.hpp"

namespace yfm {

namespace {

constexpr int kTvlGradBlock = 256;

// the seed kinds of slot S when a candidate has L lanes (tvlgrad::slot_direction: which directions it holds)
template <int L, int S>
constexpr int tvl_slot_mask() {
  namespace g = tvlgrad;
  if (L >= 32) return g::kSeedAll;
  if (S >= g::slots_before_phi(L)) return g::kSeedF;
  constexpr int lo = S * L, hi = S * L + L - 1;
  return (lo <= 0 ? g::kSeedS : 0) | ((lo < g::kOffD && hi >= g::kOffU) ? g::kSeedQ : 0) |
         ((lo < g::kOffF && hi >= g::kOffD) ? g::kSeedD : 0);
}

// This lane's index in its group, formed afresh (the wave's lane count through an operand the compiler cannot fold):
// the step loop and the epilogue ask for it again, so the index is not carried in a register across the loop,
// where it was the one value that went to scratch.
template <int L>
__device__ __forceinline__ int fresh_group_lane() {
  static_assert(64 % L == 0 && kTvlGradBlock % 64 == 0, "a group lies inside one wave");
  unsigned z = 0u;
  asm volatile("" : "+v"(z));
  return (int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z)) & (unsigned)(L - 1));
}

}  // namespace

}  // namespace yfm
