// yfm_grad_map.hpp — the lane mapping that the DNS tangent kernels share (yfm_grad.hip, yfm_score.hip): one
// candidate per group of L lanes, ND directions per lane, direction d = L·slot + lane.  Device only.
#pragma once
#include <type_traits>

#include "yfm_grad.hpp"

namespace yfm {

namespace {

constexpr int kGradBlock = 256;
constexpr int kGradMaxN = 64;

// the seed kinds of slot S when a candidate has L lanes: its directions are S·L … S·L + L − 1
template <int L, int S>
constexpr int slot_mask() {
  constexpr int lo = S * L, hi = S * L + L - 1;
  return (lo <= 1 ? grad::kSeedG : 0) | ((lo <= 7 && hi >= 2) ? grad::kSeedQ : 0) |
         ((lo <= 10 && hi >= 8) ? grad::kSeedD : 0) | ((lo <= 19 && hi >= 11) ? grad::kSeedF : 0);
}
// f(integral_constant<int, S>) for S = 0 … ND − 1
template <int ND, int S = 0, class F>
__device__ __forceinline__ void for_slots(F&& f) {
  f(std::integral_constant<int, S>{});
  if constexpr (S + 1 < ND) for_slots<ND, S + 1>(f);
}

}  // namespace

// the mapping in use (tools/ab_build.py -DYFM_GRAD_LANES=16 -DYFM_GRAD_DIRS=2 builds the other one that fits)
#ifndef YFM_GRAD_LANES
#define YFM_GRAD_LANES 8
#define YFM_GRAD_DIRS 3
#endif

}  // namespace yfm
