// yfm_msed_tree.hpp — the lane-group mapping's constants and its summation tree, shared by the λ kernels
// (yfm_msed.hip) and the neural kernels (yfm_msedn.hip).  DESIGN.md §3.6.
//
// One candidate per group of L lanes, L ∈ {4, 16}; lane j owns the maturities i ≡ j (mod L).  A candidate's sums do
// not depend on L: they are formed over 16 residue classes of the maturity index (class c holds i ≡ c mod 16, added
// in order of i) combined by one fixed tree — class bit 3 first, bit 0 last.  A lane forms the part of the tree
// over its own classes in registers (class_tree) and the group finishes it with true xor exchanges in descending
// order (group_sum_desc).
#pragma once
#include <hip/hip_runtime.h>

#include "yfm_tvl_layout.hpp"  // chunk_columns

namespace yfm {
namespace msedtree {

constexpr int kMsedBlock = 256;
constexpr int kMsedPre = 8;      // panel doubles prefetched per thread per chunk
constexpr int kMsedClasses = 16;  // residue classes of the summation tree (the largest L)

// x + (x of lane ^ 2^LVL): quad_perm for 1 and 2, ds_swizzle (the LDS crossbar, no memory) for 4, row_ror:8 for 8
template <int LVL>
__device__ __forceinline__ double xor_sum(double x) {
  const int lo = __double2loint(x), hi = __double2hiint(x);
  int plo, phi;
  if constexpr (LVL == 2) {
    constexpr int pat = (4 << 10) | 0x1f;  // bit-mask mode: and 0x1f, or 0, xor 4
    plo = __builtin_amdgcn_ds_swizzle(lo, pat);
    phi = __builtin_amdgcn_ds_swizzle(hi, pat);
  } else {
    constexpr int ctrl = LVL == 0 ? 0xB1 : LVL == 1 ? 0x4E : 0x128;
    plo = __builtin_amdgcn_mov_dpp(lo, ctrl, 0xf, 0xf, true);
    phi = __builtin_amdgcn_mov_dpp(hi, ctrl, 0xf, 0xf, true);
  }
  return x + __hiloint2double(phi, plo);
}

// the group's part of the tree: lane bits in descending order
template <int L>
__device__ __forceinline__ double group_sum_desc(double x) {
  if constexpr (L >= 16) x = xor_sum<3>(x);
  if constexpr (L >= 8) x = xor_sum<2>(x);
  if constexpr (L >= 4) x = xor_sum<1>(x);
  if constexpr (L >= 2) x = xor_sum<0>(x);
  return x;
}

// a lane's part: the classes that agree with c in the bits below 4 − K; the node's last addition joins the
// lowest of its free bits
template <int K, class S, class Leaf>
__device__ __forceinline__ void class_tree(int c, Leaf& leaf, S& s) {
  if constexpr (K == 0) {
    leaf(c, s);
  } else {
    S a, b;
    class_tree<K - 1>(c, leaf, a);
    class_tree<K - 1>(c | (kMsedClasses >> K), leaf, b);
    s.add(a, b);
  }
}

template <int L>
constexpr int log_classes_per_lane() {
  static_assert(L == 16 || L == 4, "lane counts the summation tree is built for");
  return L == 16 ? 0 : 2;
}

// columns per panel chunk: the prefetch registers hold ≤ kMsedPre·256 yields (0: N is out of range)
inline int chunk_columns(int N) { return yfm::chunk_columns(kMsedPre * kMsedBlock, N); }

}  // namespace msedtree
}  // namespace yfm
