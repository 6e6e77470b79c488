// yfm_msed_pass.hpp — what the λ kernels (yfm_msed.hip) and the neural kernels (yfm_msedn.hip, yfm_msedn_adj.hip)
// share beyond the summation tree: the panel staging, the loss epilogue, the neural kernels' statistics and their
// group-wide prepare, and the host's dispatch over kind and lane count.  Included by those three files only; the
// algebra headers (yfm_msed.hpp, yfm_msedn.hpp, yfm_msedn_adj.hpp) are also built for the host and do not see it.
//
// A device piece is here only if every kernel's assembly is unchanged with it (tools/isa_diff.py).  DESIGN.md §3.6a
// maps the pieces, names the ones that stay inline in the kernels and says which forms of them were tried.
#pragma once
#include "yfm_msedn.hpp"
#include "yfm_msed_tree.hpp"

namespace yfm {
namespace msedpass {

using namespace msedtree;

// ---- panel staging: chunk c holds the columns c·TC … c·TC + TC − 1 (CHY = TC·N doubles); zeros past the panel ----
// The kernels call these through one-line lambdas (load_chunk, store_chunk, stage_chunk): called directly, the same
// functions change every kernel (§3.6a).
// the λ kernels' form: chunk c in LDS, chunk c + 1 prefetched into registers
__device__ __forceinline__ void chunk_load(const double* __restrict__ Y, int c, int CHY, int T, int N, int tid,
                                           double (&pre)[kMsedPre]) {
  const size_t base = (size_t)c * CHY;
  const size_t lim = (size_t)T * N;
#pragma unroll
  for (int r = 0; r < kMsedPre; ++r) {
    const int e = r * kMsedBlock + tid;
    const size_t g = base + e;
    pre[r] = (e < CHY && g < lim) ? Y[g] : 0.0;
  }
}
__device__ __forceinline__ void chunk_store(double* s_y, int CHY, int tid, const double (&pre)[kMsedPre]) {
#pragma unroll
  for (int r = 0; r < kMsedPre; ++r) {
    const int e = r * kMsedBlock + tid;
    if (e < CHY) s_y[e] = pre[r];
  }
}
// the neural kernels' form: straight into LDS.  No register prefetch of the next chunk: a step there is thousands of
// instructions, so one exposed load per TC steps costs nothing, and the 16 registers are better spent on the score pass
__device__ __forceinline__ void chunk_stage(const double* __restrict__ Y, double* s_y, int c, int CHY, int T, int N,
                                            int tid) {
  const size_t base = (size_t)c * CHY;
  const size_t lim = (size_t)T * N;
#pragma unroll
  for (int r = 0; r < kMsedPre; ++r) {
    const int e = r * kMsedBlock + tid;
    const size_t g = base + e;
    if (e < CHY) s_y[e] = g < lim ? Y[g] : 0.0;
  }
}

// ---- epilogue: get_loss's value (filter.jl:242: nobs, not nobs − 1); −Inf, counted in flags[1], where it failed ----
__device__ __forceinline__ double finish_loss(double mse, double fN, int nobs, bool fail,
                                              unsigned int* __restrict__ flags) {
  double ll = mse / fN / (double)nobs;
  if (fail) {
    ll = -__builtin_inf();
    atomicAdd(&flags[1], 1u);
  }
  return ll;
}

// ---- the neural kernels' statistics ------------------------------------------------------------------------------
// NV sums through the tree
template <int NV>
struct Sums {
  double v[NV];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
  }
  __device__ __forceinline__ void add(const Sums& a, const Sums& b) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = a.v[k] + b.v[k];
  }
  template <int L>
  __device__ __forceinline__ void reduce() {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = group_sum_desc<L>(v[k]);
  }
};

// the statistics of an OLS pass, with the comparison's sum of squares
struct PassStats {
  double o[msed::NOLS];
  double vv;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < msed::NOLS; ++k) o[k] = 0.0;
    vv = 0.0;
  }
  __device__ __forceinline__ void add(const PassStats& a, const PassStats& b) {
#pragma unroll
    for (int k = 0; k < msed::NOLS; ++k) o[k] = a.o[k] + b.o[k];
    vv = a.vv + b.vv;
  }
};

// The statistics of pass A with Z'v of the comparison (yfm_msed.hpp, ∂loss/∂(δ, Φ)) through the same tree.
struct GradPassStats {
  PassStats s;
  double zv[msed::kM];
  __device__ __forceinline__ void zero() {
    s.zero();
#pragma unroll
    for (int k = 0; k < msed::kM; ++k) zv[k] = 0.0;
  }
  __device__ __forceinline__ void add(const GradPassStats& a, const GradPassStats& b) {
    s.add(a.s, b.s);
#pragma unroll
    for (int k = 0; k < msed::kM; ++k) zv[k] = a.zv[k] + b.zv[k];
  }
};

// Scal and (WITH_H) the score's data-free sums at the state's γ, by the whole group
template <int L, bool WITH_H>
__device__ __forceinline__ void prepare_group(msedn::State& st, bool anchored, const msedn::Ends& e, const double* s_m,
                                              int N, int j) {
  constexpr int NV = WITH_H ? msedn::NAUX : 1;
  msedn::anchors(st.gamma, anchored, e, st.sc);
  Sums<NV> sa;
  auto leaf = [&](int c, Sums<NV>& s) {
    s.zero();
    for (int i = c; i < N; i += kMsedClasses) msedn::accum_aux<WITH_H>(s.v, st.gamma, st.sc, i, N, s_m[i]);
  };
  class_tree<log_classes_per_lane<L>()>(j, leaf, sa);
  sa.template reduce<L>();
#pragma unroll
  for (int k = 0; k < NV; ++k) st.aux[k] = sa.v[k];
  msedn::finish_scale(st.aux[msedn::AQ], anchored, st.sc);
}

// ---- host dispatch ---------------------------------------------------------------------------------------------------
// the template arguments every kernel of both families takes, as a value a generic functor can receive
template <int LN, bool ST, bool HB, bool SC>
struct Variant {
  static constexpr int L = LN;
  static constexpr bool STATIC = ST, HASB = HB, SCALED = SC;
};
// f(Lanes<L>) for the tree's lane counts (a switch: through with_lanes_of nns_*_kernel's assembly moves)
template <class F>
hipError_t with_lanes(int lanes, F&& f) {
  switch (lanes) {
    case 4: return f(Lanes<4>{});
    case 16: return f(Lanes<16>{});
  }
  return hipErrorInvalidValue;
}

// f(Variant<L, STATIC, HASB, SCALED>) for a neural kind (the λ kinds' table is yfm_msed.hip's with_kind)
template <int L, class F>
hipError_t with_neural_kind(int kind, F&& f) {
  if (msedn::kind_static(kind)) return f(Variant<L, true, false, false>{});
  const bool hb = msedn::kind_has_b(kind), sc = msedn::kind_scaled(kind);
  if (hb && sc) return f(Variant<L, false, true, true>{});
  if (hb) return f(Variant<L, false, true, false>{});
  if (sc) return f(Variant<L, false, false, true>{});
  return f(Variant<L, false, false, false>{});
}

// blocks of kMsedBlock threads for B candidates at L lanes each
inline dim3 grid_blocks(int B, int L) {
  const int gpb = kMsedBlock / L;
  return dim3((B + gpb - 1) / gpb);
}

// shared memory of a neural kernel's block: the maturities, a panel chunk and per_group doubles for each of its groups
inline size_t neural_shmem(int L, int N, int TC, int per_group) {
  return sizeof(double) * ((size_t)N + (size_t)TC * N + (size_t)(kMsedBlock / L) * per_group);
}

}  // namespace msedpass
}  // namespace yfm
