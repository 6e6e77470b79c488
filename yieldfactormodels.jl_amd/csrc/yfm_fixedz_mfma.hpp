// yfm_fixedz_mfma.hpp — device-only pieces of the fixed-loading loglik kernels (yfm_kernels.hip; the chunk staging
// also serves yfm_split.hip): the panel chunk staging, and the DNS Z'ỹ block producers on the matrix cores.
// Uses MFMA builtins, so yfm_fixedz.hpp (which the host harness compiles) never includes it.
//
// Every function here is __forceinline__ and was moved out of fixedz_loglik_body with every kernel's assembly
// unchanged (tools/isa_diff.py); a piece that changed any kernel's assembly as a function stayed inline there.
// The layout comments travel with the code they describe.
#pragma once
#include "yfm_fixedz.hpp"

namespace yfm {

typedef double yfm_double4 __attribute__((ext_vector_type(4)));

constexpr int kFzTB = 16;  // steps per MFMA block
// z̃ scratch row stride (doubles) for NZ loading columns: one row of 64 candidates per step (+2: bank spread)
constexpr int fz_scratch_stride(int NZ) { return 64 * NZ + 2; }
// σ, the row permutation of the DNS fragments (see the 16×16×4 producers below)
constexpr int fz_sigma(int i) { return 4 * (i & 3) + (i >> 2); }

// ---- panel chunk staging: chunk c (CH doubles) of the prepared panel, PER doubles per thread of a BLOCK ----
template <int PER, int BLOCK>
__device__ __forceinline__ void chunk_load(const double* panel, size_t lim, int CH, int c, int tid,
                                           double* dst) {
  const size_t base = (size_t)c * CH;
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int e = r * BLOCK + tid;
    const size_t g = base + e;
    dst[r] = (e < CH && g < lim) ? panel[g] : 0.0;  // lim = T·ldp: zeros past the panel
  }
}
template <int PER, int BLOCK>
__device__ __forceinline__ void chunk_store(const double* src, int CH, int tid, double* buf) {
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const int e = r * BLOCK + tid;
    if (e < CH) buf[e] = src[r];
  }
}

// ---- step operands -----------------------------------------------------------------------------------------
// z̃ of a step from the operands zx read one step ahead (KTRIM: zx carries ỹ₂₈ of the step's column in element
// NZ, and the leftover term zd28·ỹ₂₈ is added when the step consumes them)
template <int NZ, bool KTRIM>
__device__ __forceinline__ void z_of(const double (&zd28)[KTRIM ? NZ : 1], const double (&zx)[NZ + (KTRIM ? 1 : 0)],
                                     double (&z)[NZ]) {
  if constexpr (KTRIM) {
    ktrim_leftover<NZ>(zd28, zx, z);
  } else {
#pragma unroll
    for (int j = 0; j < NZ; ++j) z[j] = zx[j];
  }
}

// ---- DNS: Z'ỹ of 16 steps on v_mfma_f64_16x16x4_f64 --------------------------------------------------------
// A fragments: tile r, k-step kk — lane l holds Z of pair p = 16r + σ(l & 15) (candidate p / 2 of this wave,
// column p % 2) at maturity 4kk + (l >> 4).  σ: row i = g + 4q of a tile holds pair 16r + 4g + q, so the four D
// values a lane holds (rows g, g+4, g+8, g+12 of one step) are four consecutive pairs — two 16-byte LDS stores
// per tile instead of four 8-byte ones, and still one candidate's z̃ in consecutive doubles for the step reads.
constexpr int kFzRGN = 4;  // row tiles accumulated at once (bounds live accumulators).  Two groups of 4, so the
// first group's z̃ stores overlap the second group's MFMAs (8: 0.2173 → 4: 0.2165 ms at config 2, 2: 0.2197 ms —
// two accumulator chains expose the MFMA latency; profiles/r4/ab9, ab10)
// The B operand bvk is formed by the caller (the staged panel columns of the block's 16 steps, B[k = maturity]
// [col = step]): formed inside the producers it changed the address arithmetic of the NP = 30 kernels.

// a D tile into the scratch: lane l holds step l & 15, pairs 16r + 4(l >> 4) + q (σ above)
template <int SS>
__device__ __forceinline__ void store_tile(double* dst, int lane, int r, const yfm_double4& a) {
  double* d = dst + (lane & 15) * SS + 16 * r + 4 * (lane >> 4);
  *reinterpret_cast<double2*>(d) = make_double2(a[0], a[1]);
  *reinterpret_cast<double2*>(d + 2) = make_double2(a[2], a[3]);
}

// plain tile groups of kFzRGN
template <int NRT, int NK>
__device__ __forceinline__ void zty_dns(const double (&Af)[NRT][NK], const double (&bvk)[NK], double* scr, int lane) {
  constexpr int SS = fz_scratch_stride(2), RGN = kFzRGN;
#pragma unroll
  for (int r0 = 0; r0 < NRT; r0 += RGN) {
    yfm_double4 acc[RGN];
#pragma unroll
    for (int r = 0; r < RGN; ++r) acc[r] = yfm_double4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
      for (int r = 0; r < RGN; ++r)
        acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[r0 + r][kk], bvk[kk], acc[r], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < RGN; ++r) store_tile<SS>(scr, lane, r0 + r, acc[r]);
  }
}

// IL (NP 29–32, 8 row tiles): three groups of 4, 2, 2 tiles, each group's stores interleaved with the next
// group's MFMAs: the first group's 8 stores during the second group's MFMAs, the second's 4 during the third's,
// so only the last 2 tiles' 4 stores trail the block.  Store s of a group (tile s >> 1, half s & 1) goes after a
// k-step of the next group: the first group's store s after k-step s, the second's after k-step 2s + 1 — with 7
// k-steps the last k-step takes the store that would have followed the eighth (two of the first group's, the
// second group's fourth)
constexpr bool fz_interleaved(int NRT, int NK) { return NRT == 2 * kFzRGN && (NK == 2 * kFzRGN || NK == 2 * kFzRGN - 1); }

template <int NRT, int NK>
__device__ __forceinline__ void zty_dns_interleaved(const double (&Af)[NRT][NK], const double (&bvk)[NK], double* scr,
                                                    int lane) {
  constexpr int SS = fz_scratch_stride(2), RGN = kFzRGN;
  constexpr int H = RGN / 2;
  constexpr int NS1 = 2 * RGN, NS2 = 2 * H;  // 16-byte stores of the first and the second group
  auto last1 = [](int kk) { return kk == NK - 1 ? NS1 : kk + 1; };  // first-group stores issued by k-step kk
  auto at2 = [](int s) { return 2 * s + 1 < NK - 1 ? 2 * s + 1 : NK - 1; };  // k-step of second-group store s
  yfm_double4 a1[RGN], a2[H], a3[H];
#pragma unroll
  for (int r = 0; r < RGN; ++r) a1[r] = yfm_double4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < H; ++r) a2[r] = a3[r] = yfm_double4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < NK; ++kk)
#pragma unroll
    for (int r = 0; r < RGN; ++r) a1[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[r][kk], bvk[kk], a1[r], 0, 0, 0);
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
#pragma unroll
    for (int r = 0; r < H; ++r)
      a2[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[RGN + r][kk], bvk[kk], a2[r], 0, 0, 0);
#pragma unroll
    for (int s = kk; s < last1(kk); ++s) {
      const int r1 = s >> 1, h = s & 1;
      double* d = scr + (lane & 15) * SS + 16 * r1 + 4 * (lane >> 4) + 2 * h;
      *reinterpret_cast<double2*>(d) = make_double2(a1[r1][2 * h], a1[r1][2 * h + 1]);
    }
  }
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
#pragma unroll
    for (int r = 0; r < H; ++r)
      a3[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[RGN + H + r][kk], bvk[kk], a3[r], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < NS2; ++s) {
      if (at2(s) == kk) {
        const int r2 = s >> 1, h = s & 1;
        double* d = scr + (lane & 15) * SS + 16 * (RGN + r2) + 4 * (lane >> 4) + 2 * h;
        *reinterpret_cast<double2*>(d) = make_double2(a2[r2][2 * h], a2[r2][2 * h + 1]);
      }
    }
  }
  __builtin_amdgcn_sched_group_barrier(0x008, RGN * NK, 0);  // the first group's MFMAs
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    __builtin_amdgcn_sched_group_barrier(0x008, H, 0);  // a k-step of the second group
#pragma unroll
    for (int s = kk; s < last1(kk); ++s) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // one store of the first
  }
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    __builtin_amdgcn_sched_group_barrier(0x008, H, 0);  // a k-step of the third group
#pragma unroll
    for (int s = 0; s < NS2; ++s)
      if (at2(s) == kk) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // one store of the second
  }
#pragma unroll
  for (int r = 0; r < H; ++r) store_tile<SS>(scr, lane, RGN + H + r, a3[r]);
}

// ---- GNS5 (two γ): Z'ỹ of 16 steps on v_mfma_f64_4x4x4_4b_f64 in the z-basis ------------------------------
// The MFMA rows are e_l = 1 − e^{−λ_l m} (one per γ) against the panel columns ỹ and ỹ/m, so a candidate holds
// 2 fragment rows instead of 4:
//   Σ S_l ỹ = (1/λ_l) Σ e_l ỹ/m,   Σ C_l ỹ = Σ (S_l − z_l) ỹ = Σ S_l ỹ + Σ e_l ỹ   (Σ ỹ = 0),
// which halves the fragment registers (the 5-state filter no longer spills).
// Block blk of an instruction is D[4×4] = A[4 pairs × 4 maturities]·B[4 maturities × 4 columns].  Operand lanes
// (tools/mfma_f64_4x4_probe.hip): A[blk][i][k] in lane 16k + 4blk + i — exactly the 16×16×4 A fragment (without
// σ) — B[blk][k][j] in lane 16k + 4blk + j (the same panel values for every block), D[blk][i][j] in lane
// 16i + 4blk + j.  512 flops per instruction at ≈17 cycles vs 2,048 at ≈144 for the 16×16×4 form at one wave per
// SIMD (profiles/r2/micro).
// The two producers of this form (plain, and software-pipelined over step pairs) stay inline in
// fixedz_loglik_body: every function form tried changed the GNS5 kernels' register allocation.

}  // namespace yfm
