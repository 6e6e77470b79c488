// tvl_layout_host_check.cpp — TvlSmem and TvlDdSmem (csrc/yfm_tvl_layout.hpp) beside the pointer chains and the two
// byte-count formulas they replace, restated here as they stood in tvl_loglik_kernel / launch_tvl_l and
// tvl_dd_loglik_kernel / launch_tvl_dd_l.  A stand-alone host program (tests/test_tvl_layout_host_cpu.py builds it
// with the address and undefined-behaviour sanitizers): per case the totals are equal, every region starts where
// the former chain put it, the double2 / dd regions are 16-byte aligned wherever the former chain had them so, and
// the regions are disjoint and inside the total.  Prints one line per precision and exits non-zero on a failure.
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "../yieldfactormodels.jl_amd/csrc/yfm_tvl_layout.hpp"

using namespace yfm;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::printf("FAIL %s: ", #cond);            \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      ++failures;                                 \
    }                                             \
  } while (0)

// stands for the workgroup's LDS (160 KiB, 16-byte aligned as the kernels declare smem); never read or written
alignas(16) static double lds[160 * 1024 / sizeof(double)];

struct Region {
  const char* name;
  size_t begin, bytes;  // byte offset from smem, length
  bool pair;            // holds double2 / dd: 16-byte accesses
};

// the regions in address order: disjoint, inside `total`
static void check_regions(const Region* r, int n, size_t total, int N, int L) {
  for (int i = 0; i < n; ++i) {
    CHECK(r[i].begin % (r[i].pair || i + 1 < n ? sizeof(double) : sizeof(int)) == 0, "%s N=%d L=%d", r[i].name, N, L);
    const size_t end = r[i].begin + r[i].bytes;
    CHECK(end <= (i + 1 < n ? r[i + 1].begin : total), "%s overlaps its successor, N=%d L=%d", r[i].name, N, L);
  }
  CHECK(r[n - 1].begin + r[n - 1].bytes == total, "the last region ends at the total, N=%d L=%d", N, L);
}

// ---- FP64: tvl_loglik_kernel<L, ·> ------------------------------------------------------------------------------
static void check_fp64(int N, int L) {
  constexpr int kTvlBlock = 256, kTvlPre = 8;
  const int GPB = kTvlBlock / L;
  const int TC = chunk_columns(kTvlPre * kTvlBlock, N);
  CHECK(TC >= 1 && TC <= 32, "N=%d", N);
  {  // the rule as the launchers spelled it
    int tc = (kTvlPre * kTvlBlock) / N;
    if (tc > 32) tc = 32;
    CHECK(tc == TC, "N=%d", N);
  }
  // the former byte count (launch_tvl_l), verbatim
  const struct { int N; } a = {N};
  const size_t shmem = sizeof(double) * (size_t)(2 * a.N + TC + TC * a.N + GPB * kTvlGaps + (L >= 4 ? GPB * 16 : 0)) +
                       sizeof(int) * a.N;
  // the former pointer chain (tvl_loglik_kernel), verbatim but for double2 = two doubles
  double* smem = lds;
  double* s_mr = smem;                   // (m_i, 1/m_i)
  double* s_nan = smem + 2 * N;          // TC NaN flags of the staged chunk
  double* s_y = s_nan + TC;              // TC columns of N yields (column-major, stride N)
  double* s_w = s_y + TC * N;            // per group: e^{-λ d_k}, k < K (≤ kTvlGaps)
  double* s_xch = s_w + GPB * kTvlGaps;  // per group: 4×4 exchange block (L ≥ 4)
  double* s_gi = s_xch + (L >= 4 ? GPB * 16 : 0);

  // the kernel's walk over the struct's lengths
  const TvlSmem lay{N, TC, GPB, L};
  double* n_mr = smem;
  double* n_nan = n_mr + lay.mr();
  double* n_y = n_nan + lay.nan();
  double* n_w = n_y + lay.y();
  double* n_xch = n_w + lay.w();
  double* n_gi = n_xch + lay.xch();
  CHECK(lay.bytes() == shmem, "N=%d L=%d: %zu vs %zu", N, L, lay.bytes(), shmem);
  CHECK(n_mr == s_mr && n_nan == s_nan && n_y == s_y && n_w == s_w && n_xch == s_xch && n_gi == s_gi, "N=%d L=%d", N, L);
  CHECK(reinterpret_cast<size_t>(n_mr) % 16 == 0, "s_mr is read as double2, N=%d L=%d", N, L);
  const size_t D = sizeof(double);
  const Region r[] = {{"s_mr", (n_mr - smem) * D, 2 * (size_t)N * D, true},
                      {"s_nan", (n_nan - smem) * D, (size_t)TC * D, false},
                      {"s_y", (n_y - smem) * D, (size_t)TC * N * D, false},
                      {"s_w", (n_w - smem) * D, (size_t)GPB * kTvlGaps * D, false},
                      {"s_xch", (n_xch - smem) * D, (size_t)(L >= 4 ? GPB * 16 : 0) * D, false},
                      {"s_gi", (n_gi - smem) * D, (size_t)N * sizeof(int), false}};
  check_regions(r, 6, lay.bytes(), N, L);
}

// ---- dd: tvl_dd_loglik_kernel<L, ·, ·> ----------------------------------------------------------------------------
static size_t dd_former_bytes(int N, int TC, int GPB) {
  // the former byte count (launch_tvl_dd_l), verbatim
  const struct { int N; } a = {N};
  constexpr int kSumDd = 2;
  const size_t shmem = sizeof(double) * (size_t)(3 * a.N + (2 + 2 * kSumDd) * TC + TC * a.N + GPB * kDPar +
                                                 2 * GPB * kDdWStride + 2 * GPB * kXchStride) +
                       sizeof(int) * a.N;
  return shmem;
}

static void check_dd(int N, int L) {
  constexpr int kDdBlock = 256, kDdPre = 8;
  const int GPB = kDdBlock / L;
  const int TC = chunk_columns(kDdPre * kDdBlock, N);
  CHECK(TC >= 1 && TC <= 32, "N=%d", N);
  const size_t shmem = dd_former_bytes(N, TC, GPB);
  // the former pointer chain (tvl_dd_loglik_kernel), verbatim but for dd = two doubles
  double* smem = lds;
  double* s_m = smem;                                // m_i
  double* s_rm = smem + N;                           // 1/m_i (dd)
  double* s_nan = smem + 3 * N;                      // TC NaN flags of the staged chunk
  double* s_sum = s_nan + TC;                        // per staged column: Σy, Σy² (dd)
  double* s_ymax = s_nan + (1 + 2 * kSumDd) * TC;    // per staged column: max_i |y_i|
  double* s_y = s_ymax + TC;                         // TC columns of N yields
  double* s_par = s_y + TC * N;                      // per group: σ², δ, Φ, Q (kDPar doubles)
  double* s_w = s_par + GPB * kDPar;                 // per group: e^{-λ d_k}, k < K (dd)
  double* s_xch = s_w + 2 * (GPB * kDdWStride);      // per group: 4×4 dd exchange block
  double* s_gi = s_xch + 2 * (GPB * kXchStride);

  // the kernel's walk over the struct's lengths (a dd is two doubles); it splits the first two regions at N and at TC
  const TvlDdSmem lay{N, TC, GPB, L};
  double* n_m = smem;
  double* n_rm = smem + N;
  double* n_nan = smem + lay.mats();
  double* n_sum = n_nan + TC;
  double* n_ymax = n_nan + lay.cols();
  double* n_y = n_ymax + lay.ymax();
  double* n_par = n_y + lay.y();
  double* n_w = n_par + lay.par();
  double* n_xch = n_w + 2 * lay.w();
  double* n_gi = n_xch + 2 * lay.xch();
  CHECK(lay.bytes() == shmem, "N=%d L=%d: %zu vs %zu", N, L, lay.bytes(), shmem);
  CHECK((lay.bytes() > 160 * 1024) == (shmem > 160 * 1024), "N=%d L=%d", N, L);
  CHECK(n_m == s_m && n_rm == s_rm && n_nan == s_nan && n_sum == s_sum && n_ymax == s_ymax && n_y == s_y &&
            n_par == s_par && n_w == s_w && n_xch == s_xch && n_gi == s_gi,
        "N=%d L=%d", N, L);
  // 16-byte alignment of the dd regions, wherever the former chain had it (it depends on the parity of N and TC)
  const size_t D = sizeof(double);
  const struct { const char* name; double* now; double* was; } pairs[] = {
      {"s_rm", n_rm, s_rm}, {"s_sum", n_sum, s_sum}, {"s_w", n_w, s_w}, {"s_xch", n_xch, s_xch}};
  for (const auto& p : pairs)
    if (reinterpret_cast<size_t>(p.was) % 16 == 0) CHECK(reinterpret_cast<size_t>(p.now) % 16 == 0, "%s N=%d L=%d", p.name, N, L);
  const Region r[] = {{"s_m", (n_m - smem) * D, (size_t)N * D, false},
                      {"s_rm", (n_rm - smem) * D, 2 * (size_t)N * D, true},
                      {"s_nan", (n_nan - smem) * D, (size_t)TC * D, false},
                      {"s_sum", (n_sum - smem) * D, 2 * (size_t)kSumDd * TC * D, true},
                      {"s_ymax", (n_ymax - smem) * D, (size_t)TC * D, false},
                      {"s_y", (n_y - smem) * D, (size_t)TC * N * D, false},
                      {"s_par", (n_par - smem) * D, (size_t)GPB * kDPar * D, false},
                      {"s_w", (n_w - smem) * D, 2 * (size_t)GPB * kDdWStride * D, true},
                      {"s_xch", (n_xch - smem) * D, 2 * (size_t)GPB * kXchStride * D, true},
                      {"s_gi", (n_gi - smem) * D, (size_t)N * sizeof(int), false}};
  check_regions(r, 10, lay.bytes(), N, L);
}

// The dd launcher refuses a layout beyond gfx950's 160 KiB of LDS per workgroup.  Its widest layout (L = 4: 64
// groups) is 36·N + 64,560 bytes at one column per chunk, so the refusal first triggers at N = 2,758 — past the 2,048
// yields the prefetch registers hold, where chunk_columns is already 0 and the launcher has refused.  Both are held:
// no N the chunk rule admits reaches the refusal, and at the first N that does, struct and former formula agree.
static void check_dd_refusal() {
  const int Ls[] = {4, 8, 16, 32, 64};
  for (int L : Ls) {
    const int GPB = 256 / L;
    int first = 0;
    for (int N = 1; N <= 8192 && !first; ++N) {
      const int tc = chunk_columns(8 * 256, N);
      const int TC = tc >= 1 ? tc : 1;  // past the chunk rule: the smallest layout there could be
      const bool now = TvlDdSmem{N, TC, GPB, L}.bytes() > 160 * 1024, was = dd_former_bytes(N, TC, GPB) > 160 * 1024;
      CHECK(now == was, "N=%d L=%d", N, L);
      if (was) first = N;
    }
    CHECK(first > 2048, "L=%d: first refused N = %d", L, first);
    if (L == 4) CHECK(first == 2758, "first refused N = %d", first);
    CHECK(chunk_columns(8 * 256, first) == 0, "L=%d", L);
    std::printf("dd L=%d: LDS refusal first at N=%d (chunk rule admits N <= 2048)\n", L, first);
  }
}

int main() {
  const int Ns[] = {1, 3, 4, 7, 30, 33, 360, 2047};
  const int L64[] = {1, 2, 4, 8, 16, 32, 64};
  const int Ldd[] = {4, 8, 16, 32, 64};
  int cases = 0;
  for (int N : Ns) {
    for (int L : L64) check_fp64(N, L), ++cases;
    for (int L : Ldd) check_dd(N, L), ++cases;
  }
  CHECK(chunk_columns(8 * 256, 2048) == 1 && chunk_columns(8 * 256, 2049) == 0 && chunk_columns(8 * 256, 0) == 0,
        "the chunk rule's ends");
  check_dd_refusal();
  std::printf("%d layouts checked, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
