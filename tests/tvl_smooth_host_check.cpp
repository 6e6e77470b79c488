// Host driver of the TVλ extended smoother (csrc/yfm_tvl_smooth.hpp): what the gfx950 kernel tvl_smooth_kernel
// (csrc/yfm_tvl_smooth.hip) computes, from the same functions, one candidate at a time.  The device reads the predicted
// moments a_t, P_t from the TVλ forward launch's record; here they come from yfm_smooth.hpp's predict applied to the
// filtered moments of the same update.
// Compile with -ffp-contract=off (tests/test_tvl_smooth_host_cpu.py; also built there with
// -fsanitize=address,undefined).
//
// Input file (grad_host_check.cpp's; whitespace-separated, doubles as C hex floats or "nan"):
//   N T B space, N maturities, the N×T panel column by column, then per candidate T_use and its 31 θ.
// Output, per candidate, T lines: β̂_t (4), V_t (16, column-major), C_t (16, column-major), hex floats; NaN past the
// window, in C of the window's last column, and everywhere for an unavailable candidate (singular initial state, a data
// column whose det(σ²I + P_tG_t) is not usable — tvlsmooth::det_usable —, an output that is not finite).
#include "../yieldfactormodels.jl_amd/csrc/yfm_tvl_smooth.hpp"
#include "smooth_host_io.hpp"

namespace ts = yfm::tvlsmooth;
namespace tg = yfm::tvlgrad;
constexpr int M = 4;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int N = (int)rd(f), T = (int)rd(f), B = (int)rd(f), space = (int)rd(f);
  if (N < 1 || T < 1 || B < 0) return 2;
  std::vector<double> mats(N), Y((size_t)N * T);
  for (double& v : mats) v = rd(f);
  for (double& v : Y) v = rd(f);
  double minm = INFINITY;
  for (double v : mats) minm = std::fmin(minm, v);
  for (int b = 0; b < B; ++b) {
    int n = (int)rd(f);
    n = n < 1 ? 1 : (n > T ? T : n);
    double th[tg::kNP];
    for (double& v : th) v = rd(f);
    tg::Model gm;
    sm::Model<M> m;
    ts::decode(th, space, gm, m);
    std::vector<Col<M>> col(n);
    double lds[sm::InitCov<M>::kDoubles];
    bool ok = sm::init_mean<M>(m, col[0].a);
    ok = sm::InitCov<M>::solve(m, lds, 0, 1, [] {}, col[0].P) && ok;
    // forward: the operands of every column, linearised at its predicted state
    for (int t = 0; t < n; ++t) {
      tg::StepConst kc;
      tg::step_consts(col[t].a, minm, kc);
      tg::Moments mo;
      ts::stats_zero(mo);
      bool missing = false;
      for (int i = 0; i < N; ++i) {
        const double y = Y[(size_t)t * N + i];
        missing = missing || (y != y);
        ts::accum(kc, col[t].a, mats[i], 1.0 / mats[i], exp(-(kc.lam * mats[i])), y, mo);
      }
      const double det = ts::column_operands(gm, m, col[t].a, col[t].P, mo, N, missing, col[t].o);
      ok = ts::det_usable(det, missing, t + 1) && ok;
      if (t + 1 < n) sm::predict<M>(m, col[t].o.af, col[t].o.Pf, col[t + 1].a, col[t + 1].P);
    }
    print_rows(smooth_backward<M>(m, col, T, ok), M + 2 * M * M);
  }
  std::fclose(f);
  return 0;
}
