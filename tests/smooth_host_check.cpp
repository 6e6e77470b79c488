// Host driver of the fixed-interval smoother (csrc/yfm_smooth.hpp): what the gfx950 kernel smooth_kernel
// (csrc/yfm_smooth.hip) computes, from the same functions, one candidate at a time.  The device reads the predicted
// moments a_t, P_t from the forward launch's record; here they come from yfm_smooth.hpp's own predict.
// Compile with -ffp-contract=off and -DYFM_SMOOTH_M=3 (DNS, 20 θ) or 5 (GNS5, 48 θ) (tests/test_smooth_host_cpu.py;
// also built there with -fsanitize=address,undefined).
//
// Input file (grad_host_check.cpp's; whitespace-separated, doubles as C hex floats or "nan"):
//   N T B space, N maturities, the N×T panel column by column, then per candidate T_use and its θ.
// Output, per candidate, T lines: β̂_t (M), V_t (M², column-major), C_t (M², column-major), hex floats; NaN past the
// window, in C of the window's last column, and everywhere for a candidate whose initial state is singular or that
// has an output that is not finite.
#include "../yieldfactormodels.jl_amd/csrc/yfm_smooth.hpp"
#include "smooth_host_io.hpp"

#ifndef YFM_SMOOTH_M
#define YFM_SMOOTH_M 3
#endif

constexpr int M = YFM_SMOOTH_M;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int N = (int)rd(f), T = (int)rd(f), B = (int)rd(f), space = (int)rd(f);
  if (N < 1 || T < 1 || B < 0) return 2;
  std::vector<double> mats(N), Y((size_t)N * T);
  for (double& v : mats) v = rd(f);
  for (double& v : Y) v = rd(f);
  for (int b = 0; b < B; ++b) {
    int n = (int)rd(f);
    n = n < 1 ? 1 : (n > T ? T : n);
    double th[sm::Model<M>::kNP];
    for (double& v : th) v = rd(f);
    sm::Model<M> m;
    sm::decode<M>(th, space, m);
    std::vector<double> Z((size_t)N * M);
    double G[M][M] = {};
    for (int i = 0; i < N; ++i) {
      double z[M];
      sm::loading_row<M>(m, mats[i], z);
      for (int k = 0; k < M; ++k) Z[(size_t)i * M + k] = z[k];
      for (int j = 0; j < M; ++j)
        for (int k = j; k < M; ++k) G[j][k] = sm::sfma(z[j], z[k], G[j][k]);
    }
    for (int j = 0; j < M; ++j)
      for (int k = j + 1; k < M; ++k) G[k][j] = G[j][k];
    std::vector<Col<M>> col(n);
    double lds[sm::InitCov<M>::kDoubles];
    bool ok = sm::init_mean<M>(m, col[0].a);
    ok = sm::InitCov<M>::solve(m, lds, 0, 1, [] {}, col[0].P) && ok;
    // forward: the operands of every column
    for (int t = 0; t < n; ++t) {
      double zy[M] = {};
      bool missing = false;
      for (int i = 0; i < N; ++i) {
        const double y = Y[(size_t)t * N + i];
        missing = missing || (y != y);
        for (int k = 0; k < M; ++k) zy[k] = sm::sfma(Z[(size_t)i * M + k], y, zy[k]);
      }
      sm::step_operands<M>(m, G, col[t].a, col[t].P, zy, missing, col[t].o);
      if (t + 1 < n) sm::predict<M>(m, col[t].o.af, col[t].o.Pf, col[t + 1].a, col[t + 1].P);
    }
    print_rows(smooth_backward<M>(m, col, T, ok), M + 2 * M * M);
  }
  std::fclose(f);
  return 0;
}
