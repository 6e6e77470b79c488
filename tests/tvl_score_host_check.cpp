// Host driver of the TVλ score series (csrc/yfm_tvl_grad.hpp, score_value): the per-step terms the gfx950 kernel
// tvl_score_kernel (csrc/yfm_tvl_score.hip) stores, from the same functions, with all 31 directions in one thread and
// every maturity in one "lane".  Compile with -ffp-contract=off (tests/test_tvl_info_fixture_cpu.py; also built there
// with -fsanitize=address,undefined).
//
// Input file (tvl_grad_host_check.cpp's; whitespace-separated, doubles as C hex floats or "nan"):
//   N T B space, N maturities, the N×T panel column by column, then per candidate T_use and 31 θ.
// Output, per candidate: one line ll g_0 … g_30, then T − 1 lines S[0, k] … S[30, k] (hex floats): exact zeros in the
// columns outside the accumulated range 1 … T_use − 2.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../yieldfactormodels.jl_amd/csrc/yfm_tvl_grad.hpp"

namespace g = yfm::tvlgrad;

static double rd(FILE* f) {
  char buf[128];
  if (std::fscanf(f, "%127s", buf) != 1) {
    std::fprintf(stderr, "short input\n");
    std::exit(2);
  }
  return std::strtod(buf, nullptr);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int N = (int)rd(f), T = (int)rd(f), B = (int)rd(f), space = (int)rd(f);
  if (N < 1 || T < 1 || B < 0) return 2;
  std::vector<double> mats(N), Y((size_t)N * T);
  for (double& v : mats) v = rd(f);
  for (double& v : Y) v = rd(f);
  std::vector<char> isnan_col(T);
  double minm = INFINITY;
  for (int i = 0; i < N; ++i) minm = std::fmin(minm, mats[i]);
  for (int t = 0; t < T; ++t) {
    bool nan = false;
    for (int i = 0; i < N; ++i) nan = nan || (Y[(size_t)t * N + i] != Y[(size_t)t * N + i]);
    isnan_col[t] = nan;
  }
  const int ncol = T - 1;
  std::vector<double> Sc((size_t)g::kNP * (ncol > 0 ? ncol : 1));
  for (int b = 0; b < B; ++b) {
    g::Tangent t[g::kNP];
    const int nobs = std::min(std::max((int)rd(f), 1), T);
    double th[g::kNP];
    for (double& v : th) v = rd(f);
    g::Model m;
    g::decode(th, space, m);
    g::State s;
    for (int d = 0; d < g::kNP; ++d) g::seed(d, t[d]);
    double Linv[100];
    for (int c = 0; c < 10; ++c) {
      double col[10];
      g::lyapunov_inverse_column(m.Phi, c, col);
      for (int r = 0; r < 10; ++r) Linv[r * 10 + c] = col[r];
    }
    g::init_state<g::kNP>(m, Linv, s, t);
    std::fill(Sc.begin(), Sc.end(), 0.0);
    for (int k = 0; k + 1 < nobs; ++k) {
      const bool acc = k >= 1;
      const bool nan = isnan_col[k];
      g::StepConst kc;
      g::step_consts(s.beta, minm, kc);
      g::Moments mo;
      g::moments_zero(mo);
      for (int i = 0; i < N; ++i)
        g::accum(kc, s.beta, mats[i], 1.0 / mats[i], std::exp(-(kc.lam * mats[i])), Y[(size_t)k * N + i], mo);
      g::Step u;
      g::primal_update(m, s, mo, N, u);
      g::Filtered fl;
      g::filtered_state(m, s, u, nan, fl);
      for (int d = 0; d < g::kNP; ++d) g::tangent_step<g::kSeedAll>(m, s, u, mo, N, fl, nan, t[d], acc);
      g::primal_step(m, u, fl, nan, s, acc);
      for (int d = 0; d < g::kNP; ++d)
        Sc[(size_t)k * g::kNP + d] = g::score_value(m, t[d], N, acc) * g::chain_factor(th, space, d) + 0.0;
    }
    std::printf("%a", g::loglik_value(m, s, N, nobs));
    for (int d = 0; d < g::kNP; ++d)
      std::printf(" %a", g::grad_value(m, t[d], N, nobs) * g::chain_factor(th, space, d) + 0.0);
    std::printf("\n");
    for (int k = 0; k < ncol; ++k) {
      for (int d = 0; d < g::kNP; ++d) std::printf("%s%a", d ? " " : "", Sc[(size_t)k * g::kNP + d]);
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
