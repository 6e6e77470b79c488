// Host driver of the DNS score series (csrc/yfm_grad.hpp, score_value): the per-step terms the gfx950 kernel
// dns_score_kernel (csrc/yfm_score.hip) stores, from the same functions, with all 20 directions in one thread.
// Compile with -ffp-contract=off (tests/test_score_host_cpu.py; also built there with -fsanitize=address,undefined).
//
// Input file (grad_host_check.cpp's; whitespace-separated, doubles as C hex floats or "nan"):
//   N T B space, N maturities, the N×T panel column by column, then per candidate T_use and 20 θ.
// Output, per candidate: one line ll g_0 … g_19, then T − 1 lines S[0, k] … S[19, k] (hex floats): exact zeros in the
// columns outside the accumulated range 1 … T_use − 2.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../yieldfactormodels.jl_amd/csrc/yfm_grad.hpp"

namespace g = yfm::grad;

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
  // the prepared panel of prep_panel_kernel: centered columns, ȳ, ỹ'ỹ, NaN flag
  std::vector<double> yc((size_t)N * T), ybar(T), ytt(T);
  std::vector<char> isnan_col(T);
  for (int t = 0; t < T; ++t) {
    double s1 = 0.0;
    bool nan = false;
    for (int i = 0; i < N; ++i) {
      const double v = Y[(size_t)t * N + i];
      nan = nan || (v != v);
      s1 += v;
    }
    ybar[t] = s1 / (double)N;
    double tt = 0.0;
    for (int i = 0; i < N; ++i) {
      const double d = Y[(size_t)t * N + i] - ybar[t];
      yc[(size_t)t * N + i] = d;
      tt = g::gfma(d, d, tt);
    }
    ytt[t] = tt;
    isnan_col[t] = nan;
  }
  const int ncol = T - 1;
  std::vector<double> S((size_t)g::kNP * (ncol > 0 ? ncol : 1));
  for (int b = 0; b < B; ++b) {
    int nobs = (int)rd(f);
    nobs = nobs < 1 ? 1 : (nobs > T ? T : nobs);
    double th[g::kNP];
    for (double& v : th) v = rd(f);
    g::Common c;
    g::decode(th, space, c.m);
    std::vector<double> z1(N), z2(N), d1(N), d2(N);
    double gs[5] = {0, 0, 0, 0, 0}, dgs[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < N; ++i) {
      g::loadings(c.m.gam, mats[i], z1[i], z2[i], d1[i], d2[i]);
      g::gram_add(z1[i], z2[i], d1[i], d2[i], gs, dgs);
    }
    g::setup_common(c, gs, dgs, N);
    g::State s;
    g::Tangent t[g::kNP];
    for (int d = 0; d < g::kNP; ++d) g::seed<g::kSeedAll>(c.m, d, t[d]);
    g::init_state<g::kNP>(c, s, t);
    for (double& v : S) v = 0.0;
    for (int k = 0; k + 1 < nobs; ++k) {
      const bool acc = k >= 1;
      if (isnan_col[k]) {
        for (int d = 0; d < g::kNP; ++d) g::tangent_nan_step<g::kSeedAll>(c, s, t[d], acc);
        g::primal_nan_step(c.m, s, acc);
      } else {
        double z[2] = {0, 0}, dz[2] = {0, 0};
        for (int i = 0; i < N; ++i) {
          const double y = yc[(size_t)k * N + i];
          z[0] = g::gfma(z1[i], y, z[0]);
          z[1] = g::gfma(z2[i], y, z[1]);
          dz[0] = g::gfma(d1[i], y, dz[0]);
          dz[1] = g::gfma(d2[i], y, dz[1]);
        }
        g::Step u;
        double det, q;
        g::primal_update(c, s, z, dz, ybar[k], ytt[k], u, det, q);
        for (int d = 0; d < g::kNP; ++d) g::tangent_data_step<g::kSeedAll>(c, s, u, t[d], acc);
        g::primal_account(s, det, q, acc);
        g::primal_predict(c.m, u.bf, u.Pf, s);
      }
      for (int d = 0; d < g::kNP; ++d)
        S[(size_t)k * g::kNP + d] = g::score_value(c, t[d], acc) * g::chain_factor(th, space, d) + 0.0;
    }
    std::printf("%a", g::loglik_value(c, s, nobs));
    for (int d = 0; d < g::kNP; ++d) std::printf(" %a", g::grad_value(c, t[d], nobs) * g::chain_factor(th, space, d) + 0.0);
    std::printf("\n");
    for (int k = 0; k < ncol; ++k) {
      for (int d = 0; d < g::kNP; ++d) std::printf("%s%a", d ? " " : "", S[(size_t)k * g::kNP + d]);
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
