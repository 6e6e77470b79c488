// Host build of the λ models' full loss gradient (csrc/yfm_msed.hpp: d2loadings, accum_tan, ols_tangent, score_tangent,
// update_gamma_tangent, advance_tangent, lead_accum, fullgrad_finish, driven by get_loss_fullgrad): per candidate the
// loss of src/models/filter.jl:209-243 and its P derivatives, every maturity visited in order.  Stand-alone (its own
// main), so it runs under -fsanitize=address,undefined as it is.
//
//   msed_fullgrad_host_check case.txt
// case.txt: as tests/msed_host_check.cpp reads it — kind N T B space, N maturities, N·T yields (column-major), then
// per candidate T_use and P parameters; numbers as C hex floats or "nan".  Prints per candidate one line of 3 + P + 12
// numbers: the loss, get_loss of the same header for the same candidate (the two must be the same bits), 1 where the
// gradient of a finite loss is unavailable, the P gradient entries and get_loss_grad's 12 (the same bits as the last
// 12 of the P) — hex float, "-inf" or "nan".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yieldfactormodels.jl_amd/csrc/yfm_msed.hpp"

namespace {

double read_double(FILE* f) {
  char w[64];
  if (std::fscanf(f, "%63s", w) != 1) {
    std::fprintf(stderr, "short case file\n");
    std::exit(2);
  }
  if (!std::strcmp(w, "nan")) return std::strtod("nan", nullptr);
  return std::strtod(w, nullptr);
}

int read_int(FILE* f) { return (int)read_double(f); }

void print_double(double v) {
  if (v != v) {
    std::printf("nan");
  } else if (v == -HUGE_VAL) {
    std::printf("-inf");
  } else {
    std::printf("%a", v);
  }
}

template <bool STATIC, bool HASB, bool SCALED>
void run(const double* th, int space, const double* mats, const double* Y, int N, int nobs, double* pred) {
  using namespace yfm::msed;
  constexpr int P = lead_count<STATIC, HASB>() + kGrad;
  double g[P], g12[kGrad];
  bool un = false;
  print_double(get_loss_fullgrad<STATIC, HASB, SCALED>(th, space, mats, Y, N, nobs, g, &un));
  std::printf(" ");
  print_double(get_loss<STATIC, HASB, SCALED>(th, space, mats, Y, N, nobs, pred));
  std::printf(" %d", un ? 1 : 0);
  (void)get_loss_grad<STATIC, HASB, SCALED>(th, space, mats, Y, N, nobs, g12);
  for (int k = 0; k < P; ++k) {
    std::printf(" ");
    print_double(g[k]);
  }
  for (int k = 0; k < kGrad; ++k) {
    std::printf(" ");
    print_double(g12[k]);
  }
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int kind = read_int(f), N = read_int(f), T = read_int(f), B = read_int(f), space = read_int(f);
  if (!yfm::msed::kind_known(kind) || N < 1 || T < 1 || B < 0) return 2;
  const int P = yfm::msed::kind_params(kind);
  std::vector<double> mats(N), Y((size_t)N * T), th(P), pred(N);
  for (double& v : mats) v = read_double(f);
  for (double& v : Y) v = read_double(f);
  for (int b = 0; b < B; ++b) {
    const int tu = read_int(f);
    if (tu < 1 || tu > T) return 2;
    for (double& v : th) v = read_double(f);
    switch (kind) {
      case 3: run<true, false, false>(th.data(), space, mats.data(), Y.data(), N, tu, pred.data()); break;
      case 4: run<false, true, false>(th.data(), space, mats.data(), Y.data(), N, tu, pred.data()); break;
      case 5: run<false, false, false>(th.data(), space, mats.data(), Y.data(), N, tu, pred.data()); break;
      case 6: run<false, true, true>(th.data(), space, mats.data(), Y.data(), N, tu, pred.data()); break;
      case 8: run<false, false, true>(th.data(), space, mats.data(), Y.data(), N, tu, pred.data()); break;
    }
  }
  std::fclose(f);
  return 0;
}
