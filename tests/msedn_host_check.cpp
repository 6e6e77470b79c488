// Host build of the neural-model algebra the gfx950 kernel runs (csrc/yfm_msedn.hpp): get_loss of
// src/models/filter.jl:209-243 per candidate, one full filter each, with every maturity visited in order.
// Stand-alone (its own main), so it runs under -fsanitize=address,undefined as it is.
//
//   msedn_host_check case.txt
// case.txt: kind N T B space, N maturities, N·T yields (column-major), then per candidate T_use and P parameters —
// numbers as C hex floats or "nan".  Prints one loss per line (hex float, "-inf" or "nan").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../yieldfactormodels.jl_amd/csrc/yfm_msedn.hpp"

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

double loss(int kind, const double* th, int space, const double* mats, const double* Y, int N, int nobs) {
  using namespace yfm::msedn;
  if (kind_static(kind)) return get_loss<true, false, false>(th, space, kind, mats, Y, N, nobs);
  const bool hb = kind_has_b(kind), sc = kind_scaled(kind);
  if (hb && sc) return get_loss<false, true, true>(th, space, kind, mats, Y, N, nobs);
  if (hb) return get_loss<false, true, false>(th, space, kind, mats, Y, N, nobs);
  if (sc) return get_loss<false, false, true>(th, space, kind, mats, Y, N, nobs);
  return get_loss<false, false, false>(th, space, kind, mats, Y, N, nobs);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int kind = read_int(f), N = read_int(f), T = read_int(f), B = read_int(f), space = read_int(f);
  if (!yfm::msedn::kind_known(kind) || N < yfm::msedn::kMinN || T < 1 || B < 0) return 2;
  const int P = yfm::msedn::kind_params(kind);
  std::vector<double> mats(N), Y((size_t)N * T), th(P);
  for (double& v : mats) v = read_double(f);
  for (double& v : Y) v = read_double(f);
  for (int b = 0; b < B; ++b) {
    const int tu = read_int(f);
    if (tu < 1 || tu > T) return 2;
    for (double& v : th) v = read_double(f);
    const double l = loss(kind, th.data(), space, mats.data(), Y.data(), N, tu);
    if (l != l) {
      std::printf("nan\n");
    } else if (l == -HUGE_VAL) {
      std::printf("-inf\n");
    } else {
      std::printf("%a\n", l);
    }
  }
  std::fclose(f);
  return 0;
}
