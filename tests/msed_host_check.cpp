// Host build of the λ-model algebra the gfx950 kernel runs (csrc/yfm_msed.hpp): get_loss of
// src/models/filter.jl:209-243 per candidate, one full filter each, with every maturity visited in order.
// Stand-alone (its own main), so it runs under -fsanitize=address,undefined as it is.
//
//   msed_host_check case.txt
// case.txt: kind N T B space, N maturities, N·T yields (column-major), then per candidate T_use and P parameters —
// numbers as C hex floats or "nan".  Prints one loss per line (hex float, "-inf" or "nan").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

double loss(int kind, const double* th, int space, const double* mats, const double* Y, int N, int nobs, double* pred) {
  using namespace yfm::msed;
  switch (kind) {
    case 3: return get_loss<true, false, false>(th, space, mats, Y, N, nobs, pred);
    case 4: return get_loss<false, true, false>(th, space, mats, Y, N, nobs, pred);
    case 5: return get_loss<false, false, false>(th, space, mats, Y, N, nobs, pred);
    case 6: return get_loss<false, true, true>(th, space, mats, Y, N, nobs, pred);
    case 8: return get_loss<false, false, true>(th, space, mats, Y, N, nobs, pred);
  }
  std::fprintf(stderr, "unknown kind %d\n", kind);
  std::exit(2);
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
    const double l = loss(kind, th.data(), space, mats.data(), Y.data(), N, tu, pred.data());
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
