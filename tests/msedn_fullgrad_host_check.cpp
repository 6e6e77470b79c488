// Host build of the neural models' full loss gradient (csrc/yfm_msedn_adj.hpp loss_and_fullgrad: the forward sweep with
// its trajectory, then adjoint_step backwards — the routines the gfx950 kernels of csrc/yfm_msedn_adj.hip run): per
// candidate the loss of src/models/filter.jl:209-243 and its P derivatives, every maturity visited in order.
// Stand-alone (its own main), so it runs under -fsanitize=address,undefined as it is.
//
//   msedn_fullgrad_host_check case.txt
// case.txt: as tests/msedn_grad_host_check.cpp reads it — kind N T B space, N maturities, N·T yields (column-major),
// then per candidate T_use and P parameters; numbers as C hex floats or "nan".  Prints per candidate one line of
// 3 + P + 12 numbers: the loss, loss_and_grad's loss for the same candidate, 1 where the gradient of a finite loss is
// unavailable (else 0), the P gradient entries, and loss_and_grad's 12 (the last 12 of the P must be the same bits).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yieldfactormodels.jl_amd/csrc/yfm_msedn_adj.hpp"

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
  } else if (v == HUGE_VAL) {
    std::printf("inf");
  } else {
    std::printf("%a", v);
  }
}

template <bool STATIC, bool HASB, bool SCALED>
void run(int kind, const double* th, int space, const double* mats, const double* Y, int N, int nobs) {
  using namespace yfm::msedn;
  const int P = kind_params(kind);
  // exactly the work the header asks for: a sanitizer sees any record outside it
  std::vector<double> traj((size_t)(nobs - 1) * traj_stride(kind)), g(P);
  double g12[yfm::msed::kGrad];
  bool un = false;
  print_double(loss_and_fullgrad<STATIC, HASB, SCALED>(th, space, kind, mats, Y, N, nobs, traj.data(), g.data(), &un));
  std::printf(" ");
  print_double(loss_and_grad<STATIC, HASB, SCALED>(th, space, kind, mats, Y, N, nobs, g12));
  std::printf(" %d", un ? 1 : 0);
  for (int k = 0; k < P; ++k) {
    std::printf(" ");
    print_double(g[k]);
  }
  for (int k = 0; k < yfm::msed::kGrad; ++k) {
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
  if (!yfm::msedn::kind_known(kind) || N < yfm::msedn::kMinN || T < 1 || B < 0) return 2;
  const int P = yfm::msedn::kind_params(kind);
  std::vector<double> mats(N), Y((size_t)N * T), th(P);
  for (double& v : mats) v = read_double(f);
  for (double& v : Y) v = read_double(f);
  const bool st = yfm::msedn::kind_static(kind), hb = yfm::msedn::kind_has_b(kind), sc = yfm::msedn::kind_scaled(kind);
  for (int b = 0; b < B; ++b) {
    const int tu = read_int(f);
    if (tu < 1 || tu > T) return 2;
    for (double& v : th) v = read_double(f);
    if (st) run<true, false, false>(kind, th.data(), space, mats.data(), Y.data(), N, tu);
    else if (hb && sc) run<false, true, true>(kind, th.data(), space, mats.data(), Y.data(), N, tu);
    else if (hb) run<false, true, false>(kind, th.data(), space, mats.data(), Y.data(), N, tu);
    else if (sc) run<false, false, true>(kind, th.data(), space, mats.data(), Y.data(), N, tu);
    else run<false, false, false>(kind, th.data(), space, mats.data(), Y.data(), N, tu);
  }
  std::fclose(f);
  return 0;
}
