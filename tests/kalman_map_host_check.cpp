// Host driver of the Kalman parameter map (csrc/yfm_kalman_map.hpp) for every (M, LEAD) the project has: DNS (3, 1),
// TVλ (4, 0), GNS5 (5, 2) — the text the tangent and smoother kernels call.  Compile with -ffp-contract=off
// (tests/test_kalman_map_host_cpu.py).
//
// Input file (whitespace-separated; doubles as C hex floats): any number of cases, each M LEAD space and P θ.
// Output per case, one labelled line each (hex floats):
//   theta_c  γ, σ², U by column (i ≤ j), δ, Φ row-major: the decoded parameters in θ's own layout
//   Q        M × M row-major
//   chain    chain_factor for d = 0 … P (the last is the padding row)
//   mean     the verdict (1/0) and a₁ from mean_solve<M, 1>
//   mean_inv the verdict, a₁ and (I − Φ)⁻¹ row-major from mean_solve<M, 1 + M>
//   P1       the verdict and P₁ row-major: lyapunov_matrix<M>, then gauss_solve
#include <cstdio>
#include <cstdlib>

#include "../yieldfactormodels.jl_amd/csrc/yfm_kalman_map.hpp"

namespace k = yfm::kalman;

static bool rd(FILE* f, double& v) {
  char buf[128];
  if (std::fscanf(f, "%127s", buf) != 1) return false;
  v = std::strtod(buf, nullptr);
  return true;
}

static void line(const char* label, const double* v, int n) {
  std::printf("%s", label);
  for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
  std::printf("\n");
}

template <int M, int LEAD>
static void run_case(FILE* f, int space) {
  constexpr int P = k::param_count(M, LEAD), S = M * (M + 1) / 2;
  double th[P];
  for (double& v : th)
    if (!rd(f, v)) std::exit(2);
  double gam[LEAD > 0 ? LEAD : 1], sigma2, U[M][M], Q[M][M], delta[M], Phi[M][M];
  k::decode<M, LEAD>(th, space, gam, sigma2, U, Q, delta, Phi);
  double out[P + 1 + M * M];
  int n = 0;
  for (int l = 0; l < LEAD; ++l) out[n++] = gam[l];
  out[n++] = sigma2;
  for (int j = 0; j < M; ++j)
    for (int i = 0; i <= j; ++i) out[n++] = U[i][j];
  for (int i = 0; i < M; ++i) out[n++] = delta[i];
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) out[n++] = Phi[i][j];
  line("theta_c", out, n);
  line("Q", &Q[0][0], M * M);
  for (int d = 0; d <= P; ++d) out[d] = k::chain_factor<M, LEAD>(th, space, d);
  line("chain", out, P + 1);

  double x1[M][1], xi[M][1 + M];
  out[0] = k::mean_solve<M, 1>(Phi, delta, x1) ? 1.0 : 0.0;
  for (int i = 0; i < M; ++i) out[1 + i] = x1[i][0];
  line("mean", out, 1 + M);
  out[0] = k::mean_solve<M, 1 + M>(Phi, delta, xi) ? 1.0 : 0.0;
  for (int i = 0; i < M; ++i) out[1 + i] = xi[i][0];
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) out[1 + M + i * M + j] = xi[i][1 + j];
  line("mean_inv", out, 1 + M + M * M);

  double L[S][S], q[S][1];
  k::lyapunov_matrix<M>(Phi, L);
  int r = 0;
  for (int i = 0; i < M; ++i)
    for (int j = i; j < M; ++j) q[r++][0] = Q[i][j];
  out[0] = k::gauss_solve<S, 1>(L, q) ? 1.0 : 0.0;
  r = 0;
  for (int i = 0; i < M; ++i)
    for (int j = i; j < M; ++j) {
      out[1 + i * M + j] = q[r][0];
      out[1 + j * M + i] = q[r][0];
      ++r;
    }
  line("P1", out, 1 + M * M);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  double m, lead, space;
  while (rd(f, m)) {
    if (!rd(f, lead) || !rd(f, space)) return 2;
    if (m == 3 && lead == 1)
      run_case<3, 1>(f, (int)space);
    else if (m == 4 && lead == 0)
      run_case<4, 0>(f, (int)space);
    else if (m == 5 && lead == 2)
      run_case<5, 2>(f, (int)space);
    else
      return 2;
  }
  std::fclose(f);
  return 0;
}
