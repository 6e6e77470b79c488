// yfm_kalman_map.hpp — the Kalman family's parameter map and its small dense solves, stated once for the tangent and
// smoother kernels, as plain functions that compile for the device and for the host (tests/kalman_map_host_check.cpp).
//
// Reference semantics (paths relative to the reference root):
//   decode        src/models/parameteroperations.jl:22-32 (transform_params), src/models/kalman/paramoperations.jl:6-59
//                 (set_params!), src/utils/transformations.jl:2-26
//   chain_factor  the derivative of those transformations, row by row
//   mean_solve, lyapunov_matrix   src/models/kalman/filter.jl:1-10 (initialize_filter)
// θ layout: [γ (LEAD), σ², U by column (i ≤ j), δ (M), Φ row-major (M × M)]; DNS (M, LEAD) = (3, 1), TVλ (4, 0),
// GNS5 (5, 2).
//
// Who includes this: yfm_grad.hpp, yfm_tvl_grad.hpp (through yfm_grad.hpp) and yfm_smooth.hpp, and nothing else.  Each
// of them switches contraction off at file scope before anything of its own; the pragma below does the same and, being
// at file scope, stays in force for the rest of whatever includes this file.  So it is never included from
// yfm_device.hpp, nor before it: the loglik kernels are compiled with the default contraction and keep their own text
// of the same mathematics (DESIGN.md §3.14b says what differs and by how much).
// Every fused multiply-add is an explicit fma; contraction is off.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YFM_KHD __host__ __device__ __forceinline__
#else
#include <math.h>
#define YFM_KHD inline
#endif
#include <utility>

namespace yfm {
namespace kalman {

YFM_KHD double kfma(double a, double b, double c) { return __builtin_fma(a, b, c); }

constexpr int param_count(int M, int lead) { return lead + 1 + M * (M + 1) / 2 + M + M * M; }

// Gaussian elimination with partial pivoting (getf2's pivot rule, selects instead of row indexing), n×n with R
// right-hand sides; A is left holding U (its diagonal gives |det|).  False on an exact zero pivot, where the
// reference's solve throws; a caller may ignore the verdict.
template <int n, int R>
YFM_KHD bool gauss_solve(double (&A)[n][n], double (&X)[n][R]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    int p = k;
    double amax = fabs(A[k][k]);
#pragma unroll
    for (int i = k + 1; i < n; ++i) {
      const double a = fabs(A[i][k]);
      const bool gt = a > amax;
      amax = gt ? a : amax;
      p = gt ? i : p;
    }
#pragma unroll
    for (int i = k + 1; i < n; ++i) {
      const bool s = (p == i);
#pragma unroll
      for (int c = k; c < n; ++c) {
        const double a = A[k][c], b = A[i][c];
        A[k][c] = s ? b : a;
        A[i][c] = s ? a : b;
      }
#pragma unroll
      for (int c = 0; c < R; ++c) {
        const double a = X[k][c], b = X[i][c];
        X[k][c] = s ? b : a;
        X[i][c] = s ? a : b;
      }
    }
    ok = ok && (A[k][k] != 0.0);
    const double r = 1.0 / A[k][k];
#pragma unroll
    for (int i = k + 1; i < n; ++i) {
      const double l = A[i][k] * r;
#pragma unroll
      for (int c = k + 1; c < n; ++c) A[i][c] = kfma(-l, A[k][c], A[i][c]);
#pragma unroll
      for (int c = 0; c < R; ++c) X[i][c] = kfma(-l, X[k][c], X[i][c]);
    }
  }
#pragma unroll
  for (int k = n - 1; k >= 0; --k) {
    const double r = 1.0 / A[k][k];
#pragma unroll
    for (int c = 0; c < R; ++c) {
      double s = X[k][c];
#pragma unroll
      for (int j = k + 1; j < n; ++j) s = kfma(-A[k][j], X[j][c], s);
      X[k][c] = s * r;
    }
  }
  return ok;
}

// transform_params (space == 0) + set_params!: θ → γ, σ², U, Q = U'U, δ, Φ, each into the caller's own storage
// (gam is not written at LEAD = 0).  The exps are computed unconditionally and selected.
template <int M, int LEAD>
YFM_KHD void decode(const double* th, int space, double* gam, double& sigma2, double (&U)[M][M], double (&Q)[M][M],
                    double (&delta)[M], double (&Phi)[M][M]) {
  int k = 0;
#pragma unroll
  for (int l = 0; l < LEAD; ++l) gam[l] = th[k++];
  const double es = exp(th[k]);
  sigma2 = space == 0 ? es : th[k];
  ++k;
#pragma unroll
  for (int j = 0; j < M; ++j)
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (i <= j) {
        double x = th[k++];
        if (i == j) {
          const double e = exp(x);
          x = space == 0 ? e : x;
        }
        U[i][j] = x;
      } else {
        U[i][j] = 0.0;
      }
    }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < M; ++l) s = kfma(U[l][i], U[l][j], s);
      Q[i][j] = s;
    }
#pragma unroll
  for (int i = 0; i < M; ++i) delta[i] = th[k++];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double x = th[k++];
      if (i == j) {
        const double y = exp(x);
        const double e = 2.0 * y / (1.0 + y) - 1.0;
        x = space == 0 ? e : x;
      }
      Phi[i][j] = x;
    }
}

// dθ_c[d]/dθ[d]: exp for σ² and the diagonal of U, d/dx (2y/(1+y) − 1) = 2y/(1+y)² (y = eˣ) for the Φ diagonal
// (transformations.jl:2-4, :21-26), 1 elsewhere and in the constrained space.  d ≥ P is a padding direction: the
// row read is clamped to the last one and the factor is 1.
// The rows are compile-time constants folded into one || chain each (J = 0 … M − 1): a loop over J, unrolled later, gave
// other code in all four tangent kernels.
template <int M, int LEAD, int... J>
YFM_KHD double chain_factor(const double* th, int space, int d, std::integer_sequence<int, J...>) {
  constexpr int kNP = param_count(M, LEAD);
  constexpr int kOffU = LEAD + 1, kOffF = kOffU + M * (M + 1) / 2 + M;
  const int dc = d < kNP ? d : kNP - 1;
  const double y = exp(th[dc]);
  const bool pos = ((d == LEAD) || ... || (d == kOffU + J * (J + 1) / 2 + J));
  const bool r11 = (... || (d == kOffF + J * (M + 1)));
  const double dr = 2.0 * y / ((1.0 + y) * (1.0 + y));
  const double f = pos ? y : (r11 ? dr : 1.0);
  return space == 0 ? f : 1.0;
}
template <int M, int LEAD>
YFM_KHD double chain_factor(const double* th, int space, int d) {
  return chain_factor<M, LEAD>(th, space, d, std::make_integer_sequence<int, M>{});
}

// a₁ = (I − Φ) \ δ (filter.jl:4) into column 0 of X.  With R = 1 + M the columns 1 … M come back holding (I − Φ)⁻¹,
// which the tangents of a₁ go through; with R = 1 only the mean is solved for.  False on an exact zero pivot.
template <int M, int R>
YFM_KHD bool mean_solve(const double (&Phi)[M][M], const double (&delta)[M], double (&X)[M][R]) {
  static_assert(R == 1 || R == 1 + M, "the mean alone, or the mean and the inverse");
  double A[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      A[i][j] = (i == j ? 1.0 : 0.0) - Phi[i][j];
      if constexpr (R > 1) X[i][1 + j] = (i == j) ? 1.0 : 0.0;
    }
    X[i][0] = delta[i];
  }
  return gauss_solve<M, R>(A, X);
}

// P₁ (filter.jl:7) on the symmetric subspace: the M(M+1)/2 unknowns P_kl (k ≤ l) of P − ΦPΦ' = Q, row (i, j), i ≤ j.
// The coefficient of P_kl in (ΦPΦ')_ij …
template <int M>
YFM_KHD double lyapunov_coefficient(const double (&Phi)[M][M], int i, int j, int k, int l) {
  double s = Phi[i][k] * Phi[j][l];
  if (k != l) s = kfma(Phi[i][l], Phi[j][k], s);
  return s;
}
// … and the operator I − (that), row-major over the pairs
template <int M>
YFM_KHD void lyapunov_matrix(const double (&Phi)[M][M], double (&L)[M * (M + 1) / 2][M * (M + 1) / 2]) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = i; j < M; ++j) {
      int c = 0;
#pragma unroll
      for (int k = 0; k < M; ++k)
#pragma unroll
        for (int l = k; l < M; ++l) {
          L[r][c] = (r == c ? 1.0 : 0.0) - lyapunov_coefficient<M>(Phi, i, j, k, l);
          ++c;
        }
      ++r;
    }
}

}  // namespace kalman
}  // namespace yfm
