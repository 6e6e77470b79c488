// yfm_smooth.hpp — the fixed-interval Kalman smoother of the fixed-loading models (DNS M = 3, GNS5 M = 5), as plain
// functions that compile for the device (yfm_smooth.hip) and for the host (tests/smooth_host_check.cpp).
//
// An extension: the reference's predict (src/models/kalman/filter.jl:250-282) returns the forecasts a_{t+1|t} only.
// The model is the one its fixed-loading filter! runs (filter.jl:125-179 from initialize_filter, filter.jl:1-10):
//     y_t = Zβ_t + ε_t, Var ε = σ²I;   β_{t+1} = δ + Φβ_t + η_t, Var η = Q;   a_1 = (I − Φ)⁻¹δ, P_1 = ΦP_1Φ' + Q.
// With G = Z'Z and a_t, P_t the predicted moments (include/yfm.h yfm_smooth_batch), a data column gives
//     B_t = σ²I + G P_t,   s_t = B_t⁻¹(Z'y_t − G a_t),   W_t = B_t⁻¹G,   E_t = σ²B_t⁻¹,   L_t = Φ(I − P_tW_t) = ΦE_t',
// a missing column s_t = 0, W_t = 0, L_t = Φ, and backwards from r_n = 0, N_n = 0
//     r_{t−1} = s_t + L_t'r_t,   N_{t−1} = W_t + L_t'N_tL_t.
// The outputs are taken from the filtered moments a_{t|t} = a_t + P_ts_t = G⁻¹(Z'y_t − σ²s_t) and
// P_{t|t} = P_t − P_tW_tP_t = P_tE_t, which never form I − P_tW_t by subtraction nor add P_ts_t to a large a_t: with
// X_t = L_tP_t = ΦP_{t|t},
//     β̂_t = a_t + P_tr_{t−1} = a_{t|t} + X_t'r_t,
//     V_t = P_t − P_tN_{t−1}P_t = P_{t|t} − X_t'N_tX_t,
//     C_t = Cov(β_{t+1}, β_t | y_1..n) = (I − P_{t+1}N_t)X_t.
// s_t, W_t, L_t, a_{t|t} and P_{t|t} depend on the recorded moments and the data only (step_operands: parallel over t);
// r and N are the only serial part (chain_step); the outputs are parallel over t again (step_outputs).
// Every fused multiply-add is an explicit fma; contraction is off.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YFM_SHD __host__ __device__ __forceinline__
#else
#include <math.h>
#define YFM_SHD inline
#endif

#include "yfm_kalman_map.hpp"  // the parameter map and the small solves, shared with the tangent kernels

namespace yfm {
namespace smooth {

YFM_SHD double sfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
YFM_SHD bool finite(double x) { return x - x == 0.0; }

// θ_c of a fixed-loading model: [γ (LEAD), σ², U by column (i ≤ j), δ, Φ row-major]; DNS LEAD = 1, GNS5 LEAD = 2
template <int M>
struct Model {
  static constexpr int kLead = (M - 1) / 2;
  static constexpr int kNP = kLead + 1 + M * (M + 1) / 2 + M + M * M;
  double gam[kLead];
  double sigma2;
  double Q[M][M], delta[M], Phi[M][M];
};

// transform_params (space == 0) + set_params!; the smoother has no use for U beyond Q = U'U
template <int M>
YFM_SHD void decode(const double* th, int space, Model<M>& m) {
  double U[M][M];
  kalman::decode<M, Model<M>::kLead>(th, space, m.gam, m.sigma2, U, m.Q, m.delta, m.Phi);
}

// row i of Z: [1, S(λ₁), C(λ₁) (, S(λ₂), C(λ₂))], λ = 0.01 + e^γ (dns.jl:51-65; the GNS5 extension takes two γ)
template <int M>
YFM_SHD void loading_row(const Model<M>& m, double mat, double (&z)[M]) {
  z[0] = 1.0;
#pragma unroll
  for (int l = 0; l < Model<M>::kLead; ++l) {
    const double lam = 1e-2 + exp(m.gam[l]);
    const double tau = lam * mat;
    const double e = exp(-tau);
    const double s = (1.0 - e) / tau;
    z[1 + 2 * l] = s;
    z[2 + 2 * l] = s - e;
  }
}

using kalman::gauss_solve;

// a_1 = (I − Φ) \ δ (filter.jl:4)
template <int M>
YFM_SHD bool init_mean(const Model<M>& m, double (&a)[M]) {
  double x[M][1];
  const bool ok = kalman::mean_solve<M, 1>(m.Phi, m.delta, x);
#pragma unroll
  for (int i = 0; i < M; ++i) a[i] = x[i][0];
  return ok;
}

// P_1 (filter.jl:7) on the symmetric subspace (kalman::lyapunov_coefficient): the S = M(M+1)/2 unknowns P_ij
// (i ≤ j) of P − ΦPΦ' = Q.  The S × (S + 1) augmented system lives in memory the caller provides (LDS on the device):
// a wave's lanes share the elimination, element e of a row update going to lane e mod nl, with `sync` between the
// phases; the host runs it with lane = 0, nl = 1.  Every lane returns the same verdict and reads the same P.
template <int M>
struct InitCov {
  static constexpr int S = M * (M + 1) / 2;
  static constexpr int LD = S + 1;
  static constexpr int kDoubles = S * LD;

  template <class Sync>
  YFM_SHD static bool solve(const Model<M>& m, double* A, int lane, int nl, Sync sync, double (&P)[M][M]) {
    // row r ↔ (i, j), column c ↔ (k, l): the coefficient of P_kl in (P − ΦPΦ')_ij
    // (compile-time indices throughout: the model stays in registers; element e is stored by lane e mod nl)
    {
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
              const double s = kalman::lyapunov_coefficient<M>(m.Phi, i, j, k, l);
              if ((r * LD + c) % nl == lane) A[r * LD + c] = (r == c ? 1.0 : 0.0) - s;
              ++c;
            }
          if ((r * LD + S) % nl == lane) A[r * LD + S] = m.Q[i][j];
          ++r;
        }
    }
    sync();
    bool ok = true;
    for (int k = 0; k < S; ++k) {
      // every lane finds the same pivot row (first index of the largest magnitude)
      int p = k;
      double amax = fabs(A[k * LD + k]);
      for (int i = k + 1; i < S; ++i) {
        const double a = fabs(A[i * LD + k]);
        if (a > amax) {
          amax = a;
          p = i;
        }
      }
      sync();
      if (p != k) {
        for (int c = lane; c < LD; c += nl) {
          const double a = A[k * LD + c], b = A[p * LD + c];
          A[k * LD + c] = b;
          A[p * LD + c] = a;
        }
        sync();
      }
      const double piv = A[k * LD + k];
      ok = ok && (piv != 0.0);
      const double rp = 1.0 / piv;
      // rows k + 1 … S − 1, columns k + 1 … S: column k keeps the multiplier's numerator until every lane has read it
      const int nc = LD - (k + 1);
      for (int e = lane; e < (S - k - 1) * nc; e += nl) {
        const int i = k + 1 + e / nc, c = k + 1 + e % nc;
        const double l = A[i * LD + k] * rp;
        A[i * LD + c] = sfma(-l, A[k * LD + c], A[i * LD + c]);
      }
      sync();
    }
    // back substitution, every lane for itself (S values)
    double x[S];
#pragma unroll
    for (int k = S - 1; k >= 0; --k) {
      double s = A[k * LD + S];
#pragma unroll
      for (int j = k + 1; j < S; ++j) s = sfma(-A[k * LD + j], x[j], s);
      x[k] = s * (1.0 / A[k * LD + k]);
    }
    int q = 0;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = i; j < M; ++j) {
        P[i][j] = x[q];
        P[j][i] = x[q];
        ++q;
      }
    sync();
    return ok;
  }
};

// what a column contributes: the backward recursion's operands and the filtered moments
template <int M>
struct StepOps {
  double s[M], W[M][M], L[M][M];  // the chain's operands
  double af[M], Pf[M][M];         // a_{t|t}, P_{t|t}
  double u[M];                    // Z'y_t − σ²s_t = G a_{t|t}
};

// G⁻¹ (row-major M × M) by the pivoted elimination; false on an exact zero pivot
template <int M>
YFM_SHD bool gram_inverse(const double (&G)[M][M], double (&Ginv)[M * M]) {
  double A[M][M], X[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      A[i][j] = G[i][j];
      X[i][j] = (i == j) ? 1.0 : 0.0;
    }
  const bool ok = gauss_solve<M, M>(A, X);
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) Ginv[i * M + j] = X[i][j];
  return ok;
}

// a_{t|t} = G⁻¹(Z'y − σ²s), which is a + P s: G(a + P s) = G a + (B − σ²I)s = Z'y − σ²s.  It never adds P s to a, which
// cancels where a_t is large beside β̂_t (column 1 of a candidate with an eigenvalue of Φ near or past 1).
// Ginv = gram_inverse(G): the device forms it once per candidate and reads it from LDS
template <int M>
YFM_SHD void filtered_mean(const double* Ginv, const double (&a)[M], const double (&u)[M], bool missing,
                           double (&af)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double x = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) x = sfma(Ginv[i * M + k], u[k], x);
    af[i] = missing ? a[i] : x;
  }
}

// the chain's operands, P_{t|t} and u of a column (everything of StepOps but a_{t|t}); zy = Z'y_t (ignored at a missing
// column)
template <int M>
YFM_SHD void step_operands_core(const Model<M>& m, const double (&G)[M][M], const double (&a)[M],
                                const double (&P)[M][M], const double (&zy)[M], bool missing, StepOps<M>& o) {
  constexpr int R = 2 * M + 1;
  double Bm[M][M], X[M][R];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double c = zy[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = (i == j) ? m.sigma2 : 0.0;
#pragma unroll
      for (int l = 0; l < M; ++l) s = sfma(G[i][l], P[l][j], s);
      Bm[i][j] = s;
      X[i][j] = G[i][j];
      X[i][M + 1 + j] = (i == j) ? m.sigma2 : 0.0;
      c = sfma(-G[i][j], a[j], c);
    }
    X[i][M] = c;
  }
  gauss_solve<M, R>(Bm, X);
  // W is symmetric in exact arithmetic: the two triangles are averaged so that N stays symmetric to the bit
#pragma unroll
  for (int i = 0; i < M; ++i) {
    o.s[i] = missing ? 0.0 : X[i][M];
    o.u[i] = sfma(-m.sigma2, X[i][M], zy[i]);
#pragma unroll
    for (int j = i; j < M; ++j) {
      const double w = 0.5 * (X[i][j] + X[j][i]);
      o.W[i][j] = missing ? 0.0 : w;
      o.W[j][i] = o.W[i][j];
    }
  }
  // L = ΦE', E = σ²B⁻¹ = I − WP without the subtraction
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) s = sfma(m.Phi[i][k], X[j][M + 1 + k], s);
      o.L[i][j] = missing ? m.Phi[i][j] : s;
    }
  // P_{t|t} = P E (upper triangle, mirrored)
#pragma unroll
  for (int i = 0; i < M; ++i) {
#pragma unroll
    for (int j = i; j < M; ++j) {
      double p = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) p = sfma(P[i][k], X[k][M + 1 + j], p);
      o.Pf[i][j] = missing ? P[i][j] : p;
      o.Pf[j][i] = o.Pf[i][j];
    }
  }
}

// all of StepOps, with G⁻¹ formed here (the host driver's call; the device calls the two pieces)
template <int M>
YFM_SHD void step_operands(const Model<M>& m, const double (&G)[M][M], const double (&a)[M], const double (&P)[M][M],
                           const double (&zy)[M], bool missing, StepOps<M>& o) {
  double Ginv[M * M];
  gram_inverse<M>(G, Ginv);
  step_operands_core<M>(m, G, a, P, zy, missing, o);
  filtered_mean<M>(Ginv, a, o.u, missing, o.af);
}

// r ← s + L'r,  N ← W + L'NL (upper triangle, mirrored)
template <int M>
YFM_SHD void chain_step(const double (&s)[M], const double (&W)[M][M], const double (&L)[M][M], double (&r)[M],
                        double (&N)[M][M]) {
  double rn[M], T[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double x = s[i];
#pragma unroll
    for (int k = 0; k < M; ++k) x = sfma(L[k][i], r[k], x);
    rn[i] = x;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) t = sfma(N[i][k], L[k][j], t);
      T[i][j] = t;
    }
  }
#pragma unroll
  for (int i = 0; i < M; ++i) {
    r[i] = rn[i];
#pragma unroll
    for (int j = i; j < M; ++j) {
      double x = W[i][j];
#pragma unroll
      for (int k = 0; k < M; ++k) x = sfma(L[k][i], T[k][j], x);
      N[i][j] = x;
      N[j][i] = x;
    }
  }
}

// β̂_t, V_t and (lag: t < n, Pn = P_{t+1}) C_t from the column's filtered moments and r_t, N_t; false where an output
// is not finite
template <int M>
YFM_SHD bool step_outputs(const Model<M>& m, const double (&af)[M], const double (&Pf)[M][M], const double (&r)[M],
                          const double (&N)[M][M], bool lag, const double (&Pn)[M][M], double (&bs)[M],
                          double (&V)[M][M], double (&C)[M][M]) {
  double X[M][M], T[M][M];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) s = sfma(m.Phi[i][k], Pf[k][j], s);
      X[i][j] = s;
    }
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = af[i];
#pragma unroll
    for (int k = 0; k < M; ++k) s = sfma(X[k][i], r[k], s);
    bs[i] = s;
    ok = ok && finite(s);
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) t = sfma(N[i][k], X[k][j], t);
      T[i][j] = t;  // N_t X_t
    }
  }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = i; j < M; ++j) {
      double v = Pf[i][j];
#pragma unroll
      for (int k = 0; k < M; ++k) v = sfma(-X[k][i], T[k][j], v);
      V[i][j] = v;
      V[j][i] = v;
      ok = ok && finite(v);
    }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double c = X[i][j];
#pragma unroll
      for (int k = 0; k < M; ++k) c = sfma(-Pn[i][k], T[k][j], c);
      C[i][j] = c;
      ok = ok && (!lag || finite(c));
    }
  return ok;
}

// a_{t+1} = δ + Φa_{t|t},  P_{t+1} = ΦP_{t|t}Φ' + Q: the host's stand-in for the moments the device reads from the
// forward launch's record
template <int M>
YFM_SHD void predict(const Model<M>& m, const double (&af)[M], const double (&Pf)[M][M], double (&a)[M],
                     double (&P)[M][M]) {
  double X[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double s = m.delta[i];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      s = sfma(m.Phi[i][j], af[j], s);
      double x = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) x = sfma(m.Phi[i][k], Pf[k][j], x);
      X[i][j] = x;
    }
    a[i] = s;
  }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = i; j < M; ++j) {
      double s = m.Q[i][j];
#pragma unroll
      for (int k = 0; k < M; ++k) s = sfma(X[i][k], m.Phi[j][k], s);
      P[i][j] = s;
      P[j][i] = s;
    }
}

}  // namespace smooth
}  // namespace yfm
