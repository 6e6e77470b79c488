// yfm_grad.hpp — forward-mode tangents of the DNS log-likelihood (M = 3, P = 20), as plain functions
// that compile for the device (yfm_grad.hip) and for the host (tests/grad_host_check.cpp).
//
// Differentiates what the reference computes: get_loss (src/models/kalman/filter.jl:182-209) over
// filter! (filter.jl:125-179) from initialize_filter (filter.jl:1-10), as compute_loss sees it
// (src/optimization.jl:10-23; estimate! asks ForwardDiff for this gradient, optimization.jl:367).
//
// Primal: the collapsed form of yfm_fixedz.hpp, full recursion (no frozen covariance).  With G = Z'Z,
// R = σ²G⁻¹, ĉ = G⁻¹(0, z̃) + ȳe₁, c = ĉ − β, S = P + R, x = S⁻¹c, W = S⁻¹R:
//     q = r'r/σ² + c'x,  r'r = ỹ'ỹ − z̃'G⁻¹z̃,   log det F = (N − M) log σ² + log det G + log det S,
//     β_{t|t} = β + P x,  P_{t|t} = P W,  β⁺ = δ + Φ β_{t|t},  P⁺ = Φ P_{t|t} Φ' + Q.
// Tangents, per direction, reusing the factor of S (dS = dP + dR, A = I − W):
//     dx = S⁻¹(dc − dS x),   d(c'x) = 2x'dc − x'dS x,   d log det S = tr(S⁻¹dS),
//     dβ_{t|t} = dβ + dP x + P dx,   dP_{t|t} = W'dP W + A'dR A,
//     dβ⁺ = dδ + dΦ β_{t|t} + Φ dβ_{t|t},   dP⁺ = dΦ P_{t|t} Φ' + (·)' + Φ dP_{t|t} Φ' + dQ.
// The γ direction also moves Z: dz̃ = (∂Z/∂γ)'ỹ (a second pair of panel contractions per step), dG, dG⁻¹.
// Gradients are taken with respect to the constrained parameters and multiplied by dθ_c/dθ at the end.
// Every fused multiply-add is an explicit fma; contraction is off.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YFM_GHD __host__ __device__ __forceinline__
#else
#include <math.h>
#define YFM_GHD inline
#endif

#include "yfm_kalman_map.hpp"  // the parameter map and the small solves, shared with the smoothers

namespace yfm {
namespace grad {

constexpr int kM = 3;
constexpr int kNP = 20;  // γ, σ², U (6, by column), δ (3), Φ (9, row-major)
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

YFM_GHD double gfma(double a, double b, double c) { return __builtin_fma(a, b, c); }

using kalman::gauss_solve;

// LDLᵀ of a symmetric 3×3 (lower triangle read), as yfm_device.hpp's LDLT with IEEE reciprocals
struct Ldlt3 {
  double L[3][3], rd[3];
  YFM_GHD double factor(const double (&S)[3][3]) {
    double a[3][3], d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double dj = S[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj = gfma(-a[j][k], L[j][k], dj);
      d[j] = dj;
      rd[j] = 1.0 / dj;
#pragma unroll
      for (int i = j + 1; i < 3; ++i) {
        double s = S[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = gfma(-a[i][k], L[j][k], s);
        a[i][j] = s;
        L[i][j] = s * rd[j];
      }
    }
    return d[0] * d[1] * d[2];
  }
  YFM_GHD void solve(double (&x)[3]) const {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s = x[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = gfma(-L[i][k], x[k], s);
      x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] *= rd[i];
#pragma unroll
    for (int i = 2; i >= 0; --i) {
      double s = x[i];
#pragma unroll
      for (int k = i + 1; k < 3; ++k) s = gfma(-L[k][i], x[k], s);
      x[i] = s;
    }
  }
};

// ---- parameters -------------------------------------------------------------------------------
struct Model {
  double gam, sigma2;
  double U[3][3], Q[3][3], delta[3], Phi[3][3];
};

// transform_params (space == 0) + set_params! for DNS
YFM_GHD void decode(const double* th, int space, Model& m) {
  kalman::decode<3, 1>(th, space, &m.gam, m.sigma2, m.U, m.Q, m.delta, m.Phi);
}

// dθ_c[d]/dθ[d] (the exp rows 1, 2, 4, 7, the Φ-diagonal rows 11, 15, 19)
YFM_GHD double chain_factor(const double* th, int space, int d) { return kalman::chain_factor<kM, 1>(th, space, d); }

// DNS loadings of one maturity (dns.jl:51-65) and their γ-derivatives: with κ = e^γ/λ (dτ/dγ = τκ),
// dZ₁ = −Z₂κ, dZ₂ = κ(zτ − Z₂)
YFM_GHD void loadings(double gam, double mat, double& z1, double& z2, double& d1, double& d2) {
  const double eg = exp(gam);
  const double lam = 1e-2 + eg;
  const double kap = eg / lam;
  const double tau = lam * mat;
  const double z = exp(-tau);
  z1 = (1.0 - z) / tau;
  z2 = z1 - z;
  d1 = -z2 * kap;
  d2 = kap * gfma(z, tau, -z2);
}

// Σ Z₁, Σ Z₂, Σ Z₁², Σ Z₁Z₂, Σ Z₂² and their γ-derivatives, one maturity at a time
YFM_GHD void gram_add(double z1, double z2, double d1, double d2, double (&gs)[5], double (&dgs)[5]) {
  gs[0] += z1;
  gs[1] += z2;
  gs[2] = gfma(z1, z1, gs[2]);
  gs[3] = gfma(z1, z2, gs[3]);
  gs[4] = gfma(z2, z2, gs[4]);
  dgs[0] += d1;
  dgs[1] += d2;
  dgs[2] = gfma(2.0 * z1, d1, dgs[2]);
  dgs[3] = gfma(d1, z2, gfma(z1, d2, dgs[3]));
  dgs[4] = gfma(2.0 * z2, d2, dgs[4]);
}

// ---- per-candidate constants --------------------------------------------------------------------
struct Common {
  Model m;
  int N;
  double rsig2;
  double Ginv[3][3], dGinv[3][3];  // (Z'Z)⁻¹ and its γ-derivative −G⁻¹ dG G⁻¹
  double R[3][3], dRg[3][3];      // σ²G⁻¹ and its γ-derivative (its σ²-derivative is G⁻¹)
  double logdetG, dlogdetG;        // log det G, tr(G⁻¹dG)
};

YFM_GHD void setup_common(Common& c, const double (&gs)[5], const double (&dgs)[5], int N) {
  c.N = N;
  c.rsig2 = 1.0 / c.m.sigma2;
  const double G[3][3] = {{(double)N, gs[0], gs[1]}, {gs[0], gs[2], gs[3]}, {gs[1], gs[3], gs[4]}};
  const double dG[3][3] = {{0.0, dgs[0], dgs[1]}, {dgs[0], dgs[2], dgs[3]}, {dgs[1], dgs[3], dgs[4]}};
  double A[3][3], X[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[i][j] = G[i][j];
      X[i][j] = (i == j) ? 1.0 : 0.0;
    }
  gauss_solve<3, 3>(A, X);
  c.logdetG = log(fabs(A[0][0] * A[1][1] * A[2][2]));
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c.Ginv[i][j] = 0.5 * (X[i][j] + X[j][i]);
  double Tm[3][3];  // dG G⁻¹
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s = gfma(dG[i][k], c.Ginv[k][j], s);
      Tm[i][j] = s;
      tr = gfma(c.Ginv[i][j], dG[i][j], tr);
    }
  c.dlogdetG = tr;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s = gfma(-c.Ginv[i][k], Tm[k][j], s);
      c.dGinv[i][j] = s;
      c.dGinv[j][i] = s;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      c.R[i][j] = c.m.sigma2 * c.Ginv[i][j];
      c.dRg[i][j] = c.m.sigma2 * c.dGinv[i][j];
    }
}

// ---- filter state and one tangent direction ----------------------------------------------------------
struct State {
  double beta[3], P[3][3];
  double sumq = 0.0, sumld = 0.0;      // Σ q_t, Σ log det S_t over the accumulated steps
  double last_q = 0.0, last_ld = 0.0;  // the stale term a NaN column adds again (filter.jl:195)
  bool neg = false;                    // a negative det S: the reference's DomainError → −Inf
};

// which seeds a direction can carry (compile time): G the γ and σ² directions (dR, dz̃, dσ²), Q the
// U directions, D the δ directions, F the Φ directions.  Seeds outside the mask are never read.
constexpr int kSeedG = 1, kSeedQ = 2, kSeedD = 4, kSeedF = 8, kSeedAll = 15;

struct Tangent {
  double dPhi[3][3], dQ[3][3], ddelta[3];
  double fg, fs;  // 1 for the γ / the σ² direction
  double dbeta[3], dP[3][3];
  double acc = 0.0, last = 0.0;  // Σ d(log det S + q) and the stale term
};

// the seeds of direction d (θ_c index; d ≥ kNP: a padding direction, all zero)
template <int MASK>
YFM_GHD void seed(const Model& m, int d, Tangent& t) {
  t.fg = ((MASK & kSeedG) && d == 0) ? 1.0 : 0.0;
  t.fs = ((MASK & kSeedG) && d == 1) ? 1.0 : 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t.ddelta[a] = ((MASK & kSeedD) && d == 8 + a) ? 1.0 : 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      t.dPhi[a][b] = ((MASK & kSeedF) && d == 11 + 3 * a + b) ? 1.0 : 0.0;
      t.dQ[a][b] = 0.0;
    }
  }
  if (MASK & kSeedQ) {
    // U_ij (i ≤ j) is θ_c[2 + j(j+1)/2 + i]; Q = U'U: dQ_ab = δ_aj U_ib + U_ia δ_bj
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i <= j; ++i) {
        const double f = (d == 2 + j * (j + 1) / 2 + i) ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            double v = 0.0;
            if (a == j) v += m.U[i][b];
            if (b == j) v += m.U[i][a];
            t.dQ[a][b] = gfma(f, v, t.dQ[a][b]);
          }
      }
  }
}

using kalman::lyapunov_matrix;  // the symmetric-subspace operator of P − ΦPΦ' = Q

// initialize_filter (filter.jl:1-10) and its tangents through both solves:
//   (I − Φ) dβ₀ = dδ + dΦ β₀,    dP₀ − Φ dP₀ Φ' = dQ + dΦ P₀ Φ' + Φ P₀ dΦ'
template <int ND>
YFM_GHD void init_state(const Common& c, State& s, Tangent (&t)[ND]) {
  const Model& m = c.m;
  double X[3][4];
  kalman::mean_solve<3, 4>(m.Phi, m.delta, X);  // β₀ and (I − Φ)⁻¹
#pragma unroll
  for (int i = 0; i < 3; ++i) s.beta[i] = X[i][0];
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    double rhs[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double v = t[k].ddelta[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) v = gfma(t[k].dPhi[i][j], s.beta[j], v);
      rhs[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) v = gfma(X[i][1 + j], rhs[j], v);
      t[k].dbeta[i] = v;
    }
  }
  {
    double L[6][6], q[6][1];
    lyapunov_matrix(m.Phi, L);
    int r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) q[r++][0] = m.Q[i][j];
    gauss_solve<6, 1>(L, q);
    r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        s.P[i][j] = q[r][0];
        s.P[j][i] = q[r][0];
        ++r;
      }
  }
  double L[6][6], q[6][ND];
  lyapunov_matrix(m.Phi, L);
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    double PF[3][3], Y[3][3];  // P₀Φ', dΦ P₀ Φ'
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double v = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l) v = gfma(s.P[i][l], m.Phi[j][l], v);
        PF[i][j] = v;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double v = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l) v = gfma(t[k].dPhi[i][l], PF[l][j], v);
        Y[i][j] = v;
      }
    int r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) q[r++][k] = t[k].dQ[i][j] + (Y[i][j] + Y[j][i]);
  }
  gauss_solve<6, ND>(L, q);
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        t[k].dP[i][j] = q[r][k];
        t[k].dP[j][i] = q[r][k];
        ++r;
      }
  }
}

// ---- one data step: the primal update and what the tangents reuse from it --------------------------------
struct Step {
  double x[3], Sinv[3][3], W[3][3];
  double bf[3], Pf[3][3];
  double dchp[3];  // γ-derivative of ĉ
  double rr, drr;  // r'r and its γ-derivative
};

// z = (z̃₁, z̃₂) = Z'ỹ_t, dz its γ-derivative, ybar = ȳ_t, ytt = ỹ'ỹ
YFM_GHD void primal_update(const Common& c, const State& s, const double (&z)[2], const double (&dz)[2], double ybar,
                           double ytt, Step& u, double& det, double& q) {
  double chp[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    chp[i] = gfma(c.Ginv[i][2], z[1], c.Ginv[i][1] * z[0]);
    u.dchp[i] = gfma(c.Ginv[i][2], dz[1], gfma(c.Ginv[i][1], dz[0], gfma(c.dGinv[i][2], z[1], c.dGinv[i][1] * z[0])));
  }
  u.rr = gfma(-z[1], chp[2], gfma(-z[0], chp[1], ytt));
  u.drr = -gfma(z[1], u.dchp[2], gfma(z[0], u.dchp[1], gfma(dz[1], chp[2], dz[0] * chp[1])));
  double cc[3], S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cc[i] = (chp[i] + (i == 0 ? ybar : 0.0)) - s.beta[i];
    u.x[i] = cc[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) S[i][j] = s.P[i][j] + c.R[i][j];
  }
  Ldlt3 f;
  det = f.factor(S);
  f.solve(u.x);
  double cx = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) cx = gfma(cc[i], u.x[i], cx);
  q = gfma(u.rr, c.rsig2, cx);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double e[3], w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      e[i] = (i == j) ? 1.0 : 0.0;
      w[i] = c.R[i][j];
    }
    f.solve(e);
    f.solve(w);
#pragma unroll
    for (int i = 0; i < 3; ++i) u.W[i][j] = w[i];
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      u.Sinv[i][j] = e[i];
      u.Sinv[j][i] = e[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = s.beta[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) v = gfma(s.P[i][k], u.x[k], v);
    u.bf[i] = v;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v = gfma(s.P[i][k], u.W[k][j], v);
      u.Pf[i][j] = v;
      u.Pf[j][i] = v;
    }
}

// B'XB for a symmetric X (upper triangle computed, mirrored)
YFM_GHD void congruence(const double (&Bm)[3][3], const double (&X)[3][3], double (&out)[3][3]) {
  double Tm[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v = gfma(X[i][k], Bm[k][j], v);
      Tm[i][j] = v;
    }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v = gfma(Bm[k][i], Tm[k][j], v);
      out[i][j] = v;
      out[j][i] = v;
    }
}

// the tangent of one data step: returns d(log det S + q); dbf, dPf are the tangents of β_{t|t}, P_{t|t}
template <int MASK>
YFM_GHD double tangent_update(const Common& c, const State& s, const Step& u, const Tangent& t, double (&dbf)[3],
                              double (&dPf)[3][3]) {
  constexpr bool HG = (MASK & kSeedG) != 0;
  double dR[3][3], dS[3][3], dc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    dc[i] = HG ? gfma(t.fg, u.dchp[i], -t.dbeta[i]) : -t.dbeta[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dR[i][j] = HG ? gfma(t.fg, c.dRg[i][j], t.fs * c.Ginv[i][j]) : 0.0;
      dS[i][j] = HG ? t.dP[i][j] + dR[i][j] : t.dP[i][j];
    }
  }
  double us[3], w[3], dx[3];
  double dld = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      v = gfma(dS[i][j], u.x[j], v);
      dld = gfma(u.Sinv[i][j], dS[i][j], dld);
    }
    us[i] = v;
    w[i] = dc[i] - v;
  }
  double xdc = 0.0, xus = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) v = gfma(u.Sinv[i][j], w[j], v);
    dx[i] = v;
    xdc = gfma(u.x[i], dc[i], xdc);
    xus = gfma(u.x[i], us[i], xus);
  }
  double dq = gfma(2.0, xdc, -xus);
  if (HG) dq += gfma(t.fg * u.drr, c.rsig2, -(t.fs * u.rr) * (c.rsig2 * c.rsig2));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = t.dbeta[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) v = gfma(t.dP[i][k], u.x[k], gfma(s.P[i][k], dx[k], v));
    dbf[i] = v;
  }
  congruence(u.W, t.dP, dPf);
  if (HG) {
    double Am[3][3], E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Am[i][j] = (i == j ? 1.0 : 0.0) - u.W[i][j];
    congruence(Am, dR, E);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) dPf[i][j] += E[i][j];
  }
  return dld + dq;
}

// β⁺ = δ + Φ β_{t|t}, P⁺ = Φ P_{t|t} Φ' + Q (filter.jl:162-176) …
YFM_GHD void primal_predict(const Model& m, const double (&bf)[3], const double (&Pf)[3][3], State& s) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = m.delta[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) v = gfma(m.Phi[i][j], bf[j], v);
    s.beta[i] = v;
  }
  double A[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < 3; ++l) v = gfma(m.Phi[i][l], Pf[l][j], v);
      A[i][j] = v;
    }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double v = m.Q[i][j];
#pragma unroll
      for (int l = 0; l < 3; ++l) v = gfma(A[i][l], m.Phi[j][l], v);
      s.P[i][j] = v;
      s.P[j][i] = v;
    }
}

// … and its tangent (bf, Pf: the primal's filtered state of this step)
template <int MASK>
YFM_GHD void tangent_predict(const Model& m, const double (&bf)[3], const double (&Pf)[3][3], const double (&dbf)[3],
                             const double (&dPf)[3][3], Tangent& t) {
  constexpr bool HQ = (MASK & kSeedQ) != 0, HD = (MASK & kSeedD) != 0, HF = (MASK & kSeedF) != 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = HD ? t.ddelta[i] : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      v = gfma(m.Phi[i][j], dbf[j], v);
      if (HF) v = gfma(t.dPhi[i][j], bf[j], v);
    }
    t.dbeta[i] = v;
  }
  double A[3][3], Y[3][3];  // Φ dP_{t|t} + dΦ P_{t|t};  Y = Φ P_{t|t} dΦ'
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = 0.0, y = 0.0;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        v = gfma(m.Phi[i][l], dPf[l][j], v);
        if (HF) v = gfma(t.dPhi[i][l], Pf[l][j], v);
        if (HF) y = gfma(m.Phi[i][l], Pf[l][j], y);
      }
      A[i][j] = v;
      Y[i][j] = y;
    }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double v = HQ ? t.dQ[i][j] : 0.0;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        v = gfma(A[i][l], m.Phi[j][l], v);
        if (HF) v = gfma(Y[i][l], t.dPhi[j][l], v);
      }
      t.dP[i][j] = v;
      t.dP[j][i] = v;
    }
}

// One filter! call and its share of get_loss (filter.jl:190-206) for the primal …
//   data step: `acc` (Julia t > 1) adds log det S + q; the term is kept for a later NaN column
YFM_GHD void primal_account(State& s, double det, double q, bool acc) {
  s.last_ld = log(fabs(det));
  s.last_q = q;
  s.neg = s.neg || (acc && det < 0.0);
  if (acc) {
    s.sumld += s.last_ld;
    s.sumq += q;
  }
}
//   NaN column: prediction only (filter.jl:126-140); F and v are stale, so the last term is added again
YFM_GHD void primal_nan_step(const Model& m, State& s, bool acc) {
  double bf[3], Pf[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    bf[i] = s.beta[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) Pf[i][j] = s.P[i][j];
  }
  if (acc) {
    s.sumld += s.last_ld;
    s.sumq += s.last_q;
  }
  primal_predict(m, bf, Pf, s);
}
// … and for a tangent: the same two cases (call the tangent's before the primal's predict: both read β, P)
template <int MASK>
YFM_GHD void tangent_data_step(const Common& c, const State& s, const Step& u, Tangent& t, bool acc) {
  double dbf[3], dPf[3][3];
  const double term = tangent_update<MASK>(c, s, u, t, dbf, dPf);
  t.last = term;
  if (acc) t.acc += term;
  tangent_predict<MASK>(c.m, u.bf, u.Pf, dbf, dPf, t);
}
template <int MASK>
YFM_GHD void tangent_nan_step(const Common& c, const State& s, Tangent& t, bool acc) {
  double dbf[3], dPf[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    dbf[i] = t.dbeta[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) dPf[i][j] = t.dP[i][j];
  }
  if (acc) t.acc += t.last;
  tangent_predict<MASK>(c.m, s.beta, s.P, dbf, dPf, t);
}

// get_loss's value from the sums (nobs columns: nobs − 2 accumulated terms)
YFM_GHD double loglik_value(const Common& c, const State& s, int nobs) {
  const int nterms = nobs - 2 > 0 ? nobs - 2 : 0;
  if (nterms == 0) return 0.0;
  const double per_term = (double)(c.N - kM) * log(c.m.sigma2) + c.logdetG + (double)c.N * kLog2Pi;
  const double ll = -0.5 * ((double)nterms * per_term + s.sumld + s.sumq);
  const bool bad = s.neg || !(fabs(ll) <= 1.79769313486231570815e308);
  return bad ? -__builtin_inf() : ll;
}

// ∂(+loglik)/∂θ_c[d] from a tangent's sum; multiply by chain_factor for the unconstrained space
YFM_GHD double grad_value(const Common& c, const Tangent& t, int nobs) {
  const int nterms = nobs - 2 > 0 ? nobs - 2 : 0;
  const double dconst = gfma(t.fs * (double)(c.N - kM), c.rsig2, t.fg * c.dlogdetG);
  return -0.5 * gfma((double)nterms, dconst, t.acc);
}

// ∂ℓ_k/∂θ_c[d] of the step just taken, ℓ_k the term get_loss adds after column k: −½(dconst + last), with
// grad_value's dconst and the step's own (at a NaN column: the stale) tangent term; 0 for a step that is not
// accumulated (column 0).  Summed over a window's steps these are grad_value, up to the order of the sum.
YFM_GHD double score_value(const Common& c, const Tangent& t, bool acc) {
  const double dconst = gfma(t.fs * (double)(c.N - kM), c.rsig2, t.fg * c.dlogdetG);
  return acc ? -0.5 * (dconst + t.last) : 0.0;
}

}  // namespace grad
}  // namespace yfm
