// yfm_tvl_grad.hpp — forward-mode tangents of the TVλ extended-Kalman-filter log-likelihood (M = 4, P = 31), as
// plain functions that compile for the device (yfm_tvl_grad.hip) and for the host (tests/tvl_grad_host_check.cpp).
//
// Differentiates what the reference computes, not the textbook EKF: get_loss (src/models/kalman/filter.jl:182-209)
// over filter! (filter.jl:12-80) with update_factor_loadings! (src/models/kalman/tvλdns.jl:53-64) from
// initialize_filter (filter.jl:1-10), as compute_loss sees it (src/optimization.jl:10-23; estimate! asks
// ForwardDiff for this gradient, optimization.jl:367).  So the Jacobian column stays as written at filter.jl:43
// (dZ1 = z/λ − z/(λ²m)), t = 1 is not accumulated, the last column is unused, and a NaN column is a prediction-only
// step after which the stale F/v term and its tangent are added again.
//
// Primal: the capacitance form of yfm_tvl.hip.  With the loadings Z (N×4: 1, Z₂, Z₃ and the Jacobian column Z₄),
// the innovation v = y − Z[:,1:3]β[1:3] and G = Z'Z, u = Z'v:
//     B̃ = σ²I + P G,  W = B̃⁻¹P,  K v = W u,  P_{t|t} = σ² W,  q = (v'v − u'Wu)/σ²,
//     log det F = (N − 4) log σ² + log |det B̃|.
// The O(N) part is direction-free.  Z and v depend on θ only through the predicted state β = β_{t|t−1} — β₁..β₃
// linearly, β₄ through λ = 0.01 + e^{β₄} — so next to the 14 statistics of the step the maturity loop sums their
// partial derivatives with respect to β₂, β₃, β₄ (24 more moments; those with respect to β₁..β₃ of u and v'v are
// statistics already).  Per maturity, with dl = e^{β₄} = ∂λ/∂β₄, it = 1/(λm), k1 = (β₂+β₃)dl/λ, c2 = β₃dl and
// Z₄ = z·f, f = k1(1 − it) + c2·m:
//     ∂z/∂λ = −mz,  ∂Z₂/∂λ = (z − Z₂)/λ,  ∂Z₃/∂λ = ∂Z₂/∂λ + mz,
//     ∂Z₄/∂β₂ = z·(dl/λ)(1 − it),  ∂Z₄/∂β₃ = ∂Z₄/∂β₂ + z·dl·m,
//     ∂Z₄/∂β₄ = Z₄(1 − dl·m) + z·k1·(dl/λ)(2it − 1),
//     ∂v/∂β₁ = −1, ∂v/∂β₂ = −Z₂, ∂v/∂β₃ = −Z₃, ∂v/∂β₄ = −(β₂ ∂Z₂/∂λ + β₃ ∂Z₃/∂λ)·dl.
// Each direction then gets d(stat) = J_stat·dβ and 4×4 algebra that reuses the primal's factor (B̃⁻¹ is kept):
//     dB̃ = dσ²I + dP G + P dG,   d log|det B̃| = tr(B̃⁻¹dB̃),
//     dW = B̃⁻¹(dP − dB̃ W) = σ² B̃⁻¹dP B̃⁻ᵀ − W dG W − dσ² B̃⁻¹W   (I − G W = σ² B̃⁻ᵀ: the second form has no
//          difference that cancels by ‖PG‖/σ², and is symmetric term by term),
//     d(Kv) = dW u + W du,   dP_{t|t} = dσ² W + σ² dW,
//     σ² dq = d(v'v) − 2 du'Kv + (Kv)'dG (Kv) − σ² x'dP x + dσ² (x'Kv − q),   x = B̃⁻ᵀu = Z'F⁻¹v,
//     dβ⁺ = dδ + dΦ β_{t|t} + Φ dβ_{t|t},   dP⁺ = dΦ P_{t|t} Φ' + (·)' + Φ dP_{t|t} Φ' + dQ,
// and the initial state's tangent goes through both solves of initialize_filter.
// Gradients are taken with respect to the constrained parameters and multiplied by dθ_c/dθ at the end.
// Every fused multiply-add is an explicit fma; contraction is off.
#pragma once
#include "yfm_grad.hpp"  // gfma, YFM_GHD, and yfm_kalman_map.hpp through it
#include "yfm_tvl_step.hpp"  // the statistics of a step, shared with tvl_loglik_kernel

namespace yfm {
namespace tvlgrad {

using grad::gauss_solve;
using grad::gfma;
using namespace tvlstep;  // S2 … VV, NSTAT, Row, accum_stats, tvl_gram

constexpr int kM = 4;
constexpr int kNP = 31;  // σ², U (10, by column), δ (4), Φ (16, row-major)
constexpr int kOffU = 1, kOffD = 11, kOffF = 15;
constexpr double kLog2Pi = grad::kLog2Pi;
constexpr double kDblMax = 1.79769313486231570815e308;

YFM_GHD bool finite(double x) { return fabs(x) <= kDblMax; }

// ---- parameters -------------------------------------------------------------------------------
struct Model {
  double sigma2, rsig2;
  double U[4][4], Q[4][4], delta[4], Phi[4][4];
};

// transform_params (space == 0) + set_params! for TVλ.  (1/σ² is formed before the shared call, from the same select:
// formed after it, from m.sigma2, it moved tvl_grad_kernel<32, 1> by three instructions.)
YFM_GHD void decode(const double* th, int space, Model& m) {
  const double es = exp(th[0]);
  m.rsig2 = 1.0 / (space == 0 ? es : th[0]);
  kalman::decode<4, 0>(th, space, nullptr, m.sigma2, m.U, m.Q, m.delta, m.Phi);
}

// dθ_c[d]/dθ[d] (the exp rows 0, 1, 3, 6, 10, the Φ-diagonal rows 15, 20, 25, 30)
YFM_GHD double chain_factor(const double* th, int space, int d) { return kalman::chain_factor<kM, 0>(th, space, d); }

// ---- filter state and one tangent direction ----------------------------------------------------------
struct State {
  double beta[4], P[4][4];
  double sumq = 0.0, sumld = 0.0;      // Σ q_t, Σ log |det B̃_t| over the accumulated steps
  double last_q = 0.0, last_ld = 0.0;  // the stale term a NaN column adds again (filter.jl:195); a fresh model's is 0
  bool neg = false;                    // a negative det B̃ among the accumulated terms: the reference's DomainError → −Inf
  bool last_neg = false;
  bool bad = false;                    // a zero or non-finite det B̃ (inv(F) threw, filter.jl:51-56)
};

// which seeds a direction can carry (compile time): S the σ² direction, Q the U directions, D the δ directions,
// F the Φ directions.  Seeds outside the mask are never read.
constexpr int kSeedS = 1, kSeedQ = 2, kSeedD = 4, kSeedF = 8, kSeedAll = 15;

struct Tangent {
  int d;  // the direction (θ_c index; kNP: padding).  The seeds are functions of it (below), not stored values
  double dbeta[4], dP[4][4];
  double acc = 0.0, last = 0.0;  // Σ d(log |det B̃| + q) and the stale term
};
// dσ², dδ_a, dΦ = er·ec' (a unit matrix entry, or zero), dQ_ab = δ_{a,qj} U_{qi,b} + U_{qi,a} δ_{b,qj} (Q = U'U).
// U is read with a lane-dependent row: the kernel keeps the Model in LDS, where that is an address, not a select.
YFM_GHD double seed_fs(const Tangent& t) { return t.d == 0 ? 1.0 : 0.0; }
YFM_GHD double seed_dd(const Tangent& t, int a) { return t.d == kOffD + a ? 1.0 : 0.0; }
YFM_GHD double seed_er(const Tangent& t, int a) {
  const int f = t.d - kOffF;
  return (f >= 0 && f < 16 && (f >> 2) == a) ? 1.0 : 0.0;
}
YFM_GHD double seed_ec(const Tangent& t, int a) {
  const int f = t.d - kOffF;
  return (f >= 0 && f < 16 && (f & 3) == a) ? 1.0 : 0.0;
}
// U_{qi,qj} (qi ≤ qj) is θ_c[1 + qj(qj+1)/2 + qi]: the column and row of a U direction (qj = −1 otherwise; qi is
// always a valid row)
YFM_GHD void seed_u(const Tangent& t, int& qi, int& qj) {
  const int e = t.d - kOffU;
  qj = (e < 0 || e >= 10) ? -1 : (e >= 6 ? 3 : (e >= 3 ? 2 : (e >= 1 ? 1 : 0)));
  const int qc = qj < 0 ? 0 : qj;
  qi = qj < 0 ? 0 : e - qc * (qc + 1) / 2;
}
YFM_GHD double seed_dq(const Model& m, int qi, int qj, int a, int b) {
  const double* u = &m.U[0][0] + 4 * qi;
  return (a == qj ? u[b] : 0.0) + (b == qj ? u[a] : 0.0);
}

// The direction (θ_c index) of slot `slot` of lane j when a candidate has L lanes: the 15 directions before Φ fill
// the first ⌈15/L⌉ slots (the rest of the last of them is padding, direction kNP), the 16 entries of Φ the others,
// so no slot carries both the Φ seeds and the σ² / U / δ seeds.
constexpr int slots_before_phi(int L) { return L >= 32 ? 0 : (kOffF + L - 1) / L; }
YFM_GHD int slot_direction(int L, int slot, int j) {
  if (L >= 32) return j < kOffF ? j : (j >= 16 ? j - 1 : kNP);  // one slot: lane 15 is the padding
  const int s0 = slots_before_phi(L);
  if (slot < s0) return slot * L + j < kOffF ? slot * L + j : kNP;
  const int d = kOffF + (slot - s0) * L + j;
  return d < kNP ? d : kNP;
}

// direction d (θ_c index; d ≥ kNP: a padding direction, every seed zero)
YFM_GHD void seed(int d, Tangent& t) { t.d = d; }

using kalman::lyapunov_matrix;  // the symmetric-subspace operator of P − ΦPΦ' = Q

// column c of the inverse of that operator (the same pivots whichever column: every caller factors the same matrix)
YFM_GHD void lyapunov_inverse_column(const double (&Phi)[4][4], int c, double (&col)[10]) {
  double L[10][10], q[10][1];
  lyapunov_matrix(Phi, L);
#pragma unroll
  for (int r = 0; r < 10; ++r) q[r][0] = (r == c) ? 1.0 : 0.0;
  gauss_solve<10, 1>(L, q);
#pragma unroll
  for (int r = 0; r < 10; ++r) col[r] = q[r][0];
}

// x = Linv·rhs into the symmetric 4×4 X (Linv: the operator's inverse, row-major 10×10)
YFM_GHD void lyapunov_apply(const double* Linv, const double (&rhs)[10], double (&X)[4][4]) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int c = 0; c < 10; ++c) v = gfma(Linv[r * 10 + c], rhs[c], v);
      X[i][j] = v;
      X[j][i] = v;
      ++r;
    }
}

// initialize_filter (filter.jl:1-10) and its tangents through both solves:
//   (I − Φ) dβ₀ = dδ + dΦ β₀,    dP₀ − Φ dP₀ Φ' = dQ + dΦ P₀ Φ' + Φ P₀ dΦ'
// Linv: the inverse of the Lyapunov operator (lyapunov_inverse_column), which the kernel's lane group forms once,
// a column per lane, and shares; every direction then costs one 10×10 product.
template <int ND>
YFM_GHD void init_state(const Model& m, const double* Linv, State& s, Tangent (&t)[ND]) {
  double X[4][5];
  kalman::mean_solve<4, 5>(m.Phi, m.delta, X);  // β₀ and (I − Φ)⁻¹
#pragma unroll
  for (int i = 0; i < 4; ++i) s.beta[i] = X[i][0];
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    double cb = 0.0;  // ec'β₀
#pragma unroll
    for (int j = 0; j < 4; ++j) cb = gfma(seed_ec(t[k], j), s.beta[j], cb);
    double rhs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rhs[i] = gfma(seed_er(t[k], i), cb, seed_dd(t[k], i));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) v = gfma(X[i][1 + j], rhs[j], v);
      t[k].dbeta[i] = v;
    }
  }
  {
    double q[10];
    int r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) q[r++] = m.Q[i][j];
    lyapunov_apply(Linv, q, s.P);
  }
  double PF[4][4];  // P₀Φ'
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(s.P[i][l], m.Phi[j][l], v);
      PF[i][j] = v;
    }
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    double row[4];  // ec'P₀Φ': dΦ P₀ Φ' = er·row'
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(seed_ec(t[k], l), PF[l][j], v);
      row[j] = v;
    }
    double q[10];
    int r = 0, qi, qj;
    seed_u(t[k], qi, qj);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j)
        q[r++] = seed_dq(m, qi, qj, i, j) + gfma(seed_er(t[k], i), row[j], seed_er(t[k], j) * row[i]);
    lyapunov_apply(Linv, q, t[k].dP);
  }
}

// ---- the O(N) part of a data step: statistics and their state derivatives ------------------------------
// the statistics of one EKF step are tvlstep's (yfm_tvl_step.hpp); those that move with β₂ and β₃ beyond what other statistics already give: through Z₄
enum : int { JS4 = 0, JG24, JG34, JG44, JU4, NJ };

struct Moments {
  double s[NSTAT];   // the statistics
  double j3[NSTAT];  // ∂s/∂β₄
  double j1[NJ];     // ∂/∂β₂ of S4, G24, G34, G44 and the part of ∂U4/∂β₂ that is not −G24
  double j2[NJ];     // the same for β₃
};

YFM_GHD void moments_zero(Moments& mo) {
#pragma unroll
  for (int k = 0; k < NSTAT; ++k) mo.s[k] = mo.j3[k] = 0.0;
#pragma unroll
  for (int k = 0; k < NJ; ++k) mo.j1[k] = mo.j2[k] = 0.0;
}

// the per-step constants of the loadings (yfm_tvl.hip's, with its λ-overflow branch) and of their derivatives
struct StepConst {
  double lam, rl, dl;
  double c2, k1;   // Z₄ = z·(k1 − k1/(λm) + c2·m)
  double dr, dlb;  // ∂f/∂β₂ = dr(1 − it), ∂f/∂β₃ = that + dlb·m   (dr = dlb/λ)
  double kq;       // k1·dl/λ
  double el;       // dl/λ
};

// minm: the smallest maturity this lane owns (the overflow test is per lane, as in tvl_loglik_kernel)
YFM_GHD void step_consts(const double (&beta)[4], double minm, StepConst& k) {
  k.lam = 1e-2 + exp(beta[3]);  // tvλdns.jl:56
  k.rl = 1.0 / k.lam;
  k.dl = k.lam - 1e-2;  // filter.jl:38
  const double c1r = (beta[1] + beta[2]) * k.dl, c2r = beta[2] * k.dl;
  const bool big = !(k.lam * minm <= 746.0) || !(fabs(c1r) <= kDblMax) || !(fabs(c2r) <= kDblMax);
  const double c1 = big ? 0.0 * k.dl : c1r;
  k.c2 = big ? 0.0 * k.dl : c2r;
  k.k1 = c1 * k.rl;
  k.dlb = big ? 0.0 * k.dl : k.dl;  // the branch taken has constant (zero) coefficients
  k.dr = k.dlb * k.rl;
  k.el = k.dl * k.rl;
  k.kq = k.k1 * k.el;
}

// one maturity m (rm = 1/m) with z = e^{−λm} and yield y
YFM_GHD void accum(const StepConst& k, const double (&beta)[4], double m, double rm, double z, double y, Moments& mo) {
  Row r;
  accum_stats(k.rl, k.k1, k.c2, beta, m, rm, z, y, mo.s, r);
  const double it = r.it, z2 = r.z2, z3 = r.z3, z4 = r.z4, v = r.v;
  // derivatives with respect to β₄ (∂λ/∂β₄ = dl) …
  const double mzd = (m * z) * k.dl;
  const double e2 = (z - z2) * k.el;  // ∂Z₂/∂β₄
  const double e3 = e2 + mzd;         // ∂Z₃/∂β₄
  const double p3 = gfma(z4, gfma(-k.dl, m, 1.0), z * (k.kq * gfma(2.0, it, -1.0)));  // ∂Z₄/∂β₄
  const double vl = -gfma(beta[2], e3, beta[1] * e2);                                  // ∂v/∂β₄
  // … and of Z₄ with respect to β₂, β₃
  const double a = k.dr * (1.0 - it);
  const double p1 = z * a;
  const double p2 = z * gfma(k.dlb, m, a);
  double* j3 = mo.j3;
  j3[S2] += e2;
  j3[S3] += e3;
  j3[S4] += p3;
  j3[G22] = gfma(2.0 * z2, e2, j3[G22]);
  j3[G23] = gfma(e2, z3, gfma(z2, e3, j3[G23]));
  j3[G24] = gfma(e2, z4, gfma(z2, p3, j3[G24]));
  j3[G33] = gfma(2.0 * z3, e3, j3[G33]);
  j3[G34] = gfma(e3, z4, gfma(z3, p3, j3[G34]));
  j3[G44] = gfma(2.0 * z4, p3, j3[G44]);
  j3[U1] += vl;
  j3[U2] = gfma(e2, v, gfma(z2, vl, j3[U2]));
  j3[U3] = gfma(e3, v, gfma(z3, vl, j3[U3]));
  j3[U4] = gfma(p3, v, gfma(z4, vl, j3[U4]));
  j3[VV] = gfma(2.0 * v, vl, j3[VV]);
  mo.j1[JS4] += p1;
  mo.j1[JG24] = gfma(z2, p1, mo.j1[JG24]);
  mo.j1[JG34] = gfma(z3, p1, mo.j1[JG34]);
  mo.j1[JG44] = gfma(2.0 * z4, p1, mo.j1[JG44]);
  mo.j1[JU4] = gfma(p1, v, mo.j1[JU4]);
  mo.j2[JS4] += p2;
  mo.j2[JG24] = gfma(z2, p2, mo.j2[JG24]);
  mo.j2[JG34] = gfma(z3, p2, mo.j2[JG34]);
  mo.j2[JG44] = gfma(2.0 * z4, p2, mo.j2[JG44]);
  mo.j2[JU4] = gfma(p2, v, mo.j2[JU4]);
}

// ---- one data step: the primal update and what the tangents reuse from it --------------------------------
struct Step {
  double G[4][4], u[4], vv;
  double W[4][4], Binv[4][4];  // W = B̃⁻¹P (upper triangle mirrored, as the loglik kernel uses it), B̃⁻¹
  double trB;                  // tr B̃⁻¹
  double w[4], x[4];           // K v = W u;  x = B̃⁻ᵀu (= Z'F⁻¹v)
  double xw;                   // x'w
  double bf[4];                // β_{t|t};  P_{t|t} = σ² W is formed where it is used
  double det, q;
};

YFM_GHD void primal_update(const Model& m, const State& s, const Moments& mo, int N, Step& u) {
  const double* st = mo.s;
  tvl_gram(mo.s, N, u.G);
  u.u[0] = st[U1];
  u.u[1] = st[U2];
  u.u[2] = st[U3];
  u.u[3] = st[U4];
  u.vv = st[VV];
  // The capacitance solve in its symmetric form.  B̃ = σ²I + P G is not normal, and the LU of yfm_device.hpp's
  // Capacitance::solve loses cond₂(B̃)·ε in W — harmless to the value at the project's bar, but the tangents
  // amplify it (measured on the host: up to 3e-8 of ‖g‖∞ on the N = 7 fixture case).  With P = L J L', L lower
  // triangular and J = diag(±1) (a Cholesky factor that carries signs: a non-stationary Φ gives an indefinite P, and
  // the reference goes on filtering):
  //     B̃ = L J S L⁻¹,  S = σ²J + L'G L  (symmetric; for a positive definite P, cond S ≤ 1 + ‖L'GL‖/σ²),
  //     W = L S⁻¹ L',  B̃⁻¹ = L S⁻¹ J L⁻¹,  det B̃ = det J · det S.
  double L[4][4], Li[4][4], sg[4];
  double detJ = 1.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double d = s.P[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = gfma(-(sg[k] * L[j][k]), L[j][k], d);
    sg[j] = d < 0.0 ? -1.0 : 1.0;
    detJ = d < 0.0 ? -detJ : detJ;
    const double l = sqrt(fabs(d));
    const double r = 1.0 / l;
    L[j][j] = l;
    Li[j][j] = r;
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double v = s.P[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v = gfma(-(sg[k] * L[i][k]), L[j][k], v);
      L[i][j] = (v * r) * sg[j];
    }
  }
  // L⁻¹ (lower): column j by forward substitution
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) v = gfma(-L[i][k], Li[k][j], v);
      Li[i][j] = v * Li[i][i];
    }
  double A[4][4], X[4][4];
  {
    double Tm[4][4];  // G L
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double v = 0.0;
#pragma unroll
        for (int l = j; l < 4; ++l) v = gfma(u.G[k][l], L[l][j], v);
        Tm[k][j] = v;
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) {
        double v = (i == j) ? m.sigma2 * sg[i] : 0.0;
#pragma unroll
        for (int k = i; k < 4; ++k) v = gfma(L[k][i], Tm[k][j], v);
        A[i][j] = v;
        A[j][i] = v;
        X[i][j] = (i == j) ? 1.0 : 0.0;
        X[j][i] = X[i][j];
      }
  }
  // S⁻¹ column by column from the LDLᵀ of S (no pivoting: the symmetric solve keeps the error of S⁻¹ structured,
  // where an LU's unsymmetric one cost up to 6e-8 of ‖g‖∞ on the fixture); det S = ∏ d_i carries its sign
  double Lf[4][4], rd[4];
  double prod = 1.0;
  {
    double a[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double dj = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj = gfma(-a[j][k], Lf[j][k], dj);
      prod *= dj;
      rd[j] = 1.0 / dj;
#pragma unroll
      for (int i = j + 1; i < 4; ++i) {
        double v = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v = gfma(-a[i][k], Lf[j][k], v);
        a[i][j] = v;
        Lf[i][j] = v * rd[j];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) v = gfma(-Lf[i][k], x[k], v);
      x[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] *= rd[i];
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      double v = x[i];
#pragma unroll
      for (int k = i + 1; k < 4; ++k) v = gfma(-Lf[k][i], x[k], v);
      x[i] = v;
    }
#pragma unroll
    for (int i = 0; i <= c; ++i) {
      X[i][c] = x[i];
      X[c][i] = x[i];
    }
  }
  u.det = prod * detJ;
  {
    double LY[4][4];  // L S⁻¹
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k <= i; ++k) v = gfma(L[i][k], X[k][j], v);
        LY[i][j] = v;
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double b = 0.0;
#pragma unroll
        for (int l = j; l < 4; ++l) b = gfma(LY[i][l] * sg[l], Li[l][j], b);
        u.Binv[i][j] = b;
        if (i <= j) {
          double w = 0.0;
#pragma unroll
          for (int l = 0; l <= j; ++l) w = gfma(LY[i][l], L[j][l], w);
          u.W[i][j] = w;
          u.W[j][i] = w;
        }
      }
  }
  double uk = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double w = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) w = gfma(u.W[i][k], u.u[k], w);
    u.w[i] = w;
    u.bf[i] = s.beta[i] + w;
    uk = gfma(u.u[i], w, uk);
  }
  u.q = (u.vv - uk) * m.rsig2;
  u.trB = ((u.Binv[0][0] + u.Binv[1][1]) + u.Binv[2][2]) + u.Binv[3][3];
  u.xw = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double x = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) x = gfma(u.Binv[k][i], u.u[k], x);
    u.x[i] = x;
    u.xw = gfma(x, u.w[i], u.xw);
  }
}

// the tangent of one data step: returns d(log |det B̃| + q); dbf, dPf are the tangents of β_{t|t}, P_{t|t}
template <int MASK>
YFM_GHD double tangent_update(const Model& m, const State& s, const Step& u, const Moments& mo, int N, const Tangent& t,
                              double (&dbf)[4], double (&dPf)[4][4]) {
  constexpr bool HS = (MASK & kSeedS) != 0;
  const double b0 = t.dbeta[0], b1 = t.dbeta[1], b2 = t.dbeta[2], b3 = t.dbeta[3];
  const double fs = HS ? seed_fs(t) : 0.0;
  const double* st = mo.s;
  const double* j3 = mo.j3;
  // d(stat) = J_stat·dβ
  double dG[4][4], du[4];
  dG[0][0] = 0.0;
  dG[0][1] = dG[1][0] = j3[S2] * b3;
  dG[0][2] = dG[2][0] = j3[S3] * b3;
  dG[0][3] = dG[3][0] = gfma(mo.j1[JS4], b1, gfma(mo.j2[JS4], b2, j3[S4] * b3));
  dG[1][1] = j3[G22] * b3;
  dG[1][2] = dG[2][1] = j3[G23] * b3;
  dG[1][3] = dG[3][1] = gfma(mo.j1[JG24], b1, gfma(mo.j2[JG24], b2, j3[G24] * b3));
  dG[2][2] = j3[G33] * b3;
  dG[2][3] = dG[3][2] = gfma(mo.j1[JG34], b1, gfma(mo.j2[JG34], b2, j3[G34] * b3));
  dG[3][3] = gfma(mo.j1[JG44], b1, gfma(mo.j2[JG44], b2, j3[G44] * b3));
  du[0] = gfma(-(double)N, b0, gfma(-st[S2], b1, gfma(-st[S3], b2, j3[U1] * b3)));
  du[1] = gfma(-st[S2], b0, gfma(-st[G22], b1, gfma(-st[G23], b2, j3[U2] * b3)));
  du[2] = gfma(-st[S3], b0, gfma(-st[G23], b1, gfma(-st[G33], b2, j3[U3] * b3)));
  du[3] = gfma(-st[S4], b0, gfma(mo.j1[JU4] - st[G24], b1, gfma(mo.j2[JU4] - st[G34], b2, j3[U4] * b3)));
  const double dvv = gfma(-2.0 * st[U1], b0, gfma(-2.0 * st[U2], b1, gfma(-2.0 * st[U3], b2, j3[VV] * b3)));
  // dW = σ² B̃⁻¹ dP B̃⁻ᵀ − W dG W − dσ² B̃⁻¹W: with I − G W = σ² B̃⁻ᵀ the difference dP − dB̃ W is never formed
  // (it cancels by (PG)/σ²), and every term is a congruence, so dW is symmetric as W is
  // row by row (Tm = B̃⁻¹dP and W dG are never whole in registers);
  // d log |det B̃| = tr(B̃⁻¹dB̃) = dσ² tr B̃⁻¹ + tr(G B̃⁻¹dP) + tr(W dG)
  double dW[4][4];
  double dld = HS ? fs * u.trB : 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double ti[4], hi[4];  // row i of B̃⁻¹dP and of W dG
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 0.0, h = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        v = gfma(u.Binv[i][l], t.dP[l][j], v);
        h = gfma(u.W[i][l], dG[l][j], h);
      }
      ti[j] = v;
      hi[j] = h;
      dld = gfma(v, u.G[j][i], dld);
    }
    dld += hi[i];
#pragma unroll
    for (int j = i; j < 4; ++j) {
      double e = 0.0, wd = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        e = gfma(ti[l], u.Binv[j][l], e);
        wd = gfma(hi[l], u.W[l][j], wd);
      }
      double v = gfma(m.sigma2, e, -wd);
      if (HS) {
        double bw = 0.0;  // (B̃⁻¹W)_ij, symmetric
#pragma unroll
        for (int l = 0; l < 4; ++l) bw = gfma(u.Binv[i][l], u.W[l][j], bw);
        v = gfma(-fs, bw, v);
      }
      dW[i][j] = v;
      dW[j][i] = v;
    }
  }
  // d(Kv) = dW u + W du;  σ² dq = d(v'v) − 2 du'Kv − u'dW u − q dσ², u'dW u = σ² x'dP x − w'dG w − dσ² x'w (x = B̃⁻ᵀu)
  double duw = 0.0, wgw = 0.0, xpx = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double v = 0.0, gw = 0.0, px = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v = gfma(dW[i][k], u.u[k], gfma(u.W[i][k], du[k], v));
      gw = gfma(dG[i][k], u.w[k], gw);
      px = gfma(t.dP[i][k], u.x[k], px);
    }
    dbf[i] = t.dbeta[i] + v;
    duw = gfma(du[i], u.w[i], duw);
    wgw = gfma(u.w[i], gw, wgw);
    xpx = gfma(u.x[i], px, xpx);
  }
  double dq = gfma(-xpx, 1.0, (gfma(-2.0, duw, dvv) + wgw) * m.rsig2);
  if (HS) dq = gfma(fs * (u.xw - u.q), m.rsig2, dq);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      double v = m.sigma2 * dW[i][j];
      if (HS) v = gfma(fs, u.W[i][j], v);
      dPf[i][j] = v;
      dPf[j][i] = v;
    }
  return dld + dq;
}

// β⁺ = δ + Φ β_{t|t}, P⁺ = Φ P_{t|t} Φ' + Q (filter.jl:162-176), P_{t|t} = sc·X (σ²W after data, 1·P after a NaN column) …
YFM_GHD void primal_predict(const Model& m, const double (&bf)[4], const double (&X)[4][4], double sc, State& s) {
  double bn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double v = m.delta[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v = gfma(m.Phi[i][j], bf[j], v);
    bn[i] = v;
  }
  double A[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(m.Phi[i][l], sc * X[l][j], v);
      A[i][j] = v;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) s.beta[i] = bn[i];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double v = m.Q[i][j];
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(A[i][l], m.Phi[j][l], v);
      s.P[i][j] = v;
      s.P[j][i] = v;
    }
}

// … and its tangent (bf, sc·X: the primal's filtered state of this step)
template <int MASK>
YFM_GHD void tangent_predict(const Model& m, const double (&bf)[4], const double (&X)[4][4], double sc,
                             const double (&dbf)[4], const double (&dPf)[4][4], Tangent& t) {
  constexpr bool HQ = (MASK & kSeedQ) != 0, HD = (MASK & kSeedD) != 0, HF = (MASK & kSeedF) != 0;
  double cb = 0.0;  // ec'β_{t|t}: dΦ β_{t|t} = er·cb
  if (HF) {
#pragma unroll
    for (int j = 0; j < 4; ++j) cb = gfma(seed_ec(t, j), bf[j], cb);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double v = HD ? seed_dd(t, i) : 0.0;
    if (HF) v = gfma(seed_er(t, i), cb, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v = gfma(m.Phi[i][j], dbf[j], v);
    t.dbeta[i] = v;
  }
  double A[4][4];  // Φ dP_{t|t}
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(m.Phi[i][l], dPf[l][j], v);
      A[i][j] = v;
    }
  double row[4];  // ec'P_{t|t}Φ': dΦ P_{t|t} Φ' = er·row'
  int qi = 0, qj = -1;
  if (HQ) seed_u(t, qi, qj);
  if (HF) {
    double pe[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v = gfma(seed_ec(t, k), X[k][l], v);
      pe[l] = sc * v;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(pe[l], m.Phi[j][l], v);
      row[j] = v;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i <= j; ++i) {
      double v = HQ ? seed_dq(m, qi, qj, i, j) : 0.0;
#pragma unroll
      for (int l = 0; l < 4; ++l) v = gfma(A[i][l], m.Phi[j][l], v);
      if (HF) v += gfma(seed_er(t, i), row[j], seed_er(t, j) * row[i]);
      t.dP[i][j] = v;
      t.dP[j][i] = v;
    }
}

// One filter! call and its share of get_loss (filter.jl:190-206).  A NaN column is a prediction-only step
// (filter.jl:13-29): F and v stay stale, so get_loss adds the last term — and its tangent — again.  Both kinds of
// column run the same code: the update is computed either way (from NaN data it is garbage) and selects keep the
// predicted state and the stale terms on a NaN column, so the kernel has one path and no divergence.
struct Filtered {
  double bf[4], X[4][4], sc;  // β_{t|t} and P_{t|t} = sc·X: (σ², W) after data, (1, P) after a NaN column
};
YFM_GHD void filtered_state(const Model& m, const State& s, const Step& u, bool nan, Filtered& f) {
  f.sc = nan ? 1.0 : m.sigma2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f.bf[i] = nan ? s.beta[i] : u.bf[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) f.X[i][j] = nan ? s.P[i][j] : u.W[i][j];
  }
}
// the tangent's step (call it before primal_step: both read β, P)
template <int MASK>
YFM_GHD void tangent_step(const Model& m, const State& s, const Step& u, const Moments& mo, int N, const Filtered& f,
                          bool nan, Tangent& t, bool acc) {
  double dbf[4], dPf[4][4];
  const double fresh = tangent_update<MASK>(m, s, u, mo, N, t, dbf, dPf);
  const double term = nan ? t.last : fresh;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    dbf[i] = nan ? t.dbeta[i] : dbf[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) dPf[i][j] = nan ? t.dP[i][j] : dPf[i][j];
  }
  t.last = term;
  if (acc) t.acc += term;
  tangent_predict<MASK>(m, f.bf, f.X, f.sc, dbf, dPf, t);
}
// the primal's: `acc` (Julia t > 1) adds log |det B̃| + q of this column, or the stale ones
YFM_GHD void primal_step(const Model& m, const Step& u, const Filtered& f, bool nan, State& s, bool acc) {
  s.bad = s.bad || (!nan && (!(u.det != 0.0) || !finite(u.det)));
  const double ld = log(fabs(u.det));
  s.last_ld = nan ? s.last_ld : ld;
  s.last_q = nan ? s.last_q : u.q;
  s.last_neg = nan ? s.last_neg : u.det < 0.0;
  if (acc) {
    s.neg = s.neg || s.last_neg;
    s.sumld += s.last_ld;
    s.sumq += s.last_q;
  }
  primal_predict(m, f.bf, f.X, f.sc, s);
}

// get_loss's value from the sums (nobs columns: nobs − 2 accumulated terms)
YFM_GHD double loglik_value(const Model& m, const State& s, int N, int nobs) {
  const int nterms = nobs - 2 > 0 ? nobs - 2 : 0;
  if (nterms == 0) return 0.0;
  const double per_term = (double)(N - kM) * log(m.sigma2) + (double)N * kLog2Pi;
  const double ll = -0.5 * ((double)nterms * per_term + s.sumld + s.sumq);
  const bool bad = s.neg || s.bad || !finite(ll);
  return bad ? -__builtin_inf() : ll;
}

// this recursion's own value is usable: finite, no negative determinant among its terms
YFM_GHD bool primal_ok(const Model& m, const State& s, int N, int nobs) {
  return finite(loglik_value(m, s, N, nobs));
}

// ∂(+loglik)/∂θ_c[d] from a tangent's sum; multiply by chain_factor for the unconstrained space
YFM_GHD double grad_value(const Model& m, const Tangent& t, int N, int nobs) {
  const int nterms = nobs - 2 > 0 ? nobs - 2 : 0;
  const double dconst = (seed_fs(t) * (double)(N - kM)) * m.rsig2;
  return -0.5 * gfma((double)nterms, dconst, t.acc);
}

// ∂ℓ_k/∂θ_c[d] of the step just taken, ℓ_k the term get_loss adds after column k: −½(dconst + last), with
// grad_value's dconst and the step's own (at a NaN column: the stale) tangent term; 0 for a step that is not
// accumulated (column 0).  Summed over a window's steps these are grad_value, up to the order of the sum.
YFM_GHD double score_value(const Model& m, const Tangent& t, int N, bool acc) {
  const double dconst = (seed_fs(t) * (double)(N - kM)) * m.rsig2;
  return acc ? -0.5 * (dconst + t.last) : 0.0;
}

}  // namespace tvlgrad
}  // namespace yfm
