// yfm_msed.hpp — the algebra of the static and score-driven λ Nelson–Siegel models (NS, SD-NS, RWSD-NS,
// SSD-NS, SRWSD-NS), as plain functions that compile for the device (yfm_msed.hip) and for the host
// (tests/msed_host_check.cpp).
//
// Restates, per candidate θ_b (paths relative to the reference root):
//   set_params!              src/models/msedriven/paramteroperations.jl:25-65, src/models/static/paramteroperations.jl:19-43
//   transformations          src/models/msedriven/mselambda.jl:17-34, msebasemodel.jl:77-90, static/staticbasemodel.jl:48-59
//   update_factor_loadings!  src/models/msedriven/mselambda.jl:63-76, src/models/static/staticlambda.jl:46-60
//   filter (one step)        src/models/filter.jl:52-110
//   get_β_OLS!               src/models/filter.jl:122-137
//   get_grad_gamma!          src/models/filter.jl:168-184 (the exact derivative, no dual numbers)
//   update_gamma_with_grad!  src/models/filter.jl:29-50
//
// One step needs the maturities only through sums, so a step is written as "accumulate the sufficient
// statistics of every maturity, then do 3×3 work":
//   OLS      G = Z'Z (G₁₁ = N and the five entries Σz₂, Σz₃, Σz₂², Σz₂z₃, Σz₃²) and Z'y (3);
//   score    g = ∂(−‖y − Z(γ)β‖²)/∂γ = 2 v'(∂Z/∂γ)β with v = y − Zβ, expanded so that it needs no second
//            pass over the maturities once β is known:
//                g = 2 [ β₂ (d₂'y − d₂'Zβ) + β₃ (d₃'y − d₃'Zβ) ],   ∂Z/∂γ = [0, d₂, d₃]
//            — the eight contractions d₂'[1 z₂ z₃], d₃'[1 z₂ z₃], d₂'y, d₃'y;
//   loss     ‖y − ŷ‖² against the previous step's prediction ŷ = Z(γ)β, formed per maturity: the loadings
//            a step starts from are the ones its predecessor predicted with, so the comparison of
//            get_loss (filter.jl:226-230) shares the first pass of the next step.
// The scaled kinds divide the score by the root of its own running mean square, which turns any rounding noise in
// a score that is exactly zero (N = 3: OLS interpolates and v = 0) into a step of ±A.  They therefore evaluate the
// score at the refined β: one more pass forms the residual v = y − Zβ with its rounding errors carried, Z'v and
// v'(∂Z/∂γ)β, one correction δβ = (Z'Z)⁻¹Z'v reuses the factorisation's branch, and g = 2[v'w − δβ'Z'w].
// The Cholesky pivots are formed without fused multiply-adds (contraction is off and no fma is written
// there): a pivot that is exactly zero as LAPACK forms it — N = 1, or λ = Inf — is exactly zero here, so
// the ridge retry of filter.jl:128-135 runs for the same candidates.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YFM_MHD __host__ __device__ __forceinline__
#else
#include <math.h>
#include <stddef.h>
#define YFM_MHD inline
#endif

namespace yfm {
namespace msed {

constexpr int kM = 3;
constexpr double kForget = 0.98;                  // forget_factor (mselambda.jl:15)
constexpr double kRidge = 1e-3;                   // filter.jl:132
constexpr double kEps = 2.220446049250313e-16;    // eps(Float64) (filter.jl:39)

// model_kind values (include/yfm.h) → the three switches of the step
YFM_MHD bool kind_known(int kind) { return kind == 3 || kind == 4 || kind == 5 || kind == 6 || kind == 8; }
YFM_MHD bool kind_static(int kind) { return kind == 3; }
YFM_MHD bool kind_has_b(int kind) { return kind == 4 || kind == 6; }
YFM_MHD bool kind_scaled(int kind) { return kind == 6 || kind == 8; }
YFM_MHD int kind_params(int kind) { return kind_static(kind) ? 13 : (kind_has_b(kind) ? 15 : 14); }

YFM_MHD double mfma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// transformations.jl:21-26, evaluated as written
YFM_MHD double from_R_to_11(double x) {
  const double y = exp(x);
  return 2.0 * y / (1.0 + y) - 1.0;
}

// What set_params! leaves in the model: the constants of the recursion and its initial state.
struct Model {
  double A, B, nu;   // A; B and ν = (1 − B)ω (0 and 0 where the model has no B, 0 everywhere for NS)
  double mu[kM];     // (I − Φ)δ
  double Phi[kM][kM];
  double beta0[kM];  // δ
  double gamma0;     // ω (NS: γ)
};

// The filter's state: β, γ and the score's second-moment average (reset by initialize_filter, filter.jl:19-26).
struct State {
  double beta[kM];
  double gamma;
  double ewma;
  double fpow;  // forget_factor^count
};

// θ_b → Model.  Layouts: NS [γ, δ(3), vec Φ(9)]; SD-NS / SSD-NS [A, B, ω, δ(3), vec Φ(9)]; RWSD-NS / SRWSD-NS the
// same without B.  vec Φ is column-major (reshape, paramteroperations.jl:56).  space 0: θ as compute_loss
// receives it (A → exp, B → 1/(1 + e^−x), diagonal of Φ → from_R_to_11); space 1: θ_c as set_params! does.
template <bool STATIC, bool HASB>
YFM_MHD void decode(const double* th, int space, Model& m) {
  const bool un = space == 0;
  int k = 0;
  m.A = 0.0;
  m.B = 0.0;
  if (!STATIC) {
    m.A = un ? exp(th[k]) : th[k];
    ++k;
    if (HASB) {
      m.B = un ? 1.0 / (1.0 + exp(-th[k])) : th[k];
      ++k;
    }
  }
  m.gamma0 = th[k++];
  for (int i = 0; i < kM; ++i) m.beta0[i] = th[k + i];
  k += kM;
  for (int c = 0; c < kM; ++c)
    for (int r = 0; r < kM; ++r) {
      const double x = th[k + c * kM + r];
      m.Phi[r][c] = (un && r == c) ? from_R_to_11(x) : x;
    }
  for (int r = 0; r < kM; ++r) {  // (I − Φ)δ, the matrix formed first (paramteroperations.jl:61)
    double s = 0.0;
    for (int c = 0; c < kM; ++c) s = s + ((r == c ? 1.0 : 0.0) - m.Phi[r][c]) * m.beta0[c];
    m.mu[r] = s;
  }
  m.nu = HASB ? (1.0 - m.B) * m.gamma0 : 0.0;
}

YFM_MHD void init_state(const Model& m, State& s) {
  for (int i = 0; i < kM; ++i) s.beta[i] = m.beta0[i];
  s.gamma = m.gamma0;
  s.ewma = 0.0;
  s.fpow = 1.0;
}

// λ = 0.01 + e^γ with what the loadings and their γ-derivative need of it
struct Lambda {
  double lam, rl, dl;  // λ, 1/λ, dλ/dγ = e^γ
};
YFM_MHD Lambda make_lambda(double gamma) {
  Lambda l;
  l.dl = exp(gamma);
  l.lam = 1e-2 + l.dl;
  l.rl = 1.0 / l.lam;
  return l;
}

// One maturity m (rm = 1/m): z = e^{−λm}, Z₂ = (1 − z)/(λm), Z₃ = Z₂ − z.  λ = Inf gives z = Z₂ = Z₃ = 0 exactly.
YFM_MHD void loadings(const Lambda& l, double m, double rm, double& z, double& z2, double& z3) {
  z = exp(-(l.lam * m));
  z2 = (1.0 - z) * (l.rl * rm);
  z3 = z2 - z;
}

// ∂Z₂/∂γ = (z − Z₂)·e^γ/λ and ∂Z₃/∂γ = ∂Z₂/∂γ + z·m·e^γ
YFM_MHD void dloadings(const Lambda& l, double m, double z, double z2, double& d2, double& d3) {
  d2 = (z - z2) * (l.dl * l.rl);
  d3 = mfma(z * m, l.dl, d2);
}

// Indices of the statistics.
enum : int { S2 = 0, S3, G22, G23, G33, Y1, Y2, Y3, NOLS };
enum : int { D21 = 0, D22, D23, D31, D32, D33, DY2, DY3, NSCORE };

YFM_MHD void accum_ols(double (&o)[NOLS], double z2, double z3, double y) {
  o[S2] += z2;
  o[S3] += z3;
  o[G22] = mfma(z2, z2, o[G22]);
  o[G23] = mfma(z2, z3, o[G23]);
  o[G33] = mfma(z3, z3, o[G33]);
  o[Y1] += y;
  o[Y2] = mfma(z2, y, o[Y2]);
  o[Y3] = mfma(z3, y, o[Y3]);
}

YFM_MHD void accum_score(double (&d)[NSCORE], double z2, double z3, double d2, double d3, double y) {
  d[D21] += d2;
  d[D22] = mfma(d2, z2, d[D22]);
  d[D23] = mfma(d2, z3, d[D23]);
  d[D31] += d3;
  d[D32] = mfma(d3, z2, d[D32]);
  d[D33] = mfma(d3, z3, d[D33]);
  d[DY2] = mfma(d2, y, d[DY2]);
  d[DY3] = mfma(d3, y, d[DY3]);
}

YFM_MHD double fitted(const double (&beta)[kM], double z2, double z3) { return mfma(beta[2], z3, mfma(beta[1], z2, beta[0])); }

// Cholesky of the symmetric 3×3 (lower entries g) and the solve G x = b.  A pivot that is not > 0 (NaN included:
// LAPACK's test) returns false and leaves x alone.
YFM_MHD bool chol3_solve(double g11, double g21, double g31, double g22, double g32, double g33, const double (&b)[kM],
                         double (&x)[kM]) {
  if (!(g11 > 0.0)) return false;
  const double r11 = 1.0 / sqrt(g11);
  const double l21 = g21 * r11, l31 = g31 * r11;
  const double a22 = g22 - l21 * l21;
  if (!(a22 > 0.0)) return false;
  const double r22 = 1.0 / sqrt(a22);
  const double l32 = (g32 - l31 * l21) * r22;
  const double a33 = g33 - (l31 * l31 + l32 * l32);
  if (!(a33 > 0.0)) return false;
  const double r33 = 1.0 / sqrt(a33);
  const double w0 = b[0] * r11;
  const double w1 = (b[1] - l21 * w0) * r22;
  const double w2 = (b[2] - l31 * w0 - l32 * w1) * r33;
  x[2] = w2 * r33;
  x[1] = (w1 - l32 * x[2]) * r22;
  x[0] = (w0 - l21 * x[1] - l31 * x[2]) * r11;
  return true;
}

// get_β_OLS! (filter.jl:122-137): β = (Z'Z)⁻¹Z'y by Cholesky; on failure once more with 1e-3 added to the
// diagonal (`ridged`); false where that fails too (the step then returns −Inf, filter.jl:62-67) — β is left alone.
YFM_MHD bool ols(const double (&o)[NOLS], double n, double (&beta)[kM], bool& ridged) {
  const double b[kM] = {o[Y1], o[Y2], o[Y3]};
  ridged = false;
  if (chol3_solve(n, o[S2], o[S3], o[G22], o[G23], o[G33], b, beta)) return true;
  ridged = true;
  return chol3_solve(n + kRidge, o[S2], o[S3], o[G22] + kRidge, o[G23], o[G33] + kRidge, b, beta);
}
YFM_MHD bool ols(const double (&o)[NOLS], double n, double (&beta)[kM]) {
  bool ridged;
  return ols(o, n, beta, ridged);
}

// s + e = a + b exactly
YFM_MHD void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// v = y − (β₁ + β₂z₂ + β₃z₃) with every rounding error of the evaluation carried: accurate relative to v itself,
// however much of y cancels
YFM_MHD double residual_carried(const double (&beta)[kM], double z2, double z3, double y) {
  const double p1 = beta[1] * z2, e1 = mfma(beta[1], z2, -p1);
  const double p2 = beta[2] * z3, e2 = mfma(beta[2], z3, -p2);
  double s1, f1, s2, f2, s3, f3;
  two_sum(y, -beta[0], s1, f1);
  two_sum(s1, -p1, s2, f2);
  two_sum(s2, -p2, s3, f3);
  return s3 + ((((f1 + f2) + f3) - e1) - e2);
}

// statistics of the refinement pass: Z'v (3) and v'w, w = (∂Z/∂γ)β
enum : int { R1 = 0, R2, R3, RH, NREFINE };

YFM_MHD void accum_refine(double (&r)[NREFINE], const double (&beta)[kM], double z2, double z3, double d2, double d3,
                          double y) {
  const double v = residual_carried(beta, z2, z3, y);
  const double w = mfma(d3, beta[2], d2 * beta[1]);
  r[R1] += v;
  r[R2] = mfma(z2, v, r[R2]);
  r[R3] = mfma(z3, v, r[R3]);
  r[RH] = mfma(v, w, r[RH]);
}

// g = 2 v'(∂Z/∂γ)β at the OLS β (filter.jl:168-184)
YFM_MHD double score(const double (&d)[NSCORE], const double (&beta)[kM]) {
  const double zb2 = mfma(d[D23], beta[2], mfma(d[D22], beta[1], d[D21] * beta[0]));  // d₂'Zβ
  const double zb3 = mfma(d[D33], beta[2], mfma(d[D32], beta[1], d[D31] * beta[0]));  // d₃'Zβ
  return 2.0 * mfma(beta[2], d[DY3] - zb3, beta[1] * (d[DY2] - zb2));
}

// The score at the refined β (the scaled kinds): δβ solves the system ols() solved (ridged or not) for the residual
// of its normal equations, Z'v − ridge·β, and g = 2 (v − Zδβ)'w = 2 [v'w − δβ'(Z'w)], Z'w from the contractions.
YFM_MHD double score_refined(const double (&o)[NOLS], double n, bool ridged, const double (&d)[NSCORE],
                             const double (&r)[NREFINE], const double (&beta)[kM]) {
  const double rd = ridged ? kRidge : 0.0;
  const double rhs[kM] = {r[R1] - rd * beta[0], r[R2] - rd * beta[1], r[R3] - rd * beta[2]};
  double db[kM] = {0.0, 0.0, 0.0};
  (void)chol3_solve(n + rd, o[S2], o[S3], o[G22] + rd, o[G23], o[G33] + rd, rhs, db);
  const double zw0 = mfma(d[D31], beta[2], d[D21] * beta[1]);
  const double zw1 = mfma(d[D32], beta[2], d[D22] * beta[1]);
  const double zw2 = mfma(d[D33], beta[2], d[D23] * beta[1]);
  return 2.0 * (r[RH] - mfma(db[2], zw2, mfma(db[1], zw1, db[0] * zw0)));
}

// update_gamma_with_grad! (filter.jl:29-50): γ ← γ + A·g, g first scaled by the bias-corrected root of its
// second-moment average where the model scales its score.
template <bool SCALED>
YFM_MHD void update_gamma(const Model& m, State& s, double g) {
  if (SCALED) {
    s.ewma = kForget * s.ewma + (1.0 - kForget) * (g * g);
    s.fpow = s.fpow * kForget;
    g = g / (sqrt(s.ewma / (1.0 - s.fpow)) + kEps);
  }
  s.gamma = s.gamma + g * m.A;
}

// The prediction half of a step (filter.jl:84-88, and the whole of a missing-data step, :53-59):
// γ ← ν + Bγ where the model has a B, β ← μ + Φβ.
template <bool HASB>
YFM_MHD void advance(const Model& m, State& s) {
  if (HASB) s.gamma = m.nu + m.B * s.gamma;
  double nb[kM];
  for (int r = 0; r < kM; ++r) {
    double a = 0.0;
    for (int c = 0; c < kM; ++c) a = mfma(m.Phi[r][c], s.beta[c], a);
    nb[r] = m.mu[r] + a;
  }
  for (int r = 0; r < kM; ++r) s.beta[r] = nb[r];
}

// ---- ∂loss/∂(δ, Φ) --------------------------------------------------------------------------------------------
// On a data column the step replaces β by an OLS fit and takes the score at that β (filter.jl:52-91), so γ, the
// loadings and β_post never see δ or Φ: they enter only the prediction β_pred = μ + Φβ_post = δ + Φ(β_post − δ).
// With v = y_{t+1} − Zβ_pred at the loadings Z the prediction used and s = Z'v,
//   loss = −Σ‖v‖²/(N·nobs),  ∂loss/∂δ = 2/(N·nobs)·Σ(I − Φ)'s,  ∂loss/∂Φ = 2/(N·nobs)·Σ s(β_post − δ)'
// and no tangent is carried through the recursion.  A missing first column makes step 1 prediction-only from
// β₀ = δ, so β_pred = δ: that step adds s to ∂/∂δ and nothing to ∂/∂Φ.  A missing column anywhere else inside the
// window is compared (filter.jl:226-234) and makes the loss −Inf, whose gradient is NaN.
constexpr int kGrad = kM + kM * kM;  // δ(3), then vec Φ column-major: the order of θ's last 12 rows

struct Grad {
  double d[kM];       // Σ ∂β_pred'/∂δ · s
  double F[kM][kM];   // Σ s (β_post − δ)', F[r][c] ↔ Φ[r][c]
};

YFM_MHD void grad_zero(Grad& g) {
  for (int r = 0; r < kM; ++r) {
    g.d[r] = 0.0;
    for (int c = 0; c < kM; ++c) g.F[r][c] = 0.0;
  }
}

// Z'v of one maturity into s (the sums the comparison pass adds to its statistics)
YFM_MHD void accum_zv(double (&s)[kM], double z2, double z3, double v) {
  s[0] += v;
  s[1] = mfma(z2, v, s[1]);
  s[2] = mfma(z3, v, s[2]);
}

// One compared prediction: s = Z'v; bpost the β the prediction advanced from (unused where pred_only, the
// prediction-only first step).  MODEL: anything with Φ and β₀ = δ (this file's Model, msedn::Model)
template <class MODEL>
YFM_MHD void grad_accum(const MODEL& m, bool pred_only, const double (&s)[kM], const double (&bpost)[kM], Grad& g) {
  if (pred_only) {
    for (int c = 0; c < kM; ++c) g.d[c] += s[c];
    return;
  }
  for (int c = 0; c < kM; ++c) {
    double a = 0.0;  // column c of (I − Φ) against s
    for (int r = 0; r < kM; ++r) a = mfma((r == c ? 1.0 : 0.0) - m.Phi[r][c], s[r], a);
    g.d[c] += a;
    const double db = bpost[c] - m.beta0[c];
    for (int r = 0; r < kM; ++r) g.F[r][c] = mfma(s[r], db, g.F[r][c]);
  }
}

// The 12 entries in the caller's space: scaled by 2/(N·nobs); space 0 multiplies the diagonal of Φ by
// d from_R_to_11/dx = 2y/(1 + y)², y = eˣ (δ and the off-diagonal entries are identity).  A candidate whose loss is
// −Inf (fail) gets NaN in all 12.
YFM_MHD void grad_finish(const Grad& g, const double* th, int P, int space, double n, int nobs, bool fail,
                         double (&out)[kGrad]) {
  const double sc = 2.0 / n / (double)nobs;
  for (int c = 0; c < kM; ++c) out[c] = g.d[c] * sc;
  for (int c = 0; c < kM; ++c)
    for (int r = 0; r < kM; ++r) {
      double v = g.F[r][c] * sc;
      if (space == 0 && r == c) {
        const double y = exp(th[P - kM * kM + c * kM + r]);
        v = v * (2.0 * y / ((1.0 + y) * (1.0 + y)));
      }
      out[kM + c * kM + r] = v;
    }
  if (fail)
    for (int k = 0; k < kGrad; ++k) out[k] = __builtin_nan("");
}

// One filter step on the column y (N yields) with every maturity visited in order — the form the host check
// runs; the kernel distributes the two accumulation loops over a lane group and runs the same 3×3 functions.
// Returns false where the reference's step returns −Inf (the state then stays as the failing call left it).
// bpost, where given, receives the β a data step predicts from (a prediction-only step leaves it alone).
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD bool filter_step(const Model& m, State& s, const double* mats, const double* y, int N,
                         double* bpost = nullptr) {
  if (y[0] != y[0]) {  // isnan(y[1]) (filter.jl:53, :95): prediction only
    advance<HASB>(m, s);
    return true;
  }
  Lambda l = make_lambda(s.gamma);
  double o[NOLS] = {0, 0, 0, 0, 0, 0, 0, 0}, d[NSCORE] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < N; ++i) {
    double z, z2, z3, d2, d3;
    loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
    accum_ols(o, z2, z3, y[i]);
    if (!STATIC) {
      dloadings(l, mats[i], z, z2, d2, d3);
      accum_score(d, z2, z3, d2, d3, y[i]);
    }
  }
  bool ridged;
  if (!ols(o, (double)N, s.beta, ridged)) return false;
  if (!STATIC) {
    double g;
    if (SCALED) {
      double r[NREFINE] = {0, 0, 0, 0};
      for (int i = 0; i < N; ++i) {
        double z, z2, z3, d2, d3;
        loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
        dloadings(l, mats[i], z, z2, d2, d3);
        accum_refine(r, s.beta, z2, z3, d2, d3, y[i]);
      }
      g = score_refined(o, (double)N, ridged, d, r, s.beta);
    } else {
      g = score(d, s.beta);
    }
    update_gamma<SCALED>(m, s, g);
    l = make_lambda(s.gamma);
    double o2[NOLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < N; ++i) {
      double z, z2, z3;
      loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
      accum_ols(o2, z2, z3, y[i]);
    }
    if (!ols(o2, (double)N, s.beta)) return false;
  }
  if (bpost)
    for (int r = 0; r < kM; ++r) bpost[r] = s.beta[r];
  advance<HASB>(m, s);
  return true;
}

// Z(γ)β of the current state for every maturity: the prediction filter returns (filter.jl:90, :109)
YFM_MHD void predict_column(const State& s, const double* mats, int N, double* pred) {
  const Lambda l = make_lambda(s.gamma);
  for (int i = 0; i < N; ++i) {
    double z, z2, z3;
    loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
    pred[i] = fitted(s.beta, z2, z3);
  }
}

// get_loss (filter.jl:209-243, K = 1) on the first nobs columns of Y (N×T column-major)
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double get_loss(const double* th, int space, const double* mats, const double* Y, int N, int nobs,
                        double* pred /* N scratch */) {
  Model m;
  State s;
  decode<STATIC, HASB>(th, space, m);
  init_state(m, s);
  double mse = 0.0;
  for (int t = 0; t + 1 < nobs; ++t) {
    const bool ok = filter_step<STATIC, HASB, SCALED>(m, s, mats, Y + (size_t)t * N, N);
    if (!ok) return -HUGE_VAL;
    predict_column(s, mats, N, pred);
    double vv = 0.0;
    for (int i = 0; i < N; ++i) {
      const double v = Y[(size_t)(t + 1) * N + i] - pred[i];
      vv = mfma(v, v, vv);
    }
    mse -= vv;
    if (!(fabs(mse) <= 1.79769313486231570815e308)) return -HUGE_VAL;  // isinf || isnan (filter.jl:232-234)
  }
  return mse / (double)N / (double)nobs;
}

// get_loss with ∂loss/∂(δ, Φ) in the caller's space (grad: kGrad entries).  The loss is get_loss's, sum for sum.
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double get_loss_grad(const double* th, int space, const double* mats, const double* Y, int N, int nobs,
                             double (&grad)[kGrad]) {
  Model m;
  State s;
  decode<STATIC, HASB>(th, space, m);
  init_state(m, s);
  Grad g;
  grad_zero(g);
  const int P = STATIC ? 13 : (HASB ? 15 : 14);
  double mse = 0.0;
  bool fail = false;
  for (int t = 0; t + 1 < nobs && !fail; ++t) {
    const double* y = Y + (size_t)t * N;
    const bool pred_only = y[0] != y[0];
    double bpost[kM] = {0.0, 0.0, 0.0};
    if (!filter_step<STATIC, HASB, SCALED>(m, s, mats, y, N, bpost)) {
      fail = true;
      break;
    }
    const Lambda l = make_lambda(s.gamma);
    double vv = 0.0, zv[kM] = {0.0, 0.0, 0.0};
    for (int i = 0; i < N; ++i) {
      double z, z2, z3;
      loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
      const double v = y[N + i] - fitted(s.beta, z2, z3);
      vv = mfma(v, v, vv);
      accum_zv(zv, z2, z3, v);
    }
    mse -= vv;
    fail = !(fabs(mse) <= 1.79769313486231570815e308);
    grad_accum(m, pred_only, zv, bpost, g);  // pred_only: t = 0 (a later missing column was compared: fail)
  }
  grad_finish(g, th, P, space, (double)N, nobs, fail, grad);
  return fail ? -HUGE_VAL : mse / (double)N / (double)nobs;
}

// ---- ∂loss/∂(A, B, ω; γ for NS): the full gradient ---------------------------------------------------------------
// The derivative of the function get_loss computes with respect to the leading parameters, by a forward tangent
// through the score recursion.  γ is a scalar, so per direction k the state tangent is the scalar
// γ̇ₖ and, for the scaled kinds, ėₖ of the score's second-moment average.  The directions are the constrained
// parameters — (A, B, ω), (A, ω) or (γ) — and space 0 multiplies the finished rows by dA/dx = A and dB/dx = B(1 − B).
//
// With Z = Z(γ), D = ∂Z/∂γ, E = ∂²Z/∂γ², G = Z'Z (ridged where ols ridged), v = y − Zβ and w = Dβ:
//   β' = ∂β/∂γ = G⁻¹(D'v − Z'w)                                   (ols_tangent)
//   g' = ∂g/∂γ = 2[−(w + Zβ')'w + v'Eβ + v'Dβ']                   (score_tangent)
// both from contractions over the maturities: the score's eight, and D'D (3), E'[1 z₂ z₃] (6), E'y (2) (accum_tan).
// The value path is untouched: the scaled kinds keep score_refined, and the tangent is the exact score's.
enum : int { DD22 = 0, DD23, DD33, E21, E22, E23, E31, E32, E33, EY2, EY3, NTAN };

// ∂²Z₂/∂γ² = (∂u/∂λ)q² + uq and ∂²Z₃/∂γ² = (∂u/∂λ − m²z)q² + (u + mz)q with q = e^γ, u = ∂Z₂/∂λ = (z − Z₂)/λ,
// ∂u/∂λ = (−mz − 2u)/λ
YFM_MHD void d2loadings(const Lambda& l, double m, double z, double z2, double& e2, double& e3) {
  const double u = (z - z2) * l.rl;
  const double mz = m * z;
  const double du = (-mz - 2.0 * u) * l.rl;
  e2 = mfma(du, l.dl, u) * l.dl;
  e3 = mfma(mfma(-m, mz, du), l.dl, u + mz) * l.dl;
}

YFM_MHD void accum_tan(double (&t)[NTAN], double z2, double z3, double d2, double d3, double e2, double e3, double y) {
  t[DD22] = mfma(d2, d2, t[DD22]);
  t[DD23] = mfma(d2, d3, t[DD23]);
  t[DD33] = mfma(d3, d3, t[DD33]);
  t[E21] += e2;
  t[E22] = mfma(e2, z2, t[E22]);
  t[E23] = mfma(e2, z3, t[E23]);
  t[E31] += e3;
  t[E32] = mfma(e3, z2, t[E32]);
  t[E33] = mfma(e3, z3, t[E33]);
  t[EY2] = mfma(e2, y, t[EY2]);
  t[EY3] = mfma(e3, y, t[EY3]);
}

// D'v of one maturity of the comparison: v = y_{t+1} − Zβ_pred at the loadings the prediction used
YFM_MHD void accum_dv(double (&s)[2], double d2, double d3, double v) {
  s[0] = mfma(d2, v, s[0]);
  s[1] = mfma(d3, v, s[1]);
}

// β' = G⁻¹(D'v − Z'Dβ) at the OLS β of the statistics o, d, in the system ols solved (ridged or not); dv receives
// d₂'v and d₃'v.  bp is left alone where the factorisation fails (ols failed on the same matrix: the step is −Inf).
YFM_MHD void ols_tangent(const double (&o)[NOLS], double n, bool ridged, const double (&d)[NSCORE],
                         const double (&beta)[kM], double (&bp)[kM], double (&dv)[2]) {
  const double zb2 = mfma(d[D23], beta[2], mfma(d[D22], beta[1], d[D21] * beta[0]));  // d₂'Zβ
  const double zb3 = mfma(d[D33], beta[2], mfma(d[D32], beta[1], d[D31] * beta[0]));  // d₃'Zβ
  dv[0] = d[DY2] - zb2;
  dv[1] = d[DY3] - zb3;
  const double zw0 = mfma(d[D31], beta[2], d[D21] * beta[1]);  // Z'w
  const double zw1 = mfma(d[D32], beta[2], d[D22] * beta[1]);
  const double zw2 = mfma(d[D33], beta[2], d[D23] * beta[1]);
  const double rhs[kM] = {-zw0, dv[0] - zw1, dv[1] - zw2};
  const double rd = ridged ? kRidge : 0.0;
  (void)chol3_solve(n + rd, o[S2], o[S3], o[G22] + rd, o[G23], o[G33] + rd, rhs, bp);
}

// g' = ∂g/∂γ of the score g = 2v'Dβ at the OLS β (β' and D'v from ols_tangent)
YFM_MHD double score_tangent(const double (&d)[NSCORE], const double (&t)[NTAN], const double (&beta)[kM],
                             const double (&bp)[kM], const double (&dv)[2]) {
  const double ww = mfma(beta[2] * beta[2], t[DD33], mfma(2.0 * beta[1] * beta[2], t[DD23], beta[1] * beta[1] * t[DD22]));
  const double zw0 = mfma(d[D31], beta[2], d[D21] * beta[1]);
  const double zw1 = mfma(d[D32], beta[2], d[D22] * beta[1]);
  const double zw2 = mfma(d[D33], beta[2], d[D23] * beta[1]);
  const double bzw = mfma(bp[2], zw2, mfma(bp[1], zw1, bp[0] * zw0));                            // β''Z'w
  const double ev2 = t[EY2] - mfma(t[E23], beta[2], mfma(t[E22], beta[1], t[E21] * beta[0]));  // e₂'v
  const double ev3 = t[EY3] - mfma(t[E33], beta[2], mfma(t[E32], beta[1], t[E31] * beta[0]));  // e₃'v
  const double veb = mfma(beta[2], ev3, beta[1] * ev2);                                          // v'Eβ
  const double vdb = mfma(bp[2], dv[1], bp[1] * dv[0]);                                          // v'Dβ'
  return 2.0 * ((veb + vdb) - (ww + bzw));
}

// The tangents of one candidate.  K directions: (A, B, ω) K = 3, (A, ω) K = 2, (γ) K = 1 — A is direction 0, B
// direction 1 where there is one, ω (γ) the last.
template <int K>
struct Tangent {
  double gd[K];     // γ̇ₖ of the state's γ
  double ed[K];     // ėₖ of the score's second-moment average (scaled kinds)
  double gp[K];     // γ̇⁺ₖ of the γ the last data step's second OLS ran at
  double pb[kM];    // Φβ'(γ⁺) of that OLS: ∂β_pred/∂pₖ = pb·γ̇⁺ₖ (zero after a prediction-only step)
  double lead[K];   // Σ over the compared columns of ½ ∂(−‖v‖²)/∂pₖ
};

template <bool STATIC, bool HASB>
constexpr int lead_count() {
  return STATIC ? 1 : (HASB ? 3 : 2);
}

// γ₀ = ω (set_params!): γ̇ is 1 in the ω direction (γ for NS) and 0 in the others
template <int K>
YFM_MHD void tangent_init(Tangent<K>& tn) {
  for (int k = 0; k < K; ++k) {
    tn.gd[k] = k == K - 1 ? 1.0 : 0.0;
    tn.ed[k] = 0.0;
    tn.gp[k] = 0.0;
    tn.lead[k] = 0.0;
  }
  for (int r = 0; r < kM; ++r) tn.pb[r] = 0.0;
}

// The tangent of update_gamma, called after it (s holds e⁺ and fⁿ) with the score g it was given and g' = ∂g/∂γ:
//   ġₖ = g'γ̇ₖ;  scaled: ė⁺ₖ = fėₖ + 2(1 − f)gġₖ, c = 1 − fⁿ, r = √(e⁺/c), s = r + ε, ṡₖ = ė⁺ₖ/(2cr),
//   g̃ = g/s, g̃˙ₖ = ġₖ/s − gṡₖ/s²;  γ̇⁺ₖ = γ̇ₖ + Ȧₖg̃ + Ag̃˙ₖ.   r = 0 (a score that is exactly zero) gives NaN.
template <bool SCALED, int K>
YFM_MHD void update_gamma_tangent(const Model& m, const State& s, double g, double gprime, Tangent<K>& tn) {
  double rs = 1.0, c2r = 1.0;
  if (SCALED) {
    const double c = 1.0 - s.fpow;
    const double r = sqrt(s.ewma / c);
    rs = 1.0 / (r + kEps);
    c2r = 2.0 * c * r;
  }
  const double gs = SCALED ? g * rs : g;
  for (int k = 0; k < K; ++k) {
    double gk = gprime * tn.gd[k];
    if (SCALED) {
      tn.ed[k] = kForget * tn.ed[k] + 2.0 * (1.0 - kForget) * (g * gk);
      const double sd = tn.ed[k] / c2r;
      gk = gk * rs - g * sd * (rs * rs);
    }
    tn.gd[k] = tn.gd[k] + (k == 0 ? gs : 0.0) + m.A * gk;
  }
}

// The end of a data step: β_pred = μ + Φβ₂ with β̇₂ₖ = β'(γ⁺)γ̇⁺ₖ, then the tangent of advance's γ ← ν + Bγ⁺ (gamma: γ⁺,
// the state's γ before advance): γ̇ₖ ← ν̇ₖ + Ḃₖγ⁺ + Bγ̇⁺ₖ with ν = (1 − B)ω, so ν̇ = −ω for B and 1 − B for ω.
template <bool HASB, int K>
YFM_MHD void advance_tangent(const Model& m, double gamma, const double (&bp)[kM], Tangent<K>& tn) {
  for (int r = 0; r < kM; ++r) {
    double a = 0.0;
    for (int c = 0; c < kM; ++c) a = mfma(m.Phi[r][c], bp[c], a);
    tn.pb[r] = a;
  }
  for (int k = 0; k < K; ++k) {
    tn.gp[k] = tn.gd[k];
    if (HASB) {
      const double off = k == 1 ? gamma - m.gamma0 : (k == K - 1 ? 1.0 - m.B : 0.0);
      tn.gd[k] = mfma(m.B, tn.gd[k], off);
    }
  }
}

// A prediction-only step (a missing first column): γ₁ = ν + Bγ₀ with its tangent, and no β̇
template <bool HASB, int K>
YFM_MHD void advance_tangent_pred_only(const Model& m, double gamma, Tangent<K>& tn) {
  const double zero[kM] = {0.0, 0.0, 0.0};
  advance_tangent<HASB>(m, gamma, zero, tn);
}

// One compared column: v = y_{t+1} − Z(γ)β_pred, zv = Z'v, dv = [d₂'v, d₃'v] at the state's γ, bpred the state's β:
//   ½ ∂(−‖v‖²)/∂pₖ = (v'Dβ_pred)γ̇ₖ + (v'ZΦβ')γ̇⁺ₖ
template <int K>
YFM_MHD void lead_accum(const double (&zv)[kM], const double (&dv)[2], const double (&bpred)[kM], Tangent<K>& tn) {
  const double c1 = mfma(bpred[2], dv[1], bpred[1] * dv[0]);
  const double c2 = mfma(zv[2], tn.pb[2], mfma(zv[1], tn.pb[1], zv[0] * tn.pb[0]));
  for (int k = 0; k < K; ++k) tn.lead[k] = mfma(c2, tn.gp[k], mfma(c1, tn.gd[k], tn.lead[k]));
}

// All P rows in the caller's space: the K leading rows scaled by 2/(N·nobs) and by dA/dx = A, dB/dx = B(1 − B) in
// space 0, then grad_finish's 12.  NaN in every row where the loss is −Inf (fail) and where a tangent or a leading
// accumulator is not finite; returns true in the second case alone (the gradient of a finite loss is unavailable).
template <bool STATIC, bool HASB, int K>
YFM_MHD bool fullgrad_finish(const Model& m, const Tangent<K>& tn, const Grad& g, const double* th, int P, int space,
                             double n, int nobs, bool fail, double* out /* P */) {
  const double sc = 2.0 / n / (double)nobs;
  const double big = 1.79769313486231570815e308;
  bool bad = false;
  for (int k = 0; k < K; ++k) {
    bad = bad || !(fabs(tn.gd[k]) <= big) || !(fabs(tn.ed[k]) <= big) || !(fabs(tn.gp[k]) <= big) ||
          !(fabs(tn.lead[k]) <= big);
    double v = tn.lead[k] * sc;
    if (space == 0 && !STATIC && k == 0) v = v * m.A;
    if (space == 0 && HASB && k == 1) v = v * (m.B * (1.0 - m.B));
    out[k] = v;
  }
  for (int r = 0; r < kM; ++r) bad = bad || !(fabs(tn.pb[r]) <= big);
  double tail[kGrad];
  grad_finish(g, th, P, space, n, nobs, fail, tail);
  for (int k = 0; k < kGrad; ++k) out[K + k] = tail[k];
  if (fail || bad)
    for (int k = 0; k < P; ++k) out[k] = __builtin_nan("");
  return bad && !fail;
}

// filter_step with the tangents carried: the same value path, sum for sum, with the score statistics formed for NS too
// (β' needs them) and the second pass's as well.
template <bool STATIC, bool HASB, bool SCALED, int K>
YFM_MHD bool filter_step_tangent(const Model& m, State& s, Tangent<K>& tn, const double* mats, const double* y, int N,
                                 double* bpost) {
  if (y[0] != y[0]) {
    advance_tangent_pred_only<HASB>(m, s.gamma, tn);
    advance<HASB>(m, s);
    return true;
  }
  Lambda l = make_lambda(s.gamma);
  double o[NOLS] = {0, 0, 0, 0, 0, 0, 0, 0}, d[NSCORE] = {0, 0, 0, 0, 0, 0, 0, 0};
  double tt[NTAN] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < N; ++i) {
    double z, z2, z3, d2, d3;
    loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
    accum_ols(o, z2, z3, y[i]);
    dloadings(l, mats[i], z, z2, d2, d3);
    accum_score(d, z2, z3, d2, d3, y[i]);
    if (!STATIC) {
      double e2, e3;
      d2loadings(l, mats[i], z, z2, e2, e3);
      accum_tan(tt, z2, z3, d2, d3, e2, e3, y[i]);
    }
  }
  bool ridged;
  if (!ols(o, (double)N, s.beta, ridged)) return false;
  double bp[kM] = {0.0, 0.0, 0.0}, dv[2];
  ols_tangent(o, (double)N, ridged, d, s.beta, bp, dv);
  if (!STATIC) {
    double g;
    if (SCALED) {
      double r[NREFINE] = {0, 0, 0, 0};
      for (int i = 0; i < N; ++i) {
        double z, z2, z3, d2, d3;
        loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
        dloadings(l, mats[i], z, z2, d2, d3);
        accum_refine(r, s.beta, z2, z3, d2, d3, y[i]);
      }
      g = score_refined(o, (double)N, ridged, d, r, s.beta);
    } else {
      g = score(d, s.beta);
    }
    const double gprime = score_tangent(d, tt, s.beta, bp, dv);
    update_gamma<SCALED>(m, s, g);
    update_gamma_tangent<SCALED>(m, s, g, gprime, tn);
    l = make_lambda(s.gamma);
    double o2[NOLS] = {0, 0, 0, 0, 0, 0, 0, 0}, dd[NSCORE] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < N; ++i) {
      double z, z2, z3, d2, d3;
      loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
      accum_ols(o2, z2, z3, y[i]);
      dloadings(l, mats[i], z, z2, d2, d3);
      accum_score(dd, z2, z3, d2, d3, y[i]);
    }
    if (!ols(o2, (double)N, s.beta, ridged)) return false;
    ols_tangent(o2, (double)N, ridged, dd, s.beta, bp, dv);
  }
  for (int r = 0; r < kM; ++r) bpost[r] = s.beta[r];
  advance_tangent<HASB>(m, s.gamma, bp, tn);
  advance<HASB>(m, s);
  return true;
}

// get_loss with all P derivatives in the caller's space (grad: P entries): the loss is get_loss's and the last 12
// rows are get_loss_grad's, sum for sum.  unavailable, where given, receives fullgrad_finish's return.
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double get_loss_fullgrad(const double* th, int space, const double* mats, const double* Y, int N, int nobs,
                                 double* grad, bool* unavailable = nullptr) {
  constexpr int K = lead_count<STATIC, HASB>();
  Model m;
  State s;
  decode<STATIC, HASB>(th, space, m);
  init_state(m, s);
  Grad g;
  grad_zero(g);
  Tangent<K> tn;
  tangent_init(tn);
  const int P = K + kGrad;
  double mse = 0.0;
  bool fail = false;
  for (int t = 0; t + 1 < nobs && !fail; ++t) {
    const double* y = Y + (size_t)t * N;
    const bool pred_only = y[0] != y[0];
    double bpost[kM] = {0.0, 0.0, 0.0};
    if (!filter_step_tangent<STATIC, HASB, SCALED>(m, s, tn, mats, y, N, bpost)) {
      fail = true;
      break;
    }
    const Lambda l = make_lambda(s.gamma);
    double vv = 0.0, zv[kM] = {0.0, 0.0, 0.0}, dv[2] = {0.0, 0.0};
    for (int i = 0; i < N; ++i) {
      double z, z2, z3, d2, d3;
      loadings(l, mats[i], 1.0 / mats[i], z, z2, z3);
      const double v = y[N + i] - fitted(s.beta, z2, z3);
      vv = mfma(v, v, vv);
      accum_zv(zv, z2, z3, v);
      dloadings(l, mats[i], z, z2, d2, d3);
      accum_dv(dv, d2, d3, v);
    }
    mse -= vv;
    fail = !(fabs(mse) <= 1.79769313486231570815e308);
    grad_accum(m, pred_only, zv, bpost, g);
    lead_accum(zv, dv, s.beta, tn);
  }
  const bool un = fullgrad_finish<STATIC, HASB>(m, tn, g, th, P, space, (double)N, nobs, fail, grad);
  if (unavailable) *unavailable = un;
  return fail ? -HUGE_VAL : mse / (double)N / (double)nobs;
}

}  // namespace msed
}  // namespace yfm
