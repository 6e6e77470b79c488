// yfm_msedn.hpp — the algebra of the neural Nelson–Siegel models (NNS, NNS-Anchored and the score-driven
// 1/2/3[S][RW]SD-NNS[-Anchored] kinds), as plain functions that compile for the device (yfm_msedn.hip) and for the
// host (tests/msedn_host_check.cpp, tests/msedn_grad_host_check.cpp).
//
// Restates, per candidate θ_b (paths relative to the reference root):
//   set_params!              src/models/msedriven/paramteroperations.jl:25-65, src/models/static/paramteroperations.jl:19-43
//   duplicator, transforms   src/models/msedriven/mseneural.jl:24-57, msebasemodel.jl:77-90
//   networks                 src/models/msedriven/mseneural.jl:120-163, src/models/static/staticneural.jl:81-110
//   loading transforms       src/utils/neural_network_transform.jl
//   filter (one step)        src/models/filter.jl:52-110, update_gamma_with_grad! :29-50, get_grad_gamma! :168-184
//
// γ ∈ ℝ¹⁸: γ[0..8] drives Z₂ and γ[9..17] drives Z₃, each block [w₁(3), b(3), w₂(3)] of a 1→3→1 tanh network
// without output bias, raw(m) = Σₕ w₂ₕ·tanh(w₁ₕ·m + bₕ).  tanh is the mathematical function.
//
// The transforms need group-wide scalars before any maturity has its loadings (Scal): the anchor raws, and the
// normaliser of Z₃ from Q = Σqᵢ².  `prepare` forms them whenever γ changes, with — for the kinds that take a score —
// the data-free part of the score (Aux): the score is linear in S = Σᵢ a³ᵢqᵢ, whose coefficient vector needs no data.
// With them a pass over the maturities is one evaluation per maturity, and the score is two phases: the OLS
// statistics, β, then the sums with v formed per maturity.
//
// The 3×3 work (Cholesky, ridge retry, the OLS statistics) is yfm_msed.hpp's.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#include "yfm_msed.hpp"

namespace yfm {
namespace msedn {

using msed::kM;
using msed::mfma;
using msed::NOLS;

constexpr int kG = 18;     // length of γ
constexpr int kBlk = 9;    // one network's block
constexpr int kH = 3;      // hidden units
constexpr double kForget = 0.9;    // forget_factor (mseneural.jl:24)
constexpr double kScale = 0.9610;  // neural_network_transform.jl:27, :79
constexpr double kTiny = 1e-7;
constexpr int kMinN = 4;   // below it the transforms' anchor slots alias

// model_kind values (include/yfm.h): 16 NNS, 17 NNS-Anchored, 32 | dyn | RW<<2 | SCALED<<3 | ANCHORED<<4
YFM_MHD bool kind_static(int kind) { return kind == 16 || kind == 17; }
YFM_MHD bool kind_known(int kind) { return kind_static(kind) || (kind >= 32 && kind < 64 && (kind & 3) != 3); }
YFM_MHD bool kind_anchored(int kind) { return kind_static(kind) ? kind == 17 : ((kind >> 4) & 1) != 0; }
YFM_MHD bool kind_has_b(int kind) { return !kind_static(kind) && ((kind >> 2) & 1) == 0; }
YFM_MHD bool kind_scaled(int kind) { return !kind_static(kind) && ((kind >> 3) & 1) != 0; }
YFM_MHD int kind_dyn(int kind) { return kind & 3; }  // 0 scalar, 1 block_diag, 2 diag
YFM_MHD int dyn_unique(int dyn) { return dyn == 0 ? 2 : (dyn == 1 ? 6 : kG); }
YFM_MHD int kind_params(int kind) {
  const int tail = kG + kM + kM * kM;
  return kind_static(kind) ? tail : dyn_unique(kind_dyn(kind)) * (kind_has_b(kind) ? 2 : 1) + tail;
}
// the duplicator (mseneural.jl:33-48): the unique value component k of γ takes
YFM_MHD int dup(int dyn, int k) { return dyn == 0 ? k / kBlk : (dyn == 1 ? k / kH : k); }

// What set_params! leaves in the model besides the 18-vectors A, B, ν and γ₀ (which the caller places).
struct Model {
  bool anchored;
  double mu[kM];     // (I − Φ)δ
  double Phi[kM][kM];
  double beta0[kM];  // δ
};

// θ_b → Model, A, B, ν (18 each; B = ν = 0 where the model has no B, A = 0 for the static kinds) and γ₀ = ω.
// Layouts: static [γ(18), δ(3), vec Φ(9)]; score-driven [A_unique, B_unique (absent for random walk), ω(18), δ, vec Φ].
// space 0: A → exp, B → 1/(1 + e^−x), diagonal of Φ → from_R_to_11; space 1: θ_c as set_params! reads it.
YFM_MHD void decode(const double* th, int space, int kind, Model& m, double* A, double* B, double* nu, double* gamma0) {
  const bool un = space == 0;
  const bool st = kind_static(kind), hb = kind_has_b(kind);
  const int dyn = kind_dyn(kind), nuq = st ? 0 : dyn_unique(dyn);
  m.anchored = kind_anchored(kind);
  int k = st ? 0 : nuq * (hb ? 2 : 1);
  for (int c = 0; c < kG; ++c) {
    gamma0[c] = th[k + c];
    double a = 0.0, b = 0.0;
    if (!st) {
      const int u = dup(dyn, c);
      a = un ? exp(th[u]) : th[u];
      if (hb) b = un ? 1.0 / (1.0 + exp(-th[nuq + u])) : th[nuq + u];
    }
    A[c] = a;
    B[c] = b;
    nu[c] = hb ? (1.0 - b) * gamma0[c] : 0.0;
  }
  k += kG;
  for (int i = 0; i < kM; ++i) m.beta0[i] = th[k + i];
  k += kM;
  for (int c = 0; c < kM; ++c)
    for (int r = 0; r < kM; ++r) {
      const double x = th[k + c * kM + r];
      m.Phi[r][c] = (un && r == c) ? msed::from_R_to_11(x) : x;
    }
  for (int r = 0; r < kM; ++r) {
    double s = 0.0;
    for (int c = 0; c < kM; ++c) s = s + ((r == c ? 1.0 : 0.0) - m.Phi[r][c]) * m.beta0[c];
    m.mu[r] = s;
  }
}

// tanh of the three hidden units at one maturity
struct Tau {
  double t[kH];
};

// raw(m) of one network block g = [w₁, b, w₂]
YFM_MHD double net_raw(const double* g, double m, Tau& tau) {
  double r = 0.0;
  for (int h = 0; h < kH; ++h) {
    tau.t[h] = tanh(mfma(g[h], m, g[kH + h]));
    r = mfma(g[2 * kH + h], tau.t[h], r);
  }
  return r;
}

// acc += c·∂raw(m)/∂g: w₁ₕ: c·w₂ₕ(1 − τₕ²)m, bₕ: the same without m, w₂ₕ: c·τₕ
YFM_MHD void accum_net(double* acc, const double* g, const Tau& tau, double c, double m) {
  for (int h = 0; h < kH; ++h) {
    const double w = (c * g[2 * kH + h]) * (1.0 - tau.t[h] * tau.t[h]);
    acc[h] = mfma(w, m, acc[h]);
    acc[kH + h] += w;
    acc[2 * kH + h] = mfma(c, tau.t[h], acc[2 * kH + h]);
  }
}

// The group-wide scalars of the transforms (neural_network_transform.jl).  The anchored kinds run the same
// per-maturity text with l2 = 0, iu = 1, s3 = c3 = 0, which leaves raw exactly.
struct Scal {
  double l2, iu;   // Z₂: raw_{n−1} and 1/(raw₁ − raw_{n−1} + 1e-7)
  double s3, c3;   // Z₃: slope and intercept through (m₁, raw₁), (mₙ, rawₙ)
  double sc, kap;  // Z₃ = q·sc; ∂sc/∂qᵢ = −kap·qᵢ
};
// The maturities the anchors sit at: m₁, m_{n−1}, mₙ
struct Ends {
  double m0, mP, mN;
};

YFM_MHD void anchors(const double* gam, bool anchored, const Ends& e, Scal& s) {
  s.l2 = 0.0;
  s.iu = 1.0;
  s.s3 = 0.0;
  s.c3 = 0.0;
  if (anchored) return;
  Tau t;
  const double a2 = net_raw(gam, e.m0, t);
  s.l2 = net_raw(gam, e.mP, t);
  s.iu = 1.0 / (a2 - s.l2 + kTiny);
  const double a3 = net_raw(gam + kBlk, e.m0, t), n3 = net_raw(gam + kBlk, e.mN, t);
  s.s3 = (n3 - a3) / (e.mN - e.m0);
  s.c3 = a3 - s.s3 * e.m0;
}

YFM_MHD bool in2(int i, int N) { return i >= 1 && i <= N - 3; }  // Z₂'s transformed maturities (0-based)
YFM_MHD bool in3(int i, int N) { return i >= 1 && i <= N - 2; }  // Z₃'s

// rᵢ (as written: raw − (s·m − c)) and qᵢ = rᵢ²
YFM_MHD double resid3(const double* gam, const Scal& s, double m, Tau& tau, double& r) {
  const double raw = net_raw(gam + kBlk, m, tau);
  r = raw - (s.s3 * m - s.c3);
  return r * r;
}

YFM_MHD void finish_scale(double Q, bool anchored, Scal& s) {
  const double rq = sqrt(Q);
  if (anchored) {
    s.sc = kScale / rq + kTiny;
    s.kap = kScale / (Q * rq);
  } else {
    s.sc = 1.0 / (rq / kScale + kTiny);
    s.kap = (s.sc * s.sc) / (kScale * rq);
  }
}

// What a maturity's evaluation leaves for the score
struct Point {
  Tau t2, t3;
  double t, r, q;  // Z₂ = t², Z₃ = q·sc
};

YFM_MHD void loadings(const double* gam, const Scal& s, int i, int N, double m, double& z2, double& z3, Point& p) {
  p.t = (net_raw(gam, m, p.t2) - s.l2) * s.iu;
  p.q = resid3(gam, s, m, p.t3, p.r);
  z2 = i == 0 ? 1.0 : (in2(i, N) ? p.t * p.t : 0.0);
  z3 = in3(i, N) ? p.q * s.sc : 0.0;
}

// The data-free part of the score, summed with Q: Σ 2rᵢqᵢ·∂rawᵢ/∂γ₃ (9), Σ 2rᵢqᵢ, Σ mᵢ·2rᵢqᵢ
enum : int { AQ = 0, AH = 1, AH0 = AH + kBlk, AH1, NAUX };

template <bool WITH_H>
YFM_MHD void accum_aux(double* a, const double* gam, const Scal& s, int i, int N, double m) {
  if (!in3(i, N)) return;
  Tau tau;
  double r;
  const double q = resid3(gam, s, m, tau, r);
  a[AQ] = mfma(q, q, a[AQ]);
  if (WITH_H) {
    const double c = 2.0 * r * q;
    accum_net(a + AH, gam + kBlk, tau, c, m);
    a[AH0] += c;
    a[AH1] = mfma(m, c, a[AH1]);
  }
}

// The sums of the score pass: the two networks' Σ cᵢ·∂rawᵢ/∂γ, the anchor sums and S = Σ a³ᵢqᵢ
enum : int { C1 = 0, CU0 = kBlk, CU1, C2, CR0 = C2 + kBlk, CR1, CS, NSCORE };

YFM_MHD void accum_score(double* c, const double* gam, const Scal& s, const double (&beta)[kM], int i, int N, double m,
                         double y) {
  double z2, z3;
  Point p;
  loadings(gam, s, i, N, m, z2, z3, p);
  const double v = y - msed::fitted(beta, z2, z3);
  if (in2(i, N)) {
    const double d = 2.0 * ((2.0 * beta[1]) * v) * p.t;
    accum_net(c + C1, gam, p.t2, d * s.iu, m);
    c[CU0] = mfma(d, p.t, c[CU0]);
    c[CU1] = mfma(d, p.t - 1.0, c[CU1]);
  }
  if (in3(i, N)) {
    const double a3 = (2.0 * beta[2]) * v;
    const double cr = (2.0 * p.r) * (a3 * s.sc);
    accum_net(c + C2, gam + kBlk, p.t3, cr, m);
    c[CR0] += cr;
    c[CR1] = mfma(m, cr, c[CR1]);
    c[CS] = mfma(a3, p.q, c[CS]);
  }
}

// g = ∂(−‖y − Z(γ)β‖²)/∂γ from the sums: the anchor maturities collect what the transforms route through them
YFM_MHD void finish_score(const double* c, const double* aux, const double* gam, const Scal& s, bool anchored,
                          const Ends& e, double* g) {
  const double sk = c[CS] * s.kap;
  for (int k = 0; k < kBlk; ++k) {
    g[k] = c[C1 + k];
    g[kBlk + k] = c[C2 + k] - sk * aux[AH + k];
  }
  if (anchored) return;
  Tau t;
  (void)net_raw(gam, e.mP, t);
  accum_net(g, gam, t, c[CU1] * s.iu, e.mP);
  (void)net_raw(gam, e.m0, t);
  accum_net(g, gam, t, -(c[CU0] * s.iu), e.m0);
  const double r0 = c[CR0] - sk * aux[AH0], r1 = c[CR1] - sk * aux[AH1];
  const double cn = (-r1 - e.m0 * r0) / (e.mN - e.m0);
  (void)net_raw(gam + kBlk, e.m0, t);
  accum_net(g + kBlk, gam + kBlk, t, r0 - cn, e.m0);
  (void)net_raw(gam + kBlk, e.mN, t);
  accum_net(g + kBlk, gam + kBlk, t, cn, e.mN);
}

// The filter's state with the scalars of the loadings at γ.  The score's second-moment average (18, reset by
// initialize_filter, filter.jl:19-26) is the caller's to place: the kernel keeps it beside A, B and ν.
struct State {
  double beta[kM];
  double gamma[kG];
  double fpow;  // forget_factor^count
  Scal sc;
  double aux[NAUX];
};

// update_gamma_with_grad! (filter.jl:29-50), per component
template <bool SCALED>
YFM_MHD void update_gamma(const double* A, double* ewma, State& s, double* g) {
  double den = 1.0;
  if (SCALED) {
    s.fpow = s.fpow * kForget;
    den = 1.0 - s.fpow;
  }
  for (int k = 0; k < kG; ++k) {
    double gk = g[k];
    if (SCALED) {
      const double ew = kForget * ewma[k] + (1.0 - kForget) * (gk * gk);
      ewma[k] = ew;
      gk = gk / (sqrt(ew / den) + msed::kEps);
    }
    s.gamma[k] = s.gamma[k] + gk * A[k];
  }
}

// γ ← ν + B∘γ where the model has a B (the caller then prepares the loadings again), β ← μ + Φβ
template <bool HASB>
YFM_MHD void advance(const Model& m, const double* B, const double* nu, State& s) {
  if (HASB)
    for (int k = 0; k < kG; ++k) s.gamma[k] = nu[k] + B[k] * s.gamma[k];
  double nb[kM];
  for (int r = 0; r < kM; ++r) {
    double a = 0.0;
    for (int c = 0; c < kM; ++c) a = mfma(m.Phi[r][c], s.beta[c], a);
    nb[r] = m.mu[r] + a;
  }
  for (int r = 0; r < kM; ++r) s.beta[r] = nb[r];
}

// ---- the sequential form (the host check): every maturity visited in order ------------------------------------
YFM_MHD Ends ends_of(const double* mats, int N) {
  Ends e;
  e.m0 = mats[0];
  e.mP = mats[N - 2];
  e.mN = mats[N - 1];
  return e;
}

template <bool WITH_H>
YFM_MHD void prepare(const Model& m, State& s, const double* mats, int N) {
  anchors(s.gamma, m.anchored, ends_of(mats, N), s.sc);
  for (int k = 0; k < NAUX; ++k) s.aux[k] = 0.0;
  for (int i = 0; i < N; ++i) accum_aux<WITH_H>(s.aux, s.gamma, s.sc, i, N, mats[i]);
  finish_scale(s.aux[AQ], m.anchored, s.sc);
}

template <bool STATIC>
YFM_MHD void init_state(const Model& m, const double* gamma0, State& s, double* ewma, const double* mats, int N) {
  for (int i = 0; i < kM; ++i) s.beta[i] = m.beta0[i];
  for (int k = 0; k < kG; ++k) {
    s.gamma[k] = gamma0[k];
    ewma[k] = 0.0;
  }
  s.fpow = 1.0;
  prepare<!STATIC>(m, s, mats, N);
}

YFM_MHD void ols_pass(const State& s, const double* mats, const double* y, int N, double (&o)[NOLS]) {
  for (int k = 0; k < NOLS; ++k) o[k] = 0.0;
  for (int i = 0; i < N; ++i) {
    double z2, z3;
    Point p;
    loadings(s.gamma, s.sc, i, N, mats[i], z2, z3, p);
    msed::accum_ols(o, z2, z3, y[i]);
  }
}

// One filter step (filter.jl:52-110); false where the reference's step returns −Inf.  bpost, where given, receives
// the β a data step predicts from (a prediction-only step leaves it alone).
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD bool filter_step(const Model& m, const double* A, const double* B, const double* nu, double* ewma, State& s,
                         const double* mats, const double* y, int N, double* bpost = nullptr) {
  if (y[0] != y[0]) {  // isnan(y[1]): prediction only
    advance<HASB>(m, B, nu, s);
    if (HASB) prepare<true>(m, s, mats, N);
    return true;
  }
  double o[NOLS];
  ols_pass(s, mats, y, N, o);
  if (!msed::ols(o, (double)N, s.beta)) return false;
  if (!STATIC) {
    double c[NSCORE], g[kG];
    for (int k = 0; k < NSCORE; ++k) c[k] = 0.0;
    for (int i = 0; i < N; ++i) accum_score(c, s.gamma, s.sc, s.beta, i, N, mats[i], y[i]);
    finish_score(c, s.aux, s.gamma, s.sc, m.anchored, ends_of(mats, N), g);
    update_gamma<SCALED>(A, ewma, s, g);
    prepare<!HASB>(m, s, mats, N);
    ols_pass(s, mats, y, N, o);
    if (!msed::ols(o, (double)N, s.beta)) return false;
  }
  if (bpost)
    for (int r = 0; r < kM; ++r) bpost[r] = s.beta[r];
  advance<HASB>(m, B, nu, s);
  if (HASB) prepare<true>(m, s, mats, N);
  return true;
}

// get_loss (filter.jl:209-243, K = 1) on the first nobs columns of Y (N×T column-major)
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double get_loss(const double* th, int space, int kind, const double* mats, const double* Y, int N, int nobs) {
  Model m;
  State s;
  double A[kG], B[kG], nu[kG], g0[kG], ewma[kG];
  decode(th, space, kind, m, A, B, nu, g0);
  init_state<STATIC>(m, g0, s, ewma, mats, N);
  double mse = 0.0;
  for (int t = 0; t + 1 < nobs; ++t) {
    if (!filter_step<STATIC, HASB, SCALED>(m, A, B, nu, ewma, s, mats, Y + (size_t)t * N, N)) return -HUGE_VAL;
    double vv = 0.0;
    for (int i = 0; i < N; ++i) {
      double z2, z3;
      Point p;
      loadings(s.gamma, s.sc, i, N, mats[i], z2, z3, p);
      const double v = Y[(size_t)(t + 1) * N + i] - msed::fitted(s.beta, z2, z3);
      vv = mfma(v, v, vv);
    }
    mse -= vv;
    if (!(fabs(mse) <= 1.79769313486231570815e308)) return -HUGE_VAL;
  }
  return mse / (double)N / (double)nobs;
}

// get_loss with ∂loss/∂(δ, Φ) in the caller's space (grad: msed::kGrad entries; the algebra and its argument are
// yfm_msed.hpp's: γ, the loadings and β_post never see δ or Φ here either).  The loss is get_loss's, sum for sum.
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double loss_and_grad(const double* th, int space, int kind, const double* mats, const double* Y, int N,
                             int nobs, double (&grad)[msed::kGrad]) {
  Model m;
  State s;
  double A[kG], B[kG], nu[kG], g0[kG], ewma[kG];
  decode(th, space, kind, m, A, B, nu, g0);
  init_state<STATIC>(m, g0, s, ewma, mats, N);
  msed::Grad g;
  msed::grad_zero(g);
  double mse = 0.0;
  bool fail = false;
  for (int t = 0; t + 1 < nobs && !fail; ++t) {
    const double* y = Y + (size_t)t * N;
    const bool pred_only = y[0] != y[0];
    double bpost[kM] = {0.0, 0.0, 0.0};
    if (!filter_step<STATIC, HASB, SCALED>(m, A, B, nu, ewma, s, mats, y, N, bpost)) {
      fail = true;
      break;
    }
    double vv = 0.0, zv[kM] = {0.0, 0.0, 0.0};
    for (int i = 0; i < N; ++i) {
      double z2, z3;
      Point p;
      loadings(s.gamma, s.sc, i, N, mats[i], z2, z3, p);
      const double v = y[N + i] - msed::fitted(s.beta, z2, z3);
      vv = mfma(v, v, vv);
      msed::accum_zv(zv, z2, z3, v);
    }
    mse -= vv;
    fail = !(fabs(mse) <= 1.79769313486231570815e308);
    msed::grad_accum(m, pred_only, zv, bpost, g);  // pred_only: t = 0 (a later missing column was compared: fail)
  }
  msed::grad_finish(g, th, kind_params(kind), space, (double)N, nobs, fail, grad);
  return fail ? -HUGE_VAL : mse / (double)N / (double)nobs;
}

}  // namespace msedn
}  // namespace yfm
