// yfm_msedn_adj.hpp — ∂loss/∂θ over all P rows of the neural Nelson–Siegel models by a reverse (adjoint) sweep, as
// plain functions that compile for the device (yfm_msedn_adj.hip) and for the host
// (tests/msedn_fullgrad_host_check.cpp).  DESIGN.md §3.10 has the derivation; notation is yfm_msedn.hpp's.
//
// It is the derivative of the function get_loss computes (β₁ = G⁻¹Z'y differentiated through), not the reference's
// dual-number path, which strips β's tangent (filter.jl:175).
//
// One data step with column y, entering γ (and e for the scaled kinds):
//   β₁ = OLS(γ, y), g = score(γ; β₁, y), g̃ = g or g/(√(e⁺/c) + ε), γ⁺ = γ + A∘g̃, β₂ = OLS(γ⁺, y),
//   γ_next = ν + B∘γ⁺ (γ⁺ for a random walk), β_pred = μ + Φβ₂, ℓ = −‖y_next − Z(γ_next)β_pred‖².
// pull(γ; a², a³) = Σᵢ a²ᵢ∂Z₂ᵢ/∂γ + a³ᵢ∂Z₃ᵢ/∂γ is accum_pull + finish_score: the score is pull at aʲᵢ = 2βⱼvᵢ.
// The transpose of an OLS fit's Jacobian against a 3-vector w is pull(γ; uⱼvᵢ − (Zu)ᵢβⱼ) with u = G⁻¹w, G the matrix
// msed::ols solved with.  The transpose of the score's Jacobian against ḡ is a Hessian–vector product — symmetric, so
// one forward directional derivative of the score routines along ḡ on the one-direction dual scalar below — plus the
// OLS transpose of β₁ against w = ∂(ḡ·g)/∂β.
#pragma once
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#include "yfm_msedn.hpp"

namespace yfm {
namespace msedn {

// ---- a value with one directional derivative --------------------------------------------------------------------
struct Dual {
  double v, d;
};
YFM_MHD Dual mk(double v, double d) {
  Dual r;
  r.v = v;
  r.d = d;
  return r;
}
YFM_MHD Dual operator+(Dual a, Dual b) { return mk(a.v + b.v, a.d + b.d); }
YFM_MHD Dual operator+(Dual a, double b) { return mk(a.v + b, a.d); }
YFM_MHD Dual operator-(Dual a, Dual b) { return mk(a.v - b.v, a.d - b.d); }
YFM_MHD Dual operator-(Dual a, double b) { return mk(a.v - b, a.d); }
YFM_MHD Dual operator-(double a, Dual b) { return mk(a - b.v, -b.d); }
YFM_MHD Dual operator-(Dual a) { return mk(-a.v, -a.d); }
YFM_MHD Dual operator*(Dual a, Dual b) { return mk(a.v * b.v, mfma(a.d, b.v, a.v * b.d)); }
YFM_MHD Dual operator*(double a, Dual b) { return mk(a * b.v, a * b.d); }
YFM_MHD Dual operator*(Dual a, double b) { return mk(a.v * b, a.d * b); }
YFM_MHD Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return mk(q, (a.d - q * b.d) / b.v);
}
YFM_MHD Dual operator/(double a, Dual b) {
  const double q = a / b.v;
  return mk(q, -(q * b.d) / b.v);
}
YFM_MHD Dual operator/(Dual a, double b) { return mk(a.v / b, a.d / b); }
YFM_MHD Dual dsqrt(Dual a) {
  const double r = sqrt(a.v);
  return mk(r, a.d / (2.0 * r));
}
// a·b + c
YFM_MHD Dual dfma(Dual a, Dual b, Dual c) { return mk(mfma(a.v, b.v, c.v), mfma(a.d, b.v, mfma(a.v, b.d, c.d))); }
YFM_MHD Dual dfma(Dual a, double b, Dual c) { return mk(mfma(a.v, b, c.v), mfma(a.d, b, c.d)); }
YFM_MHD Dual dfma(double a, Dual b, Dual c) { return dfma(b, a, c); }

// ---- the loadings and the score routines of yfm_msedn.hpp along one direction of γ --------------------------------
struct DTau {
  Dual t[kH];
};
YFM_MHD Dual net_raw(const Dual* g, double m, DTau& tau) {
  Dual r = mk(0.0, 0.0);
  for (int h = 0; h < kH; ++h) {
    const Dual x = dfma(g[h], m, g[kH + h]);
    const double th = tanh(x.v);
    tau.t[h] = mk(th, (1.0 - th * th) * x.d);
    r = dfma(g[2 * kH + h], tau.t[h], r);
  }
  return r;
}
YFM_MHD void accum_net(Dual* acc, const Dual* g, const DTau& tau, Dual c, double m) {
  for (int h = 0; h < kH; ++h) {
    const Dual w = (c * g[2 * kH + h]) * (1.0 - tau.t[h] * tau.t[h]);
    acc[h] = dfma(w, m, acc[h]);
    acc[kH + h] = acc[kH + h] + w;
    acc[2 * kH + h] = dfma(c, tau.t[h], acc[2 * kH + h]);
  }
}
struct DScal {
  Dual l2, iu, s3, c3, sc, kap;
};
YFM_MHD void anchors(const Dual* gam, bool anchored, const Ends& e, DScal& s) {
  s.l2 = mk(0.0, 0.0);
  s.iu = mk(1.0, 0.0);
  s.s3 = mk(0.0, 0.0);
  s.c3 = mk(0.0, 0.0);
  if (anchored) return;
  DTau t;
  const Dual a2 = net_raw(gam, e.m0, t);
  s.l2 = net_raw(gam, e.mP, t);
  s.iu = 1.0 / (a2 - s.l2 + kTiny);
  const Dual a3 = net_raw(gam + kBlk, e.m0, t), n3 = net_raw(gam + kBlk, e.mN, t);
  s.s3 = (n3 - a3) / (e.mN - e.m0);
  s.c3 = a3 - s.s3 * e.m0;
}
YFM_MHD Dual resid3(const Dual* gam, const DScal& s, double m, DTau& tau, Dual& r) {
  const Dual raw = net_raw(gam + kBlk, m, tau);
  r = raw - (s.s3 * m - s.c3);
  return r * r;
}
YFM_MHD void finish_scale(Dual Q, bool anchored, DScal& s) {
  const Dual rq = dsqrt(Q);
  if (anchored) {
    s.sc = kScale / rq + kTiny;
    s.kap = kScale / (Q * rq);
  } else {
    s.sc = 1.0 / (rq / kScale + kTiny);
    s.kap = (s.sc * s.sc) / (kScale * rq);
  }
}
struct DPoint {
  DTau t2, t3;
  Dual t, r, q;
};
YFM_MHD void loadings(const Dual* gam, const DScal& s, int i, int N, double m, Dual& z2, Dual& z3, DPoint& p) {
  p.t = (net_raw(gam, m, p.t2) - s.l2) * s.iu;
  p.q = resid3(gam, s, m, p.t3, p.r);
  z2 = i == 0 ? mk(1.0, 0.0) : (in2(i, N) ? p.t * p.t : mk(0.0, 0.0));
  z3 = in3(i, N) ? p.q * s.sc : mk(0.0, 0.0);
}
YFM_MHD void accum_aux(Dual* a, const Dual* gam, const DScal& s, int i, int N, double m) {
  if (!in3(i, N)) return;
  DTau tau;
  Dual r;
  const Dual q = resid3(gam, s, m, tau, r);
  a[AQ] = dfma(q, q, a[AQ]);
  const Dual c = 2.0 * r * q;
  accum_net(a + AH, gam + kBlk, tau, c, m);
  a[AH0] = a[AH0] + c;
  a[AH1] = dfma(m, c, a[AH1]);
}
// accum_score along the direction, with w = ∂(ḡ·g)/∂β (3): wⱼ = 2Σᵢ(vᵢŻᵢⱼ − (Żβ)ᵢZᵢⱼ), Ż the direction's part of Z
YFM_MHD void accum_score(Dual* c, double (&w)[kM], const Dual* gam, const DScal& s, const double (&beta)[kM], int i,
                         int N, double m, double y) {
  Dual z2, z3;
  DPoint p;
  loadings(gam, s, i, N, m, z2, z3, p);
  const Dual v = mk(y - msed::fitted(beta, z2.v, z3.v), -mfma(beta[2], z3.d, beta[1] * z2.d));
  w[0] += 2.0 * v.d;
  w[1] += 2.0 * mfma(v.v, z2.d, v.d * z2.v);
  w[2] += 2.0 * mfma(v.v, z3.d, v.d * z3.v);
  if (in2(i, N)) {
    const Dual d = 2.0 * ((2.0 * beta[1]) * v) * p.t;
    accum_net(c + C1, gam, p.t2, d * s.iu, m);
    c[CU0] = dfma(d, p.t, c[CU0]);
    c[CU1] = dfma(d, p.t - 1.0, c[CU1]);
  }
  if (in3(i, N)) {
    const Dual a3 = (2.0 * beta[2]) * v;
    const Dual cr = (2.0 * p.r) * (a3 * s.sc);
    accum_net(c + C2, gam + kBlk, p.t3, cr, m);
    c[CR0] = c[CR0] + cr;
    c[CR1] = dfma(m, cr, c[CR1]);
    c[CS] = dfma(a3, p.q, c[CS]);
  }
}
// finish_score along the direction: hv receives the direction's part of g alone (the Hessian–vector product)
YFM_MHD void finish_score(const Dual* c, const Dual* aux, const Dual* gam, const DScal& s, bool anchored,
                          const Ends& e, double* hv) {
  Dual g[kG];
  const Dual sk = c[CS] * s.kap;
  for (int k = 0; k < kBlk; ++k) {
    g[k] = c[C1 + k];
    g[kBlk + k] = c[C2 + k] - sk * aux[AH + k];
  }
  if (!anchored) {
    DTau t;
    (void)net_raw(gam, e.mP, t);
    accum_net(g, gam, t, c[CU1] * s.iu, e.mP);
    (void)net_raw(gam, e.m0, t);
    accum_net(g, gam, t, -(c[CU0] * s.iu), e.m0);
    const Dual r0 = c[CR0] - sk * aux[AH0], r1 = c[CR1] - sk * aux[AH1];
    const Dual cn = (-r1 - e.m0 * r0) / (e.mN - e.m0);
    (void)net_raw(gam + kBlk, e.m0, t);
    accum_net(g + kBlk, gam + kBlk, t, r0 - cn, e.m0);
    (void)net_raw(gam + kBlk, e.mN, t);
    accum_net(g + kBlk, gam + kBlk, t, cn, e.mN);
  }
  for (int k = 0; k < kG; ++k) hv[k] = g[k].d;
}

// ---- pull ----------------------------------------------------------------------------------------------------------
// One maturity of pull's sums (the layout of accum_score's, so finish_score finishes them) from its evaluated Point.
// At a² = (2β₂)v, a³ = (2β₃)v this is accum_score, operation for operation.
YFM_MHD void accum_pull(double* c, const double* gam, const Scal& s, const Point& p, int i, int N, double m, double a2,
                        double a3) {
  if (in2(i, N)) {
    const double d = 2.0 * a2 * p.t;
    accum_net(c + C1, gam, p.t2, d * s.iu, m);
    c[CU0] = mfma(d, p.t, c[CU0]);
    c[CU1] = mfma(d, p.t - 1.0, c[CU1]);
  }
  if (in3(i, N)) {
    const double cr = (2.0 * p.r) * (a3 * s.sc);
    accum_net(c + C2, gam + kBlk, p.t3, cr, m);
    c[CR0] += cr;
    c[CR1] = mfma(m, cr, c[CR1]);
    c[CS] = mfma(a3, p.q, c[CS]);
  }
}
// the OLS transpose's coefficients at one maturity: aʲ = uⱼv − (Zu)βⱼ, v = y − Zβ
YFM_MHD void ols_pull_coef(const double (&beta)[kM], const double (&u)[kM], double z2, double z3, double y, double& a2,
                           double& a3) {
  const double v = y - msed::fitted(beta, z2, z3);
  const double zu = msed::fitted(u, z2, z3);
  a2 = mfma(u[1], v, -(zu * beta[1]));
  a3 = mfma(u[2], v, -(zu * beta[2]));
}
// u = G⁻¹w with the matrix msed::ols solved with (ridged: the retry's)
YFM_MHD bool ols_solve(const double (&o)[NOLS], double n, bool ridged, const double (&w)[kM], double (&u)[kM]) {
  const double rd = ridged ? msed::kRidge : 0.0;
  return msed::chol3_solve(n + rd, o[msed::S2], o[msed::S3], o[msed::G22] + rd, o[msed::G23], o[msed::G33] + rd, w, u);
}
// w = Φ'(2s), s = Z'v_n of the compared column: the adjoint of β₂ from ℓ through β_pred = μ + Φβ₂
YFM_MHD void beta_adjoint(const Model& m, const double (&zv)[kM], double (&w)[kM]) {
  for (int c = 0; c < kM; ++c) {
    double a = 0.0;
    for (int r = 0; r < kM; ++r) a = mfma(m.Phi[r][c], 2.0 * zv[r], a);
    w[c] = a;
  }
}

// ---- the adjoint state and its 18-vector algebra -----------------------------------------------------------------
// γ̄ and ē handed from step to step and the accumulators of the rows A, B and ω: 90 doubles per candidate
enum : int { JG = 0, JE = kG, JA = 2 * kG, JB = 3 * kG, JW = 4 * kG, NADJ = 5 * kG };

// forget_factor^n as update_gamma leaves it after n updates is a running product; the adjoint reads the power
YFM_MHD double forget_pow(int n) { return pow(kForget, (double)n); }

// update_gamma with what its adjoint needs kept: e⁺ (ep), s = √(e⁺/c) + ε (sden), g̃ (gt) and γ⁺ (gp)
template <bool SCALED>
YFM_MHD void update_keep(const double* A, const double* gam, const double* ew, double den, const double* g, double* ep,
                         double* sden, double* gt, double* gp) {
  for (int k = 0; k < kG; ++k) {
    double gk = g[k];
    ep[k] = 0.0;
    sden[k] = 1.0;
    if (SCALED) {
      ep[k] = kForget * ew[k] + (1.0 - kForget) * (gk * gk);
      sden[k] = sqrt(ep[k] / den) + msed::kEps;
      gk = gk / sden[k];
    }
    gt[k] = gk;
    gp[k] = gam[k] + gk * A[k];
  }
}

// Items 2–4 of the backward step at component k, given γ̄_next (item 1 added) in adj[JG + k] and p2 = the OLS transpose
// of β₂ at γ⁺.  Leaves γ̄⁺ in adj[JG + k], passes ē on and returns ḡ_k.
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double adjoint_update(double* adj, int k, double A, double B, double omega, double p2, double g, double gt,
                              double gp, double ep, double sden, double den) {
  const double gn = adj[JG + k];
  double gbp = gn;
  if (HASB) {
    gbp = B * gn;
    adj[JB + k] = mfma(gn, gp - omega, adj[JB + k]);
    adj[JW + k] = mfma(1.0 - B, gn, adj[JW + k]);
  }
  gbp = gbp + p2;
  adj[JG + k] = gbp;
  if (STATIC) return 0.0;
  adj[JA + k] = mfma(gbp, gt, adj[JA + k]);
  const double gtb = A * gbp;
  if (!SCALED) return gtb;
  const double r = sden - msed::kEps;
  const double eb = adj[JE + k] - (gtb * g) / (2.0 * den * r * (sden * sden));
  adj[JE + k] = kForget * eb;
  return gtb / sden + (2.0 * (1.0 - kForget)) * g * eb;
}

// Rows 0 … P−13 in the caller's space from the finished adjoint (ω̄ has γ̄₀ added), scaled by 1/(N·nobs); rows
// P−12 … P−1 are tail (grad_finish's).  NaN in every row where the loss is −Inf (fail) and where an adjoint or an
// accumulator is not finite; returns true in the second case alone (the gradient of a finite loss is unavailable).
YFM_MHD bool fullgrad_finish(const double* adj, const double* A, const double* B, const double (&tail)[msed::kGrad],
                             int kind, int space, double n, int nobs, bool fail, double* out /* P */) {
  const double sc = 1.0 / n / (double)nobs;
  const double big = 1.79769313486231570815e308;
  const bool st = kind_static(kind), hb = kind_has_b(kind);
  const int dyn = kind_dyn(kind), nuq = st ? 0 : dyn_unique(dyn);
  const int P = kind_params(kind);
  bool bad = false;
  for (int k = 0; k < NADJ; ++k) bad = bad || !(fabs(adj[k]) <= big);
  int o = 0;
  if (!st) {
    for (int u = 0; u < nuq; ++u) {
      double sa = 0.0, sb = 0.0, av = 0.0, bv = 0.0;
      for (int k = 0; k < kG; ++k)
        if (dup(dyn, k) == u) {
          sa += adj[JA + k];
          sb += adj[JB + k];
          av = A[k];
          bv = B[k];
        }
      sa = sa * sc;
      sb = sb * sc;
      if (space == 0) {
        sa = sa * av;
        sb = sb * (bv * (1.0 - bv));
      }
      out[u] = sa;
      if (hb) out[nuq + u] = sb;
    }
    o = nuq * (hb ? 2 : 1);
  }
  for (int k = 0; k < kG; ++k) out[o + k] = adj[JW + k] * sc;
  for (int k = 0; k < msed::kGrad; ++k) out[o + kG + k] = tail[k];
  for (int k = 0; k < P - msed::kGrad; ++k) bad = bad || !(fabs(out[k]) <= big);
  if (fail || bad)
    for (int k = 0; k < P; ++k) out[k] = __builtin_nan("");
  return bad && !fail;
}

// ---- the sequential form (the host check): every maturity visited in order ------------------------------------
YFM_MHD void prepare_dual(bool anchored, const Dual* gam, DScal& sc, Dual* aux, const double* mats, int N) {
  anchors(gam, anchored, ends_of(mats, N), sc);
  for (int k = 0; k < NAUX; ++k) aux[k] = mk(0.0, 0.0);
  for (int i = 0; i < N; ++i) accum_aux(aux, gam, sc, i, N, mats[i]);
  finish_scale(aux[AQ], anchored, sc);
}

// pull(γ; the OLS transpose's coefficients for (β, u) on column y) at the prepared state s (aux with H)
YFM_MHD void ols_pull(const Model& m, const State& s, const double (&beta)[kM], const double (&u)[kM],
                      const double* mats, const double* y, int N, double* out) {
  double c[NSCORE];
  for (int k = 0; k < NSCORE; ++k) c[k] = 0.0;
  for (int i = 0; i < N; ++i) {
    double z2, z3, a2, a3;
    Point p;
    loadings(s.gamma, s.sc, i, N, mats[i], z2, z3, p);
    ols_pull_coef(beta, u, z2, z3, y[i], a2, a3);
    accum_pull(c, s.gamma, s.sc, p, i, N, mats[i], a2, a3);
  }
  finish_score(c, s.aux, s.gamma, s.sc, m.anchored, ends_of(mats, N), out);
}

// The backward step of one column t: gam, ew the γ and e the step entered with (the trajectory's), den = 1 − fⁿ of its
// update, gnext the γ the next step entered with, y and ynext the columns t and t + 1.  pred_only: column t is
// missing (t = 0).  false where a fit the forward sweep made does not factor here.
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD bool adjoint_step(const Model& m, const double* A, const double* B, const double* omega, const double* gam,
                          const double* ew, double den, const double* gnext, bool pred_only, const double* mats,
                          const double* y, const double* ynext, int N, double* adj) {
  const Ends e = ends_of(mats, N);
  const double fN = (double)N;
  State s1, s2, sn;
  double o1[NOLS], o2[NOLS], b1[kM], b2[kM], bpred[kM];
  double g[kG], ep[kG], sden[kG], gt[kG], gp[kG];
  bool rd1 = false, rd2 = false;
  for (int k = 0; k < kG; ++k) {
    s1.gamma[k] = gam[k];
    sn.gamma[k] = gnext[k];
    g[k] = 0.0;
  }
  if (!pred_only) {
    prepare<true>(m, s1, mats, N);
    ols_pass(s1, mats, y, N, o1);
    if (!msed::ols(o1, fN, b1, rd1)) return false;
    if (!STATIC) {
      double c[NSCORE];
      for (int k = 0; k < NSCORE; ++k) c[k] = 0.0;
      for (int i = 0; i < N; ++i) accum_score(c, s1.gamma, s1.sc, b1, i, N, mats[i], y[i]);
      finish_score(c, s1.aux, s1.gamma, s1.sc, m.anchored, e, g);
    }
    update_keep<SCALED>(A, gam, ew, den, g, ep, sden, gt, gp);
    for (int k = 0; k < kG; ++k) s2.gamma[k] = gp[k];
    prepare<true>(m, s2, mats, N);
    ols_pass(s2, mats, y, N, o2);
    if (!msed::ols(o2, fN, b2, rd2)) return false;
  } else {
    for (int r = 0; r < kM; ++r) b2[r] = m.beta0[r];
  }
  for (int r = 0; r < kM; ++r) {
    double a = 0.0;
    for (int c = 0; c < kM; ++c) a = mfma(m.Phi[r][c], b2[c], a);
    bpred[r] = m.mu[r] + a;
  }
  // 1. the loss term at γ_next
  prepare<true>(m, sn, mats, N);
  double zv[kM] = {0.0, 0.0, 0.0};
  {
    double c[NSCORE], gs[kG];
    for (int k = 0; k < NSCORE; ++k) c[k] = 0.0;
    for (int i = 0; i < N; ++i) {
      double z2, z3;
      Point p;
      loadings(sn.gamma, sn.sc, i, N, mats[i], z2, z3, p);
      const double v = ynext[i] - msed::fitted(bpred, z2, z3);
      msed::accum_zv(zv, z2, z3, v);
      accum_pull(c, sn.gamma, sn.sc, p, i, N, mats[i], (2.0 * bpred[1]) * v, (2.0 * bpred[2]) * v);
    }
    finish_score(c, sn.aux, sn.gamma, sn.sc, m.anchored, e, gs);
    for (int k = 0; k < kG; ++k) adj[JG + k] += gs[k];
  }
  if (pred_only) {  // γ₁ = ν + B∘γ₀ and no β adjoint
    for (int k = 0; k < kG; ++k)
      (void)adjoint_update<true, HASB, false>(adj, k, 0.0, B[k], omega[k], 0.0, 0.0, 0.0, gam[k], 0.0, 1.0, 1.0);
    return true;
  }
  // 2. the OLS transpose of β₂ at γ⁺; 3., 4. accumulators and the update's adjoint
  double w[kM], u[kM] = {0.0, 0.0, 0.0}, p2[kG], gb[kG];
  beta_adjoint(m, zv, w);
  (void)ols_solve(o2, fN, rd2, w, u);
  ols_pull(m, s2, b2, u, mats, y, N, p2);
  for (int k = 0; k < kG; ++k)
    gb[k] = adjoint_update<STATIC, HASB, SCALED>(adj, k, A[k], B[k], omega[k], p2[k], g[k], gt[k], gp[k], ep[k],
                                                 sden[k], den);
  if (STATIC) return true;
  // 5. the score's adjoint: the Hessian–vector product along ḡ, then the OLS transpose of β₁
  Dual dg[kG], daux[NAUX], dc[NSCORE];
  DScal dsc;
  double hv[kG], p1[kG];
  for (int k = 0; k < kG; ++k) dg[k] = mk(gam[k], gb[k]);
  prepare_dual(m.anchored, dg, dsc, daux, mats, N);
  for (int k = 0; k < NSCORE; ++k) dc[k] = mk(0.0, 0.0);
  double w1[kM] = {0.0, 0.0, 0.0};
  for (int i = 0; i < N; ++i) accum_score(dc, w1, dg, dsc, b1, i, N, mats[i], y[i]);
  finish_score(dc, daux, dg, dsc, m.anchored, e, hv);
  (void)ols_solve(o1, fN, rd1, w1, u);
  ols_pull(m, s1, b1, u, mats, y, N, p1);
  for (int k = 0; k < kG; ++k) adj[JG + k] = adj[JG + k] + (hv[k] + p1[k]);
  return true;
}

// doubles of trajectory per step: the entering γ, and e for the scaled kinds
YFM_MHD int traj_stride(int kind) { return kind_scaled(kind) ? 2 * kG : kG; }

// get_loss with ∂loss/∂θ over all P rows in the caller's space (grad: P entries; traj: (nobs − 1)·traj_stride(kind)
// doubles of work).  The loss and rows P−12 … P−1 are loss_and_grad's, sum for sum.  unavailable, where given,
// receives fullgrad_finish's return.
template <bool STATIC, bool HASB, bool SCALED>
YFM_MHD double loss_and_fullgrad(const double* th, int space, int kind, const double* mats, const double* Y, int N,
                                 int nobs, double* traj, double* grad, bool* unavailable = nullptr) {
  constexpr int STR = SCALED ? 2 * kG : kG;
  Model m;
  State s;
  double A[kG], B[kG], nu[kG], g0[kG], ewma[kG];
  decode(th, space, kind, m, A, B, nu, g0);
  init_state<STATIC>(m, g0, s, ewma, mats, N);
  msed::Grad g;
  msed::grad_zero(g);
  double mse = 0.0;
  bool fail = false;
  int steps = 0;
  for (int t = 0; t + 1 < nobs && !fail; ++t) {
    const double* y = Y + (size_t)t * N;
    const bool pred_only = y[0] != y[0];
    double bpost[kM] = {0.0, 0.0, 0.0};
    for (int k = 0; k < kG; ++k) {
      traj[(size_t)t * STR + k] = s.gamma[k];
      if (SCALED) traj[(size_t)t * STR + kG + k] = ewma[k];
    }
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
    msed::grad_accum(m, pred_only, zv, bpost, g);
    ++steps;
  }
  double adj[NADJ];
  for (int k = 0; k < NADJ; ++k) adj[k] = 0.0;
  if (!fail) {
    const bool first_missing = nobs > 1 && Y[0] != Y[0];
    double gnext[kG];
    for (int k = 0; k < kG; ++k) gnext[k] = s.gamma[k];
    for (int t = steps - 1; t >= 0; --t) {
      const double* y = Y + (size_t)t * N;
      const double* rec = traj + (size_t)t * STR;
      const double den = SCALED ? 1.0 - forget_pow(t + (first_missing ? 0 : 1)) : 1.0;
      if (!adjoint_step<STATIC, HASB, SCALED>(m, A, B, g0, rec, rec + (SCALED ? kG : 0), den, gnext, y[0] != y[0], mats,
                                              y, y + N, N, adj))
        adj[JG] = __builtin_nan("");
      for (int k = 0; k < kG; ++k) gnext[k] = rec[k];
    }
    for (int k = 0; k < kG; ++k) adj[JW + k] += adj[JG + k];
  }
  double tail[msed::kGrad];
  msed::grad_finish(g, th, kind_params(kind), space, (double)N, nobs, fail, tail);
  const bool un = fullgrad_finish(adj, A, B, tail, kind, space, (double)N, nobs, fail, grad);
  if (unavailable) *unavailable = un;
  return fail ? -HUGE_VAL : mse / (double)N / (double)nobs;
}

}  // namespace msedn
}  // namespace yfm
