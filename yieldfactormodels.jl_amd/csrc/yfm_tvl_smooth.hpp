// yfm_tvl_smooth.hpp — the extended Kalman smoother of the TVλ model (M = 4, P = 31), as plain functions that compile
// for the device (yfm_tvl_smooth.hip) and for the host (tests/tvl_smooth_host_check.cpp).
//
// An extension, as the fixed-loading smoother of yfm_smooth.hpp is: the reference's predict
// (src/models/kalman/filter.jl:250-282) returns the forecasts a_{t+1|t} only.  The model is the one the reference's TVλ
// filter! runs (filter.jl:12-80 with update_factor_loadings!, tvλdns.jl:53-64, from initialize_filter, filter.jl:1-10),
// linearised once, at the forward pass's predicted states a_t, P_t (include/yfm.h yfm_tvl_smooth_batch).  At a data
// column, with λ_t = 0.01 + e^{a₄,t}, Z_t = [1, S(λ_t), C(λ_t), ż_t] (ż_t the Jacobian column as written at
// filter.jl:38-46), v_t = y_t − Z_t[:,1:3]a_t[1:3], G_t = Z_t'Z_t and u_t = Z_t'v_t, the operands of the backward
// recursion are taken from the symmetric form of the capacitance solve (yfm_tvl_grad.hpp primal_update: B̃⁻¹ and
// B̃⁻¹P from a signed Cholesky factor of P and an LDLᵀ, no LU of the non-normal B̃ = σ²I + P_tG_t):
//     s_t = B̃⁻ᵀu_t,   W_t = G_tB̃⁻¹ (triangles averaged),   L_t = Φ(I − P_tW_t) = σ²ΦB̃⁻¹,
//     P_{t|t} = σ²(B̃⁻¹P_t),   a_{t|t} = a_t + P_ts_t,
// so I − P_tW_t is never formed by subtraction.  A missing column has s_t = 0, W_t = 0, L_t = Φ.  The chain
// r_{t−1} = s_t + L_t'r_t, N_{t−1} = W_t + L_t'N_tL_t and the outputs β̂_t, V_t, C_t are chain_step and step_outputs of
// yfm_smooth.hpp at M = 4; a_1 and P_1 are its init_mean and InitCov<4>.
// Every fused multiply-add is an explicit fma; contraction is off.
#pragma once
#include "yfm_smooth.hpp"
#include "yfm_tvl_grad.hpp"

namespace yfm {
namespace tvlsmooth {

namespace sm = smooth;
namespace tg = tvlgrad;

constexpr int kM = 4;

// θ decoded as the TVλ kernels decode it, and the same Q, δ, Φ as the fixed-loading functions read them (no γ)
YFM_SHD void decode(const double* th, int space, tg::Model& gm, sm::Model<kM>& m) {
  tg::decode(th, space, gm);
  m.gam[0] = 0.0;
  m.sigma2 = gm.sigma2;
#pragma unroll
  for (int i = 0; i < kM; ++i) {
    m.delta[i] = gm.delta[i];
#pragma unroll
    for (int j = 0; j < kM; ++j) {
      m.Q[i][j] = gm.Q[i][j];
      m.Phi[i][j] = gm.Phi[i][j];
    }
  }
}

// the statistics of a column (the 14 of yfm_tvl_grad.hpp's Moments::s; its derivative sums are not touched)
YFM_SHD void stats_zero(tg::Moments& mo) {
#pragma unroll
  for (int k = 0; k < tg::NSTAT; ++k) mo.s[k] = 0.0;
}

// one maturity m (rm = 1/m) with z = e^{−λm} and yield y: the primal part of tvlgrad::accum, the same expressions
YFM_SHD void accum(const tg::StepConst& k, const double (&a)[kM], double m, double rm, double z, double y,
                   tg::Moments& mo) {
  const double it = k.rl * rm;
  const double z2 = (1.0 - z) * it;
  const double z3 = z2 - z;
  const double z4 = z * sm::sfma(k.c2, m, sm::sfma(-k.k1, it, k.k1));          // filter.jl:43-46, as written
  const double v = y - sm::sfma(a[2], z3, sm::sfma(a[1], z2, a[0]));          // y − Z[:,1:3]a[1:3]
  double* s = mo.s;
  s[tg::S2] += z2;
  s[tg::S3] += z3;
  s[tg::S4] += z4;
  s[tg::G22] = sm::sfma(z2, z2, s[tg::G22]);
  s[tg::G23] = sm::sfma(z2, z3, s[tg::G23]);
  s[tg::G24] = sm::sfma(z2, z4, s[tg::G24]);
  s[tg::G33] = sm::sfma(z3, z3, s[tg::G33]);
  s[tg::G34] = sm::sfma(z3, z4, s[tg::G34]);
  s[tg::G44] = sm::sfma(z4, z4, s[tg::G44]);
  s[tg::U1] += v;
  s[tg::U2] = sm::sfma(z2, v, s[tg::U2]);
  s[tg::U3] = sm::sfma(z3, v, s[tg::U3]);
  s[tg::U4] = sm::sfma(z4, v, s[tg::U4]);
  s[tg::VV] = sm::sfma(v, v, s[tg::VV]);
}

// The gradient kernel's rule for det B̃ = det(σ²I + PG) of column t (1-based) (yfm_tvl_grad.hpp primal_step): a data
// column whose determinant is zero or not finite makes the candidate unavailable (inv(F) threw), and so does a negative
// one from column 2 on (the log-likelihood's DomainError; on columns 2 … n − 1 the loglik is −Inf already).  Column 1 is
// not among the loss's terms: a non-stationary Φ gives an indefinite P_1, the reference goes on filtering, and so do the
// gradient kernel and this sweep.
YFM_SHD bool det_usable(double det, bool missing, int t) {
  return missing || det > 0.0 || (t == 1 && det < 0.0 && tg::finite(det));
}

// The column's operands and filtered moments from its predicted moments a, P and its statistics; returns det B̃.
YFM_SHD double column_operands(const tg::Model& gm, const sm::Model<kM>& m, const double (&a)[kM],
                             const double (&P)[kM][kM], const tg::Moments& mo, int N, bool missing,
                             sm::StepOps<kM>& o) {
  tg::State st;
#pragma unroll
  for (int i = 0; i < kM; ++i) {
    st.beta[i] = a[i];
#pragma unroll
    for (int j = 0; j < kM; ++j) st.P[i][j] = P[i][j];
  }
  tg::Step u;
  tg::primal_update(gm, st, mo, N, u);  // u.Binv = B̃⁻¹, u.W = B̃⁻¹P (symmetric), u.x = B̃⁻ᵀu, u.det = det B̃
#pragma unroll
  for (int i = 0; i < kM; ++i) o.s[i] = missing ? 0.0 : u.x[i];
  // W = G B̃⁻¹, symmetric in exact arithmetic: the two triangles are averaged so that N stays symmetric to the bit
  double GB[kM][kM];
#pragma unroll
  for (int i = 0; i < kM; ++i)
#pragma unroll
    for (int j = 0; j < kM; ++j) {
      double w = 0.0;
#pragma unroll
      for (int k = 0; k < kM; ++k) w = sm::sfma(u.G[i][k], u.Binv[k][j], w);
      GB[i][j] = w;
    }
#pragma unroll
  for (int i = 0; i < kM; ++i)
#pragma unroll
    for (int j = i; j < kM; ++j) {
      const double w = 0.5 * (GB[i][j] + GB[j][i]);
      o.W[i][j] = missing ? 0.0 : w;
      o.W[j][i] = o.W[i][j];
    }
  // L = σ²ΦB̃⁻¹ (= Φ(I − PW), without the subtraction)
#pragma unroll
  for (int i = 0; i < kM; ++i)
#pragma unroll
    for (int j = 0; j < kM; ++j) {
      double l = 0.0;
#pragma unroll
      for (int k = 0; k < kM; ++k) l = sm::sfma(m.Phi[i][k], u.Binv[k][j], l);
      o.L[i][j] = missing ? m.Phi[i][j] : m.sigma2 * l;
    }
  // a_{t|t} = a + P s,  P_{t|t} = σ²(B̃⁻¹P)
#pragma unroll
  for (int i = 0; i < kM; ++i) {
    double s = a[i];
#pragma unroll
    for (int k = 0; k < kM; ++k) s = sm::sfma(P[i][k], u.x[k], s);
    o.af[i] = missing ? a[i] : s;
#pragma unroll
    for (int j = i; j < kM; ++j) {
      o.Pf[i][j] = missing ? P[i][j] : m.sigma2 * u.W[i][j];
      o.Pf[j][i] = o.Pf[i][j];
    }
  }
  return u.det;
}

}  // namespace tvlsmooth
}  // namespace yfm
