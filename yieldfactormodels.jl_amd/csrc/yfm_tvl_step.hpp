// yfm_tvl_step.hpp — what one maturity contributes to a TVλ EKF step, stated once: the statistics' indices, a
// maturity's loadings and innovation with the 14 sums they feed, and the Gram matrix from the group's sums.  For the
// FP64 loglik kernel (yfm_tvl.hip) and yfm_tvl_grad.hpp (the gradient, score and smoother kernels and the host checks
// under tests/): device and host.  No `fp contract` pragma here and no include that brings one: the text is compiled
// under the includer's setting — the default contraction in yfm_tvl.hip, contraction off in the tangent units
// (yfm_grad.hpp) — which is what each unit had before the text was shared.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define YFM_TVL_HD __host__ __device__ __forceinline__
#else
#define YFM_TVL_HD inline
#endif

namespace yfm {
namespace tvlstep {

// Sufficient statistics of one EKF step, indices into the accumulator array.
// Σ Z_c (c = 2..4), the Gram entries, u = Z'v and v'v, with the innovation
// v = y − Z[:,1:3]β[1:3] formed per maturity as the reference does (filter.jl:33-34): the
// uncentered reconstruction v'v = y'y − 2β'Z'y + β'Gβ loses ‖Z‖‖β‖/‖v‖ digits when the
// loadings are nearly collinear (measured: 1.8e-8 on a random N = 33, T = 3 case).
enum : int { S2 = 0, S3, S4, G22, G23, G24, G33, G34, G44, U1, U2, U3, U4, VV, NSTAT };

// a maturity's 1/τ, loadings and innovation, for what is summed beside the statistics (the tangents' moments)
struct Row {
  double it, z2, z3, z4, v;
};

// one maturity m (rm = 1/m) with z = e^{−λm} and yield y, into the statistics s; rl = 1/λ and k1, c2 are the step's
// constants of the Jacobian column
YFM_TVL_HD void accum_stats(double rl, double k1, double c2, const double (&beta)[4], double m, double rm, double z,
                            double y, double (&s)[NSTAT], Row& r) {
  r.it = rl * rm;             // 1/τ
  r.z2 = (1.0 - z) * r.it;    // (1 − z)/τ
  r.z3 = r.z2 - z;
  // Jacobian column as written (filter.jl:43-46): ((β2+β3)(z/λ − z/(λ²m)) + β3·m·z)·(λ − 0.01)
  //   = z·(k1 − k1/(λm) + c2·m),  k1 = c1/λ
  r.z4 = z * __builtin_fma(c2, m, __builtin_fma(-k1, r.it, k1));
  s[S2] += r.z2;
  s[S3] += r.z3;
  s[S4] += r.z4;
  s[G22] = __builtin_fma(r.z2, r.z2, s[G22]);
  s[G23] = __builtin_fma(r.z2, r.z3, s[G23]);
  s[G24] = __builtin_fma(r.z2, r.z4, s[G24]);
  s[G33] = __builtin_fma(r.z3, r.z3, s[G33]);
  s[G34] = __builtin_fma(r.z3, r.z4, s[G34]);
  s[G44] = __builtin_fma(r.z4, r.z4, s[G44]);
  r.v = y - __builtin_fma(beta[2], r.z3, __builtin_fma(beta[1], r.z2, beta[0]));  // y − Z[:,1:3]β[1:3]
  s[U1] += r.v;
  s[U2] = __builtin_fma(r.z2, r.v, s[U2]);
  s[U3] = __builtin_fma(r.z3, r.v, s[U3]);
  s[U4] = __builtin_fma(r.z4, r.v, s[U4]);
  s[VV] = __builtin_fma(r.v, r.v, s[VV]);
}

// G = Z'Z from the group's sums (G₁₁ = N: the level loading is 1)
YFM_TVL_HD void tvl_gram(const double (&s)[NSTAT], int N, double (&G)[4][4]) {
  G[0][0] = (double)N;
  G[0][1] = G[1][0] = s[S2];
  G[0][2] = G[2][0] = s[S3];
  G[0][3] = G[3][0] = s[S4];
  G[1][1] = s[G22];
  G[1][2] = G[2][1] = s[G23];
  G[1][3] = G[3][1] = s[G24];
  G[2][2] = s[G33];
  G[2][3] = G[3][2] = s[G34];
  G[3][3] = s[G44];
}

}  // namespace tvlstep
}  // namespace yfm
