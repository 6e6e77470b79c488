// Host build of the fixed-loading filter's measurement update (csrc/yfm_fixedz.hpp: collapsed_innov inside
// collapsed_mean / collapsed_update, FixedZFilter::setup and ::step) for DNS (M = 3), run through T = 40 filters
// beside (a) the mean update as it stood before G⁻¹ was read directly (ĉ = R·(z̃/σ²), ĉ₀ += ȳ, c = ĉ − β: kept
// here as old_innov) and (b) the same filter in binary128 (__float128, libquadmath), the value both are judged
// against.  Stand-alone (its own main), so it runs under -fsanitize=address,undefined as it is; the device-only
// intrinsics come from tools/host_fixedz/stub.
//
// Every case starts all three filters from the same doubles (λ, σ², Φ, Q, δ, β₀, P₀, the panel), so the
// differences are the rounding of the loadings, G⁻¹ and the recursion alone.
//
//   fixedz_mean_host_check        prints one line per case:
//       case N sigma2 phi ll128 err_old err_new          (errors relative to |ll128|)
// and exits 1 if the forms that must agree bit for bit do not (collapsed_update against collapsed_cov +
// collapsed_mean, and FixedZFilter::step against the loop here), 2 if a case is not a collapsed lane.
#include <quadmath.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "yfm_fixedz.hpp"

using namespace yfm;

namespace {

constexpr int M = 3, NZ = 2, NP = 30, T = 40;

// ---- the update before this change (the R·(z̃/σ²) form), kept to measure the new one against ----
void old_innov(const double (&zt)[NZ], double ybar, double ytt, const double (&R)[M][M], double rsig2,
               const double (&beta)[M], double (&c)[M], double& rr) {
  double zs[NZ];
  for (int j = 0; j < NZ; ++j) zs[j] = zt[j] * rsig2;
  double ch[M];
  for (int i = 0; i < M; ++i) {
    double s = 0.0;
    for (int j = 1; j < M; ++j) s = fma(R[i][j], zs[j - 1], s);
    ch[i] = s;
  }
  rr = ytt;
  for (int j = 1; j < M; ++j) rr = fma(-zt[j - 1], ch[j], rr);
  ch[0] += ybar;
  for (int i = 0; i < M; ++i) c[i] = ch[i] - beta[i];
}

// the rest of the update, which did not change: S = P + R, x = S⁻¹c, q, β_{t|t}, P_{t|t} = P S⁻¹R
void finish_update(const double (&c)[M], double rr, const double (&R)[M][M], double rsig2, const double (&beta)[M],
                   const double (&Pm)[M][M], double (&bf)[M], double (&Pf)[M][M], double& det, double& q) {
  // collapsed_cov is the covariance half; the mean half's tail is restated (solve, c'x, q, β + Px)
  LDLT<M> f;
  det = collapsed_cov<M>(R, Pm, f, Pf);
  double x[M];
  for (int i = 0; i < M; ++i) x[i] = c[i];
  f.solve(x);
  double cx = 0.0;
  for (int i = 0; i < M; ++i) cx = fma(c[i], x[i], cx);
  q = fma(rr, rsig2, cx);
  for (int i = 0; i < M; ++i) {
    double s = beta[i];
    for (int k = 0; k < M; ++k) s = fma(Pm[i][k], x[k], s);
    bf[i] = s;
  }
}

// z̃ = Z'ỹ as yfm_kernels.hip's dot_zt (two partial sums per column)
void dot_zt(const double* col, const double (&Zc)[NZ][NP], double (&zt)[NZ]) {
  double a[NZ][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int i = 0; i < NP; i += 2)
    for (int cz = 0; cz < NZ; ++cz) {
      a[cz][0] = fma(Zc[cz][i], col[i], a[cz][0]);
      a[cz][1] = fma(Zc[cz][i + 1], col[i + 1], a[cz][1]);
    }
  for (int cz = 0; cz < NZ; ++cz) zt[cz] = a[cz][0] + a[cz][1];
}

struct Case {
  int N;
  double sigma2;
  const char* phi_name;
  Params<M, 1> p;
  std::vector<double> mats, Y;  // Y: N×T column-major
};

// ---- binary128: the collapsed form of yfm_kernels.hip's header, every operation in __float128 ----
typedef __float128 q128;

void inv3(const q128 (&A)[3][3], q128 (&X)[3][3], q128& det) {
  const q128 c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
             c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
  X[0][0] = c00 / det;
  X[1][0] = c01 / det;
  X[2][0] = c02 / det;
  X[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
  X[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
  X[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
  X[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
  X[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
  X[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
}

q128 truth_loglik(const Case& cs, const double (&beta0)[M], const double (&P0)[M][M]) {
  const int N = cs.N;
  const q128 lam = (q128)1e-2 + expq((q128)cs.p.gam[0]);
  std::vector<q128> Z((size_t)N * 3);
  for (int i = 0; i < N; ++i) {
    const q128 tau = lam * (q128)cs.mats[i];
    const q128 z = expq(-tau);
    const q128 s = ((q128)1.0 - z) / tau;
    Z[i * 3 + 0] = 1.0;
    Z[i * 3 + 1] = s;
    Z[i * 3 + 2] = s - z;
  }
  q128 G[3][3], Gi[3][3], detG;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      q128 s = 0.0;
      for (int i = 0; i < N; ++i) s += Z[i * 3 + a] * Z[i * 3 + b];
      G[a][b] = s;
    }
  inv3(G, Gi, detG);
  const q128 sig2 = cs.p.sigma2;
  q128 beta[3], P[3][3], R[3][3];
  for (int a = 0; a < 3; ++a) {
    beta[a] = beta0[a];
    for (int b = 0; b < 3; ++b) {
      P[a][b] = P0[a][b];
      R[a][b] = sig2 * Gi[a][b];
    }
  }
  q128 sum = 0.0;
  for (int t = 0; t < T - 1; ++t) {
    const double* y = cs.Y.data() + (size_t)t * N;
    q128 zy[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < N; ++i)
      for (int a = 0; a < 3; ++a) zy[a] += Z[i * 3 + a] * (q128)y[i];
    q128 ch[3];
    for (int a = 0; a < 3; ++a) ch[a] = Gi[a][0] * zy[0] + Gi[a][1] * zy[1] + Gi[a][2] * zy[2];
    q128 rr = 0.0;
    for (int i = 0; i < N; ++i) {
      const q128 r = (q128)y[i] - (Z[i * 3] * ch[0] + Z[i * 3 + 1] * ch[1] + Z[i * 3 + 2] * ch[2]);
      rr += r * r;
    }
    q128 S[3][3], Si[3][3], detS;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[a][b] = P[a][b] + R[a][b];
    inv3(S, Si, detS);
    q128 c[3], x[3];
    for (int a = 0; a < 3; ++a) c[a] = ch[a] - beta[a];
    for (int a = 0; a < 3; ++a) x[a] = Si[a][0] * c[0] + Si[a][1] * c[1] + Si[a][2] * c[2];
    const q128 qf = rr / sig2 + (c[0] * x[0] + c[1] * x[1] + c[2] * x[2]);
    if (t >= 1) sum += (q128)(N - M) * logq(sig2) + logq(detG) + logq(detS) + (q128)N * logq((q128)8.0 * atanq((q128)1.0)) + qf;
    q128 bf[3], PSi[3][3], Pf[3][3];
    for (int a = 0; a < 3; ++a) bf[a] = beta[a] + (P[a][0] * x[0] + P[a][1] * x[1] + P[a][2] * x[2]);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) PSi[a][b] = P[a][0] * Si[0][b] + P[a][1] * Si[1][b] + P[a][2] * Si[2][b];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Pf[a][b] = PSi[a][0] * R[0][b] + PSi[a][1] * R[1][b] + PSi[a][2] * R[2][b];
    q128 Phi[3][3], A[3][3];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Phi[a][b] = cs.p.Phi[a][b];
    for (int a = 0; a < 3; ++a) beta[a] = (q128)cs.p.delta[a] + Phi[a][0] * bf[0] + Phi[a][1] * bf[1] + Phi[a][2] * bf[2];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) A[a][b] = Phi[a][0] * Pf[0][b] + Phi[a][1] * Pf[1][b] + Phi[a][2] * Pf[2][b];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        P[a][b] = (q128)cs.p.Q[a][b] + A[a][0] * Phi[b][0] + A[a][1] * Phi[b][1] + A[a][2] * Phi[b][2];
    for (int a = 0; a < 3; ++a)
      for (int b = a + 1; b < 3; ++b) P[a][b] = P[b][a] = (q128)0.5 * (P[a][b] + P[b][a]);
  }
  return (q128)-0.5 * sum;
}

// ---- deterministic inputs ----
struct Rng {
  unsigned long long s;
  double uni() {  // (0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(s >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  }
  double gauss() { return sqrt(-2.0 * log(uni())) * cos(6.283185307179586 * uni()); }
};

Case make_case(int N, double sigma2, int phi_kind, unsigned long long seed) {
  Case c;
  c.N = N;
  c.sigma2 = sigma2;
  c.p.gam[0] = log(0.0609 - 1e-2);
  c.p.sigma2 = sigma2;
  static const double phis[3][3][3] = {
      {{0.95, 0.02, 0.0}, {-0.01, 0.90, 0.03}, {0.02, 0.0, 0.85}},     // ordinary
      {{0.9995, 0.0, 0.0}, {0.0, 0.98, 0.01}, {0.0, 0.02, 0.95}},      // near a unit root
      {{0.90, 0.30, 0.0}, {-0.30, 0.90, 0.0}, {0.05, 0.0, 0.80}}};     // eigenvalues 0.9 ± 0.3i
  static const char* names[3] = {"ordinary", "unit-root", "complex"};
  c.phi_name = names[phi_kind];
  const double U[3][3] = {{0.30, 0.05, -0.02}, {0.0, 0.25, 0.04}, {0.0, 0.0, 0.40}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      c.p.Phi[i][j] = phis[phi_kind][i][j];
      double s = 0.0;
      for (int l = 0; l < 3; ++l) s = fma(U[l][i], U[l][j], s);
      c.p.Q[i][j] = s;
    }
  const double mu[3] = {5.0, -1.5, 0.8};  // δ = (I − Φ)μ
  for (int i = 0; i < 3; ++i) {
    double s = mu[i];
    for (int j = 0; j < 3; ++j) s -= c.p.Phi[i][j] * mu[j];
    c.p.delta[i] = s;
  }
  c.mats.resize(N);
  for (int i = 0; i < N; ++i) c.mats[i] = 3.0 * pow(120.0, N > 1 ? (double)i / (N - 1) : 0.0);  // 3 … 360 months
  // a panel drawn from the model itself
  Rng r{seed};
  const double lam = 1e-2 + exp(c.p.gam[0]);
  double b[3] = {mu[0], mu[1], mu[2]};
  c.Y.resize((size_t)N * T);
  for (int t = 0; t < T; ++t) {
    double nb[3];
    for (int i = 0; i < 3; ++i) {
      double s = c.p.delta[i];
      for (int j = 0; j < 3; ++j) s += c.p.Phi[i][j] * b[j];
      nb[i] = s;
    }
    const double e[3] = {r.gauss(), r.gauss(), r.gauss()};
    for (int i = 0; i < 3; ++i) {
      b[i] = nb[i];
      for (int l = 0; l < 3; ++l) b[i] += U[l][i] * e[l];
    }
    for (int i = 0; i < N; ++i) {
      const double tau = lam * c.mats[i], z = exp(-tau), s = (1.0 - z) / tau;
      c.Y[(size_t)t * N + i] = b[0] + b[1] * s + b[2] * (s - z) + sqrt(sigma2) * r.gauss();
    }
  }
  return c;
}

double finish_loglik(int N, double sigma2, double logdetG, const LogDetAcc& ld, double sumq) {
  const int nterms = T - 2;
  const double per_term = (double)(N - M) * log(sigma2) + logdetG + (double)N * kLog2Pi;
  return -0.5 * ((double)nterms * per_term + ld.log_value() + sumq);
}

int run_case(const Case& cs) {
  const int N = cs.N;
  constexpr int LDP = NP + 4;
  // prep_panel_kernel: centred columns, ȳ, ỹ'ỹ
  std::vector<double> panel((size_t)T * LDP, 0.0);
  for (int t = 0; t < T; ++t) {
    const double* y = cs.Y.data() + (size_t)t * N;
    double* o = panel.data() + (size_t)t * LDP;
    double s1 = 0.0, yy = 0.0;
    for (int i = 0; i < N; ++i) {
      s1 += y[i];
      yy = fma(y[i], y[i], yy);
    }
    const double ybar = s1 / (double)N;
    double tt = 0.0;
    for (int i = 0; i < N; ++i) {
      o[i] = y[i] - ybar;
      tt = fma(o[i], o[i], tt);
    }
    o[NP] = ybar;
    o[NP + 1] = tt;
    o[NP + 3] = yy;
  }
  // the kernels' loadings (yfm_kernels.hip) and Z'Z
  double Zc[NZ][NP];
  const double lam = 1e-2 + exp(cs.p.gam[0]);
  for (int i = 0; i < NP; ++i) {
    const double tau = lam * cs.mats[i < N ? i : N - 1];
    const double z = exp(-tau);
    const double s = (1.0 - z) / tau;
    Zc[0][i] = (i < N) ? s : 0.0;
    Zc[1][i] = (i < N) ? s - z : 0.0;
  }
  double G[M][M];
  G[0][0] = (double)N;
  for (int c = 0; c < NZ; ++c) {
    double s = 0.0;
    for (int i = 0; i < NP; ++i) s += Zc[c][i];
    G[0][c + 1] = G[c + 1][0] = s;
    for (int d = c; d < NZ; ++d) {
      double g = 0.0;
      for (int i = 0; i < NP; ++i) g = fma(Zc[c][i], Zc[d][i], g);
      G[c + 1][d + 1] = G[d + 1][c + 1] = g;
    }
  }
  FixedZFilter<M, 1, false> f;  // the filter as the kernels run it (full recursion, one-body update)
  f.p = cs.p;
  f.steady_ok = false;
  f.setup(G, N, true);
  if (!f.collapsed || !f.init_ok) return 2;
  double beta0[M], P0[M][M];
  for (int i = 0; i < M; ++i) {
    beta0[i] = f.beta[i];
    for (int j = 0; j < M; ++j) P0[i][j] = f.Pm[i][j];
  }

  struct State {
    double beta[M], Pm[M][M];
    LogDetAcc ld;
    double sumq = 0.0;
  } nw, od;
  for (int i = 0; i < M; ++i) {
    nw.beta[i] = od.beta[i] = beta0[i];
    for (int j = 0; j < M; ++j) nw.Pm[i][j] = od.Pm[i][j] = P0[i][j];
  }
  unsigned flags[8] = {0};
  for (int t = 0; t < T - 1; ++t) {
    const double* col = panel.data() + (size_t)t * LDP;
    double zt[NZ];
    dot_zt(col, Zc, zt);
    const double ybar = col[NP], ytt = col[NP + 1];
    // new form: the one-body update, and the two halves beside it (bit for bit)
    double bf[M], Pf[M][M], det, q;
    collapsed_update<M>(zt, ybar, ytt, f.R, f.Gi, f.rsig2, nw.beta, nw.Pm, bf, Pf, det, q);
    {
      LDLT<M> fl;
      double Pf2[M][M], bf2[M], q2;
      const double det2 = collapsed_cov<M>(f.R, nw.Pm, fl, Pf2);
      collapsed_mean<M>(zt, ybar, ytt, f.R, f.Gi, f.rsig2, nw.beta, nw.Pm, fl, bf2, q2);
      bool same = det2 == det && q2 == q;
      for (int i = 0; i < M; ++i) {
        same = same && bf2[i] == bf[i];
        for (int j = i; j < M; ++j) same = same && Pf2[i][j] == Pf[i][j];
      }
      if (!same) {
        std::fprintf(stderr, "collapsed_update and collapsed_cov + collapsed_mean differ at step %d\n", t);
        return 1;
      }
    }
    propagate_state<M, 1>(cs.p, bf, Pf, nw.beta, nw.Pm);
    if (t >= 1) {
      nw.ld.mul(det);
      nw.sumq += q;
    }
    // old form
    double c[M], rr;
    old_innov(zt, ybar, ytt, f.R, f.rsig2, od.beta, c, rr);
    finish_update(c, rr, f.R, f.rsig2, od.beta, od.Pm, bf, Pf, det, q);
    propagate_state<M, 1>(cs.p, bf, Pf, od.beta, od.Pm);
    if (t >= 1) {
      od.ld.mul(det);
      od.sumq += q;
    }
    // the filter object itself
    f.step(t, zt, make_double2(ybar, ytt), make_double2(0.0, col[NP + 3]), t >= 1, T - 1, T - 1);
  }
  const double ll_new = finish_loglik(N, cs.sigma2, f.logdetG, nw.ld, nw.sumq);
  const double ll_old = finish_loglik(N, cs.sigma2, f.logdetG, od.ld, od.sumq);
  const double ll_obj = f.loglik(T, flags);
  if (ll_obj != ll_new) {
    std::fprintf(stderr, "FixedZFilter::step gives %a, the loop over collapsed_update %a\n", ll_obj, ll_new);
    return 1;
  }
  const q128 ll = truth_loglik(cs, beta0, P0);
  const double e_old = (double)(fabsq((q128)ll_old - ll) / fabsq(ll));
  const double e_new = (double)(fabsq((q128)ll_new - ll) / fabsq(ll));
  std::printf("case %d %.0e %s %.17g %.6e %.6e\n", N, cs.sigma2, cs.phi_name, (double)ll, e_old, e_new);
  return 0;
}

}  // namespace

int main() {
  const int Ns[4] = {3, 8, 25, 30};
  const double s2[3] = {1e-6, 1e-2, 1.0};
  unsigned long long seed = 20240607ull;
  for (int N : Ns)
    for (double sg : s2)
      for (int k = 0; k < 3; ++k) {
        const Case c = make_case(N, sg, k, seed++);
        const int rc = run_case(c);
        if (rc != 0) {
          std::fprintf(stderr, "case N=%d sigma2=%g phi=%s: rc %d\n", N, sg, c.phi_name, rc);
          return rc;
        }
      }
  return 0;
}
