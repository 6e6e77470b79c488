// What smooth_host_check.cpp and tvl_smooth_host_check.cpp share: the case file's token reader, a column's record, the
// backward loop over the columns (csrc/yfm_smooth.hpp step_outputs and chain_step) and the hex-float printer.  The
// including driver has included yfm_smooth.hpp (directly or through yfm_tvl_smooth.hpp) and forms the columns'
// operands itself.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace sm = yfm::smooth;

// the next whitespace-separated token as a double (C hex float or "nan")
static double rd(FILE* f) {
  char buf[128];
  if (std::fscanf(f, "%127s", buf) != 1) {
    std::fprintf(stderr, "short input\n");
    std::exit(2);
  }
  return std::strtod(buf, nullptr);
}

// a column's predicted moments and its operands
template <int M>
struct Col {
  double a[M], P[M][M];
  sm::StepOps<M> o;
};

// The backward loop over the window's columns col[0 … n − 1]: per column a row β̂_t (M), V_t (M², column-major), C_t
// (M², column-major; none at the window's last column) of the T rows returned, NaN elsewhere — and everywhere where `ok`
// (the forward half's verdict) or an output's finiteness fails.
template <int M>
static std::vector<double> smooth_backward(const sm::Model<M>& m, const std::vector<Col<M>>& col, int T, bool ok) {
  constexpr int kRow = M + 2 * M * M;
  const int n = (int)col.size();
  std::vector<double> out((size_t)T * kRow, std::nan(""));
  double r[M] = {}, Nm[M][M] = {};
  for (int t = n - 1; t >= 0; --t) {
    const bool lag = t + 1 < n;
    double Pn[M][M] = {}, bs[M], V[M][M], C[M][M];
    if (lag)
      for (int i = 0; i < M; ++i)
        for (int j = 0; j < M; ++j) Pn[i][j] = col[t + 1].P[i][j];
    ok = sm::step_outputs<M>(m, col[t].o.af, col[t].o.Pf, r, Nm, lag, Pn, bs, V, C) && ok;
    double* o = &out[(size_t)t * kRow];
    for (int i = 0; i < M; ++i) {
      o[i] = bs[i];
      for (int j = 0; j < M; ++j) {
        o[M + j * M + i] = V[i][j];
        if (lag) o[M + M * M + j * M + i] = C[i][j];
      }
    }
    sm::chain_step<M>(col[t].o.s, col[t].o.W, col[t].o.L, r, Nm);
  }
  if (!ok)
    for (double& v : out) v = std::nan("");
  return out;
}

// rows of `width` values, one line each: hex floats, "nan" for a NaN
static void print_rows(const std::vector<double>& out, int width) {
  for (size_t e = 0; e < out.size(); ++e) {
    const char* sep = e % width ? " " : "";
    if (out[e] != out[e])
      std::printf("%snan", sep);
    else
      std::printf("%s%a", sep, out[e]);
    if (e % width == (size_t)width - 1) std::printf("\n");
  }
}
