// Slicing of global interior arrays (user right-hand side / initial guess)
// into one block's share, the gradient of a global solution array, and the
// operator / residual of a global field.  Host only.
#include "pe/fields.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace pe {

void check_shift(const Problem& P, const char* who) {
  if (!std::isfinite(P.shift) || P.shift < 0.0)
    throw std::invalid_argument(std::string(who) + ": shift must be finite and >= 0 (got " + std::to_string(P.shift) +
                                "): a negative shift makes the system indefinite");
}

void check_reaction(const Problem& P, const double* c, const char* who) {
  if (!P.reaction && !c) return;
  if (P.reaction != (c != nullptr))
    throw std::invalid_argument(std::string(who) + ": Problem::reaction and the reaction field go together (the flag is " +
                                (P.reaction ? "set without a field" : "unset with a field") + ")");
  if (P.shift != 0.0)
    throw std::invalid_argument(std::string(who) + ": reaction together with shift != 0 (got " + std::to_string(P.shift) +
                                "): add the constant to the field");
  const int64_t n = (int64_t(P.M) - 1) * (int64_t(P.N) - 1);
  for (int64_t q = 0; q < n; ++q)
    if (!std::isfinite(c[q]) || c[q] < 0.0)
      throw std::invalid_argument(std::string(who) + ": reaction must be finite and >= 0 at every node (entry " +
                                  std::to_string(q) + " is " + std::to_string(c[q]) +
                                  "): a negative coefficient can make the system indefinite");
}

void check_stop(const Problem& P, const char* who) {
  if (P.stop != Stop::Step && P.stop != Stop::Residual)
    throw std::invalid_argument(std::string(who) + ": stop must be \"step\" or \"residual\"");
  if (!std::isfinite(P.atol) || P.atol < 0.0)
    throw std::invalid_argument(std::string(who) + ": atol must be finite and >= 0 (got " + std::to_string(P.atol) + ")");
  if (P.atol != 0.0 && P.stop != Stop::Residual)
    throw std::invalid_argument(std::string(who) + ": atol belongs to the stop rule \"residual\"; the step-size rule has none");
}

std::vector<double> block_field(const double* g, int M, int N, const Block& blk, int ring) {
  if (!g) throw std::invalid_argument("block_field: null array");
  if (ring != 0 && ring != 1) throw std::invalid_argument("block_field: ring must be 0 or 1");
  if (M < 2 || N < 2 || blk.nx < 1 || blk.ny < 1 || blk.i0 < 1 || blk.j0 < 1 || blk.i0 + blk.nx > M ||
      blk.j0 + blk.ny > N)
    throw std::invalid_argument("block_field: block outside the interior of the grid");
  const int64_t gny = int64_t(N) - 1;
  const int64_t rows = blk.nx + 2 * ring, cols = blk.ny + 2 * ring;
  std::vector<double> out(size_t(rows * cols), 0.0);
  for (int64_t a = 0; a < rows; ++a) {
    const int64_t gi = blk.i0 + a - ring;  // global node row
    if (gi < 1 || gi > M - 1) continue;    // box boundary: 0
    for (int64_t b = 0; b < cols; ++b) {
      const int64_t gj = blk.j0 + b - ring;
      if (gj < 1 || gj > N - 1) continue;
      out[size_t(a * cols + b)] = g[(gi - 1) * gny + (gj - 1)];
    }
  }
  return out;
}

GradStats gradient_field(const Problem& P, const double* w, double* gx, double* gy) {
  if (!w) throw std::invalid_argument("gradient_field: null array");
  if ((gx == nullptr) != (gy == nullptr)) throw std::invalid_argument("gradient_field: gx and gy go together");
  if (P.M < 2 || P.N < 2) throw std::invalid_argument("gradient_field: grid too small");
  const int64_t M = P.M, N = P.N, gny = N - 1;
  const double h1 = P.h1(), h2 = P.h2();
  auto in = [&](int64_t i, int64_t j) {
    if (i <= 0 || i >= M || j <= 0 || j >= N) return false;
    return in_ellipse(P.A1 + double(i) * h1, P.A2 + double(j) * h2, P.cx, P.cy);
  };
  auto at = [&](int64_t i, int64_t j) { return w[(i - 1) * gny + (j - 1)]; };
  // one component: the neighbours `lo` / `hi` are read only where they are inside
  auto diff = [](bool in_lo, bool in_hi, auto lo, auto hi, double c, double h) {
    if (in_lo && in_hi) return (hi() - lo()) / (2.0 * h);
    if (in_hi) return (hi() - c) / h;
    if (in_lo) return (c - lo()) / h;
    return 0.0;
  };
  double sw = 0.0, se = 0.0, mx = 0.0;
  for (int64_t i = 1; i < M; ++i)
    for (int64_t j = 1; j < N; ++j) {
      double dx = 0.0, dy = 0.0;
      if (in(i, j)) {
        const double c = at(i, j);
        dx = diff(in(i - 1, j), in(i + 1, j), [&] { return at(i - 1, j); }, [&] { return at(i + 1, j); }, c, h1);
        dy = diff(in(i, j - 1), in(i, j + 1), [&] { return at(i, j - 1); }, [&] { return at(i, j + 1); }, c, h2);
        const double g2 = dx * dx + dy * dy;
        sw += c;
        se += g2;
        mx = std::max(mx, g2);
      }
      if (gx) {
        gx[(i - 1) * gny + (j - 1)] = dx;
        gy[(i - 1) * gny + (j - 1)] = dy;
      }
    }
  GradStats s;
  s.integral = h1 * h2 * sw;
  s.energy = h1 * h2 * se;
  s.grad_max = std::sqrt(mx);
  return s;
}

namespace {

// Rows lo .. hi (global node rows, 1-based) of out = A v, or (resid) of
// out = B − A v; returns this range's Σ v·(A v) or Σ out², row-major.  The
// coefficient rows a_i, a_{i+1} (vertical faces left of the nodes of rows i,
// i+1) and b_i (horizontal faces below the nodes of row i, columns 1 .. N)
// are formed row by row with assemble()'s expressions.
double operator_rows(const Problem& P, const double* v, bool resid, const double* rhs, const double* cr, double* out,
                     int64_t lo, int64_t hi) {
  const int64_t M = P.M, N = P.N, gny = N - 1;
  const double h1 = P.h1(), h2 = P.h2(), eps = P.eps();
  const bool shifted = P.shift != 0.0;
  std::vector<double> a0(size_t(N + 1)), a1(size_t(N + 1)), b(size_t(N + 1));
  auto a_row = [&](int64_t i, std::vector<double>& a) {
    const double x = P.A1 + i * h1;
    for (int64_t j = 1; j < N; ++j) {
      const double y = P.A2 + j * h2;
      a[size_t(j)] = face_coef(seg_len_vertical(x - 0.5 * h1, y - 0.5 * h2, y + 0.5 * h2, P.cx, P.cy, P.sx), h2, eps);
    }
  };
  auto at = [&](int64_t i, int64_t j) {  // 0 on the box boundary
    return (i < 1 || i > M - 1 || j < 1 || j > N - 1) ? 0.0 : v[(i - 1) * gny + (j - 1)];
  };
  double s = 0.0;
  if (lo <= hi) a_row(lo, a1);
  for (int64_t i = lo; i <= hi; ++i) {
    a0.swap(a1);
    a_row(i + 1, a1);
    const double x = P.A1 + i * h1;
    for (int64_t j = 1; j <= N; ++j) {
      const double y = P.A2 + j * h2;
      b[size_t(j)] = face_coef(seg_len_horizontal(y - 0.5 * h2, x - 0.5 * h1, x + 0.5 * h1, P.cx, P.cy, P.sy), h1, eps);
    }
    for (int64_t j = 1; j < N; ++j) {
      const double c = at(i, j);
      const double Ax = -1.0 / h1 * (a1[size_t(j)] * (at(i + 1, j) - c) / h1 - a0[size_t(j)] * (c - at(i - 1, j)) / h1);
      const double Ay = -1.0 / h2 * (b[size_t(j + 1)] * (at(i, j + 1) - c) / h2 - b[size_t(j)] * (c - at(i, j - 1)) / h2);
      const double Av = cr ? shifted_apply(Ax + Ay, cr[(i - 1) * gny + (j - 1)], c)
                           : shifted ? shifted_apply(Ax + Ay, P.shift, c) : Ax + Ay;
      double o = Av;
      if (resid) {
        const double y = P.A2 + j * h2;
        const double Fij = rhs ? rhs[(i - 1) * gny + (j - 1)] : P.F;
        o = (in_ellipse(x, y, P.cx, P.cy) ? Fij : 0.0) - Av;
      }
      if (out) out[(i - 1) * gny + (j - 1)] = o;
      s += resid ? o * o : c * Av;
    }
  }
  return s;
}

double operator_pass(const Problem& P, const double* v, bool resid, const double* rhs, const double* cr, double* out,
                     int T, const char* what) {
  if (!v) throw std::invalid_argument(std::string(what) + ": null array");
  if (P.M < 2 || P.N < 2) throw std::invalid_argument(std::string(what) + ": grid too small");
  check_shift(P, what);
  check_reaction(P, cr, what);
  const int64_t nx = int64_t(P.M) - 1;
  if (T <= 1) return P.h1() * P.h2() * operator_rows(P, v, resid, rhs, cr, out, 1, nx);
  // thread t: the contiguous rows 1 + nx t / T .. nx (t + 1) / T; partials added in thread order
  std::vector<double> part(size_t(T), 0.0);
#pragma omp parallel for schedule(static, 1) num_threads(T)
  for (int t = 0; t < T; ++t)
    part[size_t(t)] = operator_rows(P, v, resid, rhs, cr, out, 1 + (nx * t) / T, (nx * (t + 1)) / T);
  double s = 0.0;
  for (int t = 0; t < T; ++t) s += part[size_t(t)];
  return P.h1() * P.h2() * s;
}

}  // namespace

double apply_operator(const Problem& P, const double* v, double* out, int threads, const double* reaction) {
  return operator_pass(P, v, false, nullptr, reaction, out, threads, "apply_operator");
}

double residual_field(const Problem& P, const double* w, const double* rhs, double* out, int threads,
                      const double* reaction) {
  return operator_pass(P, w, true, rhs, reaction, out, threads, "residual_field");
}

}  // namespace pe
