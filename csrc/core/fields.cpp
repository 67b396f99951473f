// Slicing of global interior arrays (user right-hand side / initial guess)
// into one block's share, and the gradient of a global solution array.  Host only.
#include "pe/fields.hpp"

#include <cmath>
#include <stdexcept>

namespace pe {

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

}  // namespace pe
