// pe_fields: cuts every block's share out of a global interior array whose
// value encodes (i, j) and checks it node by node — the owned parts tile the
// interior, the rings hold the neighbours' values and zeros on the box
// boundary.  Then pe::gradient_field on two small grids against the
// definition written out.  No device: the sanitizer build's driver of
// pe/fields.hpp (make asan).
//   pe_fields M N PX PY
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pe/fields.hpp"

// Mismatches of pe::gradient_field on P's grid for a w that is non-zero
// everywhere (outside the ellipse too).
static int64_t check_gradient(const pe::Problem& P) {
  const int64_t M = P.M, N = P.N, gny = N - 1, n = (M - 1) * gny;
  const double h1 = P.h1(), h2 = P.h2();
  std::vector<double> w(static_cast<size_t>(n)), gx(w.size(), -7.0), gy(w.size(), -7.0);
  std::vector<double> W(size_t((M + 1) * (N + 1)), 0.0);  // zero-padded copy
  std::vector<char> in(W.size(), 0);
  for (int64_t i = 1; i < M; ++i)
    for (int64_t j = 1; j < N; ++j) {
      const double v = 0.25 + 0.01 * double((i * 37 + j * 11) % 29) - 0.003 * double(j);
      w[size_t((i - 1) * gny + (j - 1))] = v;
      W[size_t(i * (N + 1) + j)] = v;
      in[size_t(i * (N + 1) + j)] = pe::in_ellipse(P.A1 + double(i) * h1, P.A2 + double(j) * h2, P.cx, P.cy);
    }
  const pe::GradStats got = pe::gradient_field(P, w.data(), gx.data(), gy.data());
  const pe::GradStats only = pe::gradient_field(P, w.data(), nullptr, nullptr);
  int64_t bad = 0, inside = 0;
  double sw = 0.0, se = 0.0, mx = 0.0;
  for (int64_t i = 1; i < M; ++i)
    for (int64_t j = 1; j < N; ++j) {
      const int64_t c = i * (N + 1) + j;
      double dx = 0.0, dy = 0.0;
      if (in[size_t(c)]) {
        const bool lo = in[size_t(c - (N + 1))], hi = in[size_t(c + (N + 1))], dn = in[size_t(c - 1)], up = in[size_t(c + 1)];
        if (lo && hi) dx = (W[size_t(c + (N + 1))] - W[size_t(c - (N + 1))]) / (2.0 * h1);
        else if (hi) dx = (W[size_t(c + (N + 1))] - W[size_t(c)]) / h1;
        else if (lo) dx = (W[size_t(c)] - W[size_t(c - (N + 1))]) / h1;
        if (dn && up) dy = (W[size_t(c + 1)] - W[size_t(c - 1)]) / (2.0 * h2);
        else if (up) dy = (W[size_t(c + 1)] - W[size_t(c)]) / h2;
        else if (dn) dy = (W[size_t(c)] - W[size_t(c - 1)]) / h2;
        ++inside;
        sw += W[size_t(c)];
        se += dx * dx + dy * dy;
        mx = std::max(mx, dx * dx + dy * dy);
      }
      if (gx[size_t((i - 1) * gny + (j - 1))] != dx || gy[size_t((i - 1) * gny + (j - 1))] != dy) ++bad;
    }
  if (inside == 0) ++bad;
  if (got.integral != h1 * h2 * sw || got.energy != h1 * h2 * se || got.grad_max != std::sqrt(mx)) ++bad;
  if (only.integral != got.integral || only.energy != got.energy || only.grad_max != got.grad_max) ++bad;
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: pe_fields M N PX PY\n");
    return 2;
  }
  const int M = std::atoi(argv[1]), N = std::atoi(argv[2]);
  pe::ProcessGrid pg;
  pg.Px = std::atoi(argv[3]);
  pg.Py = std::atoi(argv[4]);
  if (M < 2 || N < 2 || pg.Px < 1 || pg.Py < 1 || pg.Px > M - 1 || pg.Py > N - 1) {
    std::fprintf(stderr, "pe_fields: bad grid\n");
    return 2;
  }
  const int64_t gny = int64_t(N) - 1;
  std::vector<double> g(size_t((M - 1) * gny));
  auto code = [&](int64_t i, int64_t j) { return (i < 1 || i > M - 1 || j < 1 || j > N - 1) ? 0.0 : 1e6 * double(i) + double(j); };
  for (int64_t i = 1; i < M; ++i)
    for (int64_t j = 1; j < N; ++j) g[size_t((i - 1) * gny + (j - 1))] = code(i, j);
  std::vector<int> seen(g.size(), 0);
  int64_t bad = 0;
  for (int r = 0; r < pg.Px * pg.Py; ++r) {
    const pe::Block b = pe::decompose(M, N, pg, r);
    const std::vector<double> own = pe::block_field(g.data(), M, N, b, 0);
    const std::vector<double> ring = pe::block_field(g.data(), M, N, b, 1);
    if (int64_t(own.size()) != b.nx * b.ny || int64_t(ring.size()) != (b.nx + 2) * (b.ny + 2)) ++bad;
    for (int64_t li = 0; li <= b.nx + 1; ++li)
      for (int64_t lj = 0; lj <= b.ny + 1; ++lj) {
        const int64_t i = b.i0 - 1 + li, j = b.j0 - 1 + lj;
        if (ring[size_t(li * (b.ny + 2) + lj)] != code(i, j)) ++bad;
        if (li >= 1 && li <= b.nx && lj >= 1 && lj <= b.ny) {
          if (own[size_t((li - 1) * b.ny + (lj - 1))] != code(i, j)) ++bad;
          ++seen[size_t((i - 1) * gny + (j - 1))];
        }
      }
  }
  for (int v : seen)
    if (v != 1) ++bad;
  std::printf("pe_fields %dx%d on %dx%d blocks: %s\n", M, N, pg.Px, pg.Py, bad ? "MISMATCH" : "ok");
  // gradient_field on two small grids (the reference ellipse, and a small
  // ellipse with isolated inside nodes), against the definition written out
  // over a zero-padded copy with an explicit mask
  pe::Problem ref, tiny;
  ref.M = 10;
  ref.N = 50;
  tiny.M = tiny.N = 12;
  tiny.cx = tiny.cy = 30.0;
  tiny.sx = tiny.sy = std::sqrt(30.0);
  const int64_t gbad = check_gradient(ref) + check_gradient(tiny);
  std::printf("pe_fields gradient_field 10x50, 12x12 (cx = cy = 30): %s\n", gbad ? "MISMATCH" : "ok");
  return bad || gbad ? 1 : 0;
}
