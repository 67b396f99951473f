// pe_fields: cuts every block's share out of a global interior array whose
// value encodes (i, j) and checks it node by node — the owned parts tile the
// interior, the rings hold the neighbours' values and zeros on the box
// boundary.  Then pe::gradient_field, pe::apply_operator and
// pe::residual_field (unshifted, with Problem::shift and with a reaction
// field, whose ring-1 slices are checked too) on two small grids against their
// definitions written out.  No device: the sanitizer build's driver of pe/fields.hpp (make asan).
//   pe_fields M N PX PY
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
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

// Mismatches of pe::apply_operator / pe::residual_field on P's grid against a
// naive double loop over full coefficient arrays and a zero-padded copy of a
// field that is non-zero everywhere; one and three threads, with and without
// a destination, built-in F and a user right-hand side; the unshifted operator
// and A + σI for two shifts (A_σ v = (Ax + Ay) + σ·v written out), and the
// refusal of a negative or non-finite shift; then A + diag(c) for a reaction
// field c with zeros ((Ax + Ay) + c_ij·v written out), its refusals (a negative
// or non-finite entry, the flag without the field and the reverse, a field
// together with a shift) and its ring-1 slices on 2 × 2 blocks, the device
// plane's form.
static int64_t check_operator(const pe::Problem& P0) {
  const pe::Problem& P = P0;
  const int64_t M = P.M, N = P.N, gny = N - 1, n = (M - 1) * gny, C = N + 2;
  const double h1 = P.h1(), h2 = P.h2(), eps = P.eps();
  std::vector<double> v(static_cast<size_t>(n)), f(v.size());
  std::vector<double> V(size_t((M + 2) * C), 0.0), a(V.size(), 0.0), b(V.size(), 0.0);
  for (int64_t i = 0; i <= M; ++i)
    for (int64_t j = 0; j <= N; ++j) {
      const double x = P.A1 + i * h1, y = P.A2 + j * h2;
      a[size_t(i * C + j)] = pe::face_coef(pe::seg_len_vertical(x - 0.5 * h1, y - 0.5 * h2, y + 0.5 * h2, P.cx, P.cy, P.sx), h2, eps);
      b[size_t(i * C + j)] = pe::face_coef(pe::seg_len_horizontal(y - 0.5 * h2, x - 0.5 * h1, x + 0.5 * h1, P.cx, P.cy, P.sy), h1, eps);
      if (i >= 1 && i < M && j >= 1 && j < N) {
        const double val = 0.25 + 0.01 * double((i * 37 + j * 11) % 29) - 0.003 * double(j);
        v[size_t((i - 1) * gny + (j - 1))] = val;
        V[size_t(i * C + j)] = val;
        f[size_t((i - 1) * gny + (j - 1))] = 1.0 + 0.1 * double((i * 5 + j * 3) % 7);
      }
    }
  int64_t bad = 0;
  for (const double wrong : {-1.0, std::nan(""), HUGE_VAL}) {
    pe::Problem Q = P0;
    Q.shift = wrong;
    try {
      pe::apply_operator(Q, v.data(), nullptr, 1);
      ++bad;
    } catch (const std::invalid_argument&) {
    }
  }
  // the reaction field: 0 .. 35 in steps of 3.5, exact zeros on every eleventh node
  std::vector<double> cr(v.size());
  auto cval = [&](int64_t i, int64_t j) {
    return (i < 1 || i > M - 1 || j < 1 || j > N - 1) ? 0.0 : 3.5 * double((i * 7 + j * 13) % 11);
  };
  for (int64_t i = 1; i < M; ++i)
    for (int64_t j = 1; j < N; ++j) cr[size_t((i - 1) * gny + (j - 1))] = cval(i, j);
  {
    pe::Problem R = P0, S = P0;
    R.reaction = true;
    S.reaction = true;
    S.shift = 1.0;
    std::vector<double> neg = cr, nan = cr, inf = cr;
    neg[3] = -1e-300;
    nan[3] = std::nan("");
    inf[3] = HUGE_VAL;
    auto refused = [&](const pe::Problem& Q, const double* c) {
      try {
        pe::apply_operator(Q, v.data(), nullptr, 1, c);
        pe::residual_field(Q, v.data(), nullptr, nullptr, 1, c);
        return false;
      } catch (const std::invalid_argument&) {
        return true;
      }
    };
    for (const double* c : {neg.data(), nan.data(), inf.data()})
      if (!refused(R, c)) ++bad;
    if (!refused(R, nullptr) || !refused(P0, cr.data()) || !refused(S, cr.data())) ++bad;
    if (M > 2 && N > 2) {  // ring-1 slices: the neighbours' values, zeros on the box boundary
      pe::ProcessGrid pg;
      pg.Px = pg.Py = 2;
      for (int r = 0; r < 4; ++r) {
        const pe::Block blk = pe::decompose(int(M), int(N), pg, r);
        const std::vector<double> ring = pe::block_field(cr.data(), int(M), int(N), blk, 1);
        if (int64_t(ring.size()) != (blk.nx + 2) * (blk.ny + 2)) ++bad;
        for (int64_t li = 0; li <= blk.nx + 1; ++li)
          for (int64_t lj = 0; lj <= blk.ny + 1; ++lj)
            if (ring[size_t(li * (blk.ny + 2) + lj)] != cval(blk.i0 - 1 + li, blk.j0 - 1 + lj)) ++bad;
      }
    }
  }
  for (const int kind : {0, 1, 2, 3})  // σ = 0, 0.75, 40; 3: the reaction field
  for (int mode = 0; mode < 3; ++mode) {  // 0: A v; 1: F − A v; 2: f − A v
    pe::Problem P = P0;
    const bool field = kind == 3;
    const double sigma = kind == 1 ? 0.75 : kind == 2 ? 40.0 : 0.0;
    P.shift = sigma;
    P.reaction = field;
    const double* creact = field ? cr.data() : nullptr;
    const double* rhs = mode == 2 ? f.data() : nullptr;
    std::vector<double> want(v.size());
    double s = 0.0;
    for (int64_t i = 1; i < M; ++i)
      for (int64_t j = 1; j < N; ++j) {
        const int64_t c = i * C + j, o = (i - 1) * gny + (j - 1);
        const double Ax = -1.0 / h1 * (a[size_t(c + C)] * (V[size_t(c + C)] - V[size_t(c)]) / h1 - a[size_t(c)] * (V[size_t(c)] - V[size_t(c - C)]) / h1);
        const double Ay = -1.0 / h2 * (b[size_t(c + 1)] * (V[size_t(c + 1)] - V[size_t(c)]) / h2 - b[size_t(c)] * (V[size_t(c)] - V[size_t(c - 1)]) / h2);
        double r = Ax + Ay;
        if (field) r = r + cr[size_t(o)] * V[size_t(c)];  // (every node, c = 0 included)
        else if (sigma != 0.0) r = r + sigma * V[size_t(c)];
        if (mode) {
          const bool in = pe::in_ellipse(P.A1 + i * h1, P.A2 + j * h2, P.cx, P.cy);
          r = (in ? (rhs ? rhs[size_t(o)] : P.F) : 0.0) - r;
        }
        want[size_t(o)] = r;
        s += mode ? r * r : V[size_t(c)] * r;
      }
    for (int T : {1, 3}) {
      std::vector<double> got(v.size(), -7.0);
      const double sum = mode ? pe::residual_field(P, v.data(), rhs, got.data(), T, creact)
                              : pe::apply_operator(P, v.data(), got.data(), T, creact);
      const double only = mode ? pe::residual_field(P, v.data(), rhs, nullptr, T, creact)
                               : pe::apply_operator(P, v.data(), nullptr, T, creact);
      if (got != want || only != sum) ++bad;
      if (T == 1 ? sum != h1 * h2 * s : std::fabs(sum - h1 * h2 * s) > 1e-12 * std::fabs(h1 * h2 * s)) ++bad;
    }
  }
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
  const int64_t obad = check_operator(ref) + check_operator(tiny);
  std::printf("pe_fields apply_operator / residual_field 10x50, 12x12 (cx = cy = 30), shift 0, 0.75, 40 and a reaction "
              "field: %s\n",
              obad ? "MISMATCH" : "ok");
  return bad || gbad || obad ? 1 : 0;
}
