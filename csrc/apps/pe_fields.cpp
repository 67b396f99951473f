// pe_fields: cuts every block's share out of a global interior array whose
// value encodes (i, j) and checks it node by node — the owned parts tile the
// interior, the rings hold the neighbours' values and zeros on the box
// boundary.  No device: the sanitizer build's driver of pe/fields.hpp
// (make asan).
//   pe_fields M N PX PY
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pe/fields.hpp"

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
  return bad ? 1 : 0;
}
