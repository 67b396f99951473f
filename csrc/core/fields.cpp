// Slicing of global interior arrays (user right-hand side / initial guess)
// into one block's share.  Host only.
#include "pe/fields.hpp"

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

}  // namespace pe
