// Problem specification and fictitious-domain geometry for -Δu = F on an
// ellipse embedded in a box, shared verbatim by host (CPU backends, table
// construction) and device (HIP kernels).
//
// Reference parity (mxy-kit/poisson-ellipse-openmp-mpi-cuda):
//   box / RHS constants      stage2-mpi/poisson_mpi_decomp.cpp:9-11
//   domain test x²+4y²<1     stage2-mpi/poisson_mpi_decomp.cpp:18-20
//   face length in D         stage2-mpi/poisson_mpi_decomp.cpp:32-54
//   a_ij / b_ij blend rule   stage2-mpi/poisson_mpi_decomp.cpp:140-155
//   eps = max(h1,h2)^2       stage2-mpi/poisson_mpi_decomp.cpp:361
// The reference hard-codes the ellipse x² + 4y² < 1.  Here the ellipse is
// cx·x² + cy·y² < 1 with (cx, cy) = (1, 4) by default; every expression is
// written so that the default evaluates bit-identically to the reference
// (1.0*x is exact, and the operation order of each formula is preserved).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define PE_HD __host__ __device__ inline
#else
#define PE_HD inline
#endif

namespace pe {

enum class Norm : int { Weighted = 0, Unweighted = 1 };
enum class Init : int { Zero = 0, Random = 1 };
// Stop rule: Step — ‖w^{k+1} − w^k‖ < tol (the reference's); Residual — the
// preconditioned residual sqrt(g_k) ≤ max(tol·sqrt(g_0), atol), g = h1·h2·(z, r).
enum class Stop : int { Step = 0, Residual = 1 };

struct Problem {
  // Box Π = [A1,B1] × [A2,B2].
  double A1 = -1.0, B1 = 1.0, A2 = -0.6, B2 = 0.6;
  // Right-hand side value inside D (F_VAL in the reference).
  double F = 1.0;
  // Ellipse cx·x² + cy·y² < 1 (reference: cx = 1, cy = 4) and the exact
  // square roots of cx, cy used by the reference's |x0| >= 1 / |2 y0| >= 1.
  double cx = 1.0, cy = 4.0, sx = 1.0, sy = 2.0;
  int M = 40, N = 40;
  double tol = 1e-6;
  int64_t max_iter = -1;  // <0 → (M-1)(N-1)
  Norm norm = Norm::Weighted;
  // Constant shift σ ≥ 0 of the operator: (A + σI) w = B, the discrete
  // −Δu + σu = f (pe/fields.hpp).  0.0: −Δu = f, the unshifted code bit for bit.
  double shift = 0.0;
  // Stop rule (Stop above) and, under Stop::Residual only, the absolute floor
  // of its threshold (finite, ≥ 0; pe/fields.hpp check_stop).
  Stop stop = Stop::Step;
  double atol = 0.0;
  // A per-node reaction coefficient c ≥ 0: (A + diag(c)) w = B, the discrete
  // −Δu + c(x, y)·u = f.  The array travels with the solve's fields
  // (pe/fields.hpp UserFields::reaction); this flag fixes the plan.  false:
  // today's code bit for bit.
  bool reaction = false;

  double h1() const { return (B1 - A1) / M; }
  double h2() const { return (B2 - A2) / N; }
  double eps() const {
    const double h = std::max(h1(), h2());
    return h * h;
  }
  int64_t iter_cap() const {
    return max_iter >= 0 ? max_iter : int64_t(M - 1) * int64_t(N - 1);
  }
  int64_t interior_points() const { return int64_t(M - 1) * int64_t(N - 1); }
  // Analytic solution of -Δu = F, u|∂D = 0:  u = F (1 - cx x² - cy y²) / (2cx + 2cy)
  double u_scale() const { return F / (2.0 * cx + 2.0 * cy); }
};

// ---- geometry kernels (host + device) ------------------------------------

PE_HD bool in_ellipse(double x, double y, double cx, double cy) {
  return (cx * x * x + cy * y * y < 1.0);
}

// Length of {x = c, y ∈ [s, e]} ∩ D  (vertical face).  `sx` = sqrt(cx).
PE_HD double seg_len_vertical(double c, double s, double e, double cx, double cy,
                              double sx) {
  if (fabs(sx * c) >= 1.0) return 0.0;
  const double t = fmax(0.0, (1.0 - cx * c * c) / cy);
  const double ymax = sqrt(t);
  const double ymin = -sqrt(t);
  return fmax(0.0, fmin(e, ymax) - fmax(s, ymin));
}

// Length of {y = c, x ∈ [s, e]} ∩ D  (horizontal face).  `sy` = sqrt(cy).
PE_HD double seg_len_horizontal(double c, double s, double e, double cx, double cy,
                                double sy) {
  if (fabs(sy * c) >= 1.0) return 0.0;
  const double t = fmax(0.0, (1.0 - cy * c * c) / cx);
  const double xmax = sqrt(t);
  const double xmin = -sqrt(t);
  return fmax(0.0, fmin(e, xmax) - fmax(s, xmin));
}

// Fictitious-domain face coefficient from the face length l of a face of
// nominal length h:  1 inside, 1/eps outside, length-weighted blend otherwise.
PE_HD double face_coef(double l, double h, double eps) {
  return (fabs(l - h) < 1e-9) ? 1.0
                              : (l < 1e-9 ? 1.0 / eps : (l / h) + (1.0 - l / h) / eps);
}

// Bound of the ellipse chord used by the on-the-fly coefficient tables.
// Vertical faces at x = c: y ∈ [-yb, yb] (yb = -1 encodes "empty chord";
// any face endpoint lies in (-1, 1) so the clamp yields 0 exactly).
PE_HD double chord_half_vertical(double c, double cx, double cy, double sx) {
  if (fabs(sx * c) >= 1.0) return -1.0e300;
  return sqrt(fmax(0.0, (1.0 - cx * c * c) / cy));
}
PE_HD double chord_half_horizontal(double c, double cx, double cy, double sy) {
  if (fabs(sy * c) >= 1.0) return -1.0e300;
  return sqrt(fmax(0.0, (1.0 - cy * c * c) / cx));
}
// Face length from a chord half-width and the face endpoints; identical to
// seg_len_* because ymin = -ymax exactly, and a negative sentinel yields 0.
PE_HD double chord_len(double half, double s, double e) {
  return fmax(0.0, fmin(e, half) - fmax(s, -half));
}

// Deterministic pseudo-random initial guess w⁰(i, j) ∈ [-amp, amp] from a
// hash of the GLOBAL node index, so every rank (and every halo copy) agrees
// without communication.  Zero on the box boundary (Dirichlet).
PE_HD double random_w0(int64_t gi, int64_t gj, int M, int N, uint64_t seed, double amp) {
  if (gi <= 0 || gj <= 0 || gi >= M || gj >= N) return 0.0;
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t(gi) * 0x100000001B3ull + uint64_t(gj));
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const double u01 = double(z >> 11) * (1.0 / 9007199254740992.0);
  return amp * (2.0 * u01 - 1.0);
}

}  // namespace pe
