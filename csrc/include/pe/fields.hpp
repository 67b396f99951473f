// User fields of a solve: the right-hand side, the initial guess and the exact
// solution as arrays over the global interior, and the one function that cuts a block's share
// out of such an array (every backend and the Python binding slice with it).
//
// A global interior array is (M-1) × (N-1), row-major in i, entry
// [i-1][j-1] at node (x_i, y_j) — the shape `w_out` / `--dump` produce.
//   rhs: B_ij = rhs_ij at nodes inside the ellipse, 0 elsewhere (the
//        reference's mask, stage2-mpi/poisson_mpi_decomp.cpp:160-169, with
//        F_VAL replaced per node);
//   w0:  the initial guess, r⁰ = B − A w⁰ (box-boundary values are 0; nodes
//        outside the ellipse are unknowns of the fictitious-domain system and
//        may start non-zero).  Overrides SolveOptions::init.
//   exact: the solution to measure the end-of-solve error against, l2_err =
//        sqrt(h1 h2 Σ_D (w − exact)²) and max_err = max_D |w − exact| over the
//        nodes inside the ellipse (values outside are ignored).  It takes the
//        place of the built-in analytic solution and never enters the solve.
//   reaction: the coefficient c of −Δu + c(x, y)·u = f (Problem::reaction goes
//        with it): the system is (A + diag(c)) w = B at every interior node of
//        the box, inside and outside the ellipse; B and its mask, the stop
//        rules, norms, cap and statuses are unchanged; the preconditioner is
//        D + c.  Per node exactly the shifted trees below with c_ij for σ —
//        shifted_apply(Ax + Ay, c_ij, p_ij) and shifted_diag(D_ij, c_ij) —
//        at every node alike, c_ij = 0 included (Av + 0·p: no branch per
//        node).  Finite and ≥ 0 everywhere (check_reaction); the built-in
//        analytic solution does not apply (l2_err = max_err = −1 without
//        `exact`).  The host paths read it at owned nodes (block_field ring
//        0), the device kernels one node beyond (ring 1: kF forms p on the
//        halo ring).
// A null field keeps the built-in path (constant F / Init / the analytic
// error, or -1 with a user rhs) bit for bit.
#pragma once

#include <cstdint>
#include <vector>

#include "pe/decomp.hpp"
#include "pe/problem.hpp"

namespace pe {

struct UserFields {
  const double* rhs = nullptr;
  const double* w0 = nullptr;
  const double* exact = nullptr;
  const double* reaction = nullptr;
};

// Block `blk`'s share of the global interior array `g` of an M × N grid,
// dense row-major.  ring = 0: the owned nx × ny part (element [li-1][lj-1] =
// local node (li, lj)); ring = 1: the owned part plus a one-node ring,
// (nx+2) × (ny+2) (element [li][lj]), the ring holding the neighbours' values
// and zeros on the box boundary.  Local (li, lj) is global (i0-1+li, j0-1+lj)
// as in Block; all indices 64-bit.
std::vector<double> block_field(const double* g, int M, int N, const Block& blk, int ring);

// The gradient of a solution and three integral functionals of it — one
// definition for every backend (the device kernel kGradField is its twin).
// in(i, j) = in_ellipse(x_i, y_j), false on the box boundary i ∈ {0, M},
// j ∈ {0, N}.  At a node with in(i, j):
//   gx = (w[i+1,j] − w[i−1,j]) / (2.0 h1)   both x neighbours inside,
//        (w[i+1,j] − w[i,j]) / h1           only i+1 inside,
//        (w[i,j] − w[i−1,j]) / h1           only i−1 inside,
//        0.0                                neither;
// gy alike in j with h2.  Outside the ellipse gx = gy = 0.0 whatever w is
// there.  One subtraction and one true division per component: every backend
// gives the same bits from the same w.
//   integral = h1 h2 Σ_D w,  energy = h1 h2 Σ_D (gx² + gy²),
//   grad_max = sqrt(max_D (gx² + gy²))   (the maximum is taken of the squares).
// −1: not computed.
struct GradStats {
  double integral = -1.0, energy = -1.0, grad_max = -1.0;
};

// `w` is the global interior array of `prob`'s grid; gx / gy receive arrays of
// the same shape (both null: the functionals only).  Host only.
GradStats gradient_field(const Problem& prob, const double* w, double* gx, double* gy);

// The fictitious-domain operator applied to a user field, and the residual
// field of an iterate — one definition for every backend (the device kernel
// kApplyField is its twin).  Coefficients a, b = face_coef(seg_len_*) as the
// CPU solver's assemble() forms them; the expression is its apply_A's tree,
// Ax + Ay, the reference's.  Sums run in row-major order; threads > 1 splits
// the rows as the CPU solver's row_sum does (thread partials added in thread order).
//
// out = A v over the global interior (M−1) × (N−1); v is 0 on the box boundary.
// Every interior node, inside or outside the ellipse (the fictitious-domain
// system has unknowns everywhere).  Returns h1·h2·Σ v·(A v).  `out` may be
// null: the sum only.  With prob.shift = σ > 0 both functions take A_σ (below)
// for A: out = A_σ v and h1·h2·Σ v·(A_σ v), out = B − A_σ w and h1·h2·Σ out².
// `reaction` (with prob.reaction): the global interior array c of A + diag(c),
// per node the same tree with c_ij for σ.
double apply_operator(const Problem& prob, const double* v, double* out, int threads = 1,
                      const double* reaction = nullptr);
// The shifted operator A_σ = A + σI (Problem::shift = σ > 0; −Δu + σu = f) —
// the two expression trees every backend uses, host and device:
//   A_σ p = (Ax + Ay) + σ·p     the unshifted tree, then one multiply and one add;
//   D_σ   = D + σ               D = (a₁+a₀)/h1² + (b₁+b₀)/h2² (the fast device
//                               variant: its own sum of products), z = r / D_σ.
// Nothing is contracted into an FMA (host: no FMA target; device: kernels.hip
// is built with -ffp-contract=off).  The system holds at every interior node
// of the box, inside and outside the ellipse; B and its mask are unchanged.
// σ = 0 never comes here: callers keep the unshifted expression (not x + 0·p).
PE_HD double shifted_apply(double Av, double sigma, double p) { return Av + sigma * p; }
PE_HD double shifted_diag(double D, double sigma) { return D + sigma; }
// std::invalid_argument unless prob.shift is finite and ≥ 0 (a negative shift
// makes the system indefinite).  Every backend calls it before any work.
void check_shift(const Problem& prob, const char* who);
// The reaction field `c` of `prob` (global interior array; UserFields::reaction).
// std::invalid_argument unless prob.reaction and `c` go together (both or
// neither), prob.shift == 0 with them ("add the constant to the field"), and
// every entry is finite and ≥ 0.  Every backend calls it before any work.
void check_reaction(const Problem& prob, const double* c, const char* who);
// The breakdown test every backend makes before α = g / den exists, den =
// h1·h2·(Ap, p), g = h1·h2·(z, r).  Step-size rule: the reference's absolute
// |den| < 1e-15 (stage2-mpi/poisson_mpi_decomp.cpp:413), bit for bit.  Residual
// rule: the same 1e-15 relative to g, |den| ≤ 1e-15·|g| (α beyond 1e15, or
// den = 0).  den is of the size of g (α = O(1) for the Jacobi-scaled
// operator), so the absolute form fires at g ≈ 1e-15 — before a threshold
// below sqrt(g) ≈ 3e-8 can be met, which in the D⁻¹ norm (z = r / D, D ≈ 4/h²)
// is where relative tolerances of 1e-6 lie: 2.2e-8 for F = 1 at 40×40.
PE_HD bool cg_breakdown(double den, double g, bool res_rule) {
  return res_rule ? fabs(den) <= 1e-15 * fabs(g) : fabs(den) < 1e-15;
}
// std::invalid_argument unless prob.stop is a rule, prob.atol is finite and ≥ 0,
// and a non-zero atol comes with Stop::Residual.  Every backend, before any work.
void check_stop(const Problem& prob, const char* who);
// The residual rule's threshold max(tol·sqrt(g0), atol) from g0 = h1·h2·(z⁰, r⁰)
// (one expression on every backend; a non-finite g0 gives NaN: never met).
inline double stop_threshold(const Problem& prob, double g0) {
  const double rel = prob.tol * std::sqrt(g0);
  return rel < prob.atol ? prob.atol : rel;
}
// out = B − A w, B = rhs (null: F) at nodes inside the ellipse, 0 elsewhere
// (assemble()'s mask).  Returns h1·h2·Σ out².  `out` may be null.
double residual_field(const Problem& prob, const double* w, const double* rhs, double* out, int threads = 1,
                      const double* reaction = nullptr);

}  // namespace pe
