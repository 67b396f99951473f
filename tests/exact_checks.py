"""The one comparison of test_exact_field.py / test_exact_field_gpu.py: the
error a report carries against a user exact solution, recomputed in fp64 numpy
from the report's own w over field_checks.inside(prob),

    l2_err  = sqrt(h1 h2 Σ_D (w − u)²)   to rel 1e-12 (test_residual.py's bound on kError: the shapes used have
                                          ≤ ~4 200 inside nodes, and a reordered sum of non-negative terms stays
                                          below n · 2⁻⁵³ ≈ 5e-13),
    max_err = max_D |w − u|              bit for bit (one subtraction and one fabs per node; a max has no order),

and max_outside equal to that of the same call without `exact`.  u defaults to
field_checks.exact (then l2 is field_checks.l2_exact itself)."""

import math

import field_checks as fc
import numpy as np
import pytest

L2_REL = 1e-12
SOLVE_SAME = ("iters", "last_diff", "converged", "res_true", "res_rec", "b_norm", "max_outside", "algo", "init")


def host(w):
    """w of a report as a numpy array (a GPU tensor is copied)."""
    return w.cpu().numpy() if hasattr(w, "cpu") else np.asarray(w)


def errors(prob, w, u=None):
    """(l2, max) of the interior array w against u inside the ellipse, fp64."""
    if u is None:
        u = fc.exact(prob.M, prob.N)
        l2 = fc.l2_exact(prob, w)
    else:
        e = np.where(fc.inside(prob), np.asarray(w) - u, 0.0)
        l2 = math.sqrt(float((e * e).sum()) * prob.h1 * prob.h2)
    return l2, float(np.abs(np.asarray(w) - u)[fc.inside(prob)].max())


def check_error(tag, prob, rep, u=None, base=None, w=None):
    """rep.l2_err / rep.max_err against errors() of rep.w (or of `w`: the
    assembled array of a multi-process job); base: the report of the same call
    without `exact`.  Prints the deviations, then asserts."""
    l2, mx = errors(prob, host(rep.w) if w is None else w, u)
    print(f"exact-dev {tag} l2={rep.l2_err:.6e} l2_rel={abs(rep.l2_err - l2) / l2:.2e} max={rep.max_err:.6e} "
          f"max_diff={abs(rep.max_err - mx):.2e}"
          + ("" if base is None else f" outside_diff={abs(rep.max_outside - base.max_outside):.2e}"))
    assert l2 > 0 and rep.l2_err == pytest.approx(l2, rel=L2_REL), tag
    assert rep.max_err == mx, tag
    if base is not None:
        assert rep.max_outside == base.max_outside, tag


def same_solve(tag, rep, base, keys=SOLVE_SAME):
    """`exact` never influences the solve: every figure but the error, and w, bit for bit."""
    for k in keys:
        assert getattr(rep, k) == getattr(base, k), (tag, k, getattr(rep, k), getattr(base, k))
    assert np.array_equal(host(rep.w), host(base.w)), tag
