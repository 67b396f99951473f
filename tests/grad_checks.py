"""The gradient of a solution and its functionals in fp64 numpy — the one
definition (csrc/include/pe/fields.hpp) every backend must reproduce — and the
one comparison of test_gradient.py / test_gradient_gpu.py.

Nodes are the global interior i = 1..M−1, j = 1..N−1, x_i = A1 + i·h1,
y_j = A2 + j·h2, in(i, j) = (cx·x·x + cy·y·y) < 1.0 and false on the box
boundary.  At a node with in(i, j)

    gx = (w[i+1,j] − w[i−1,j]) / (2.0·h1)   both x neighbours inside (class 3)
         (w[i+1,j] − w[i,j]) / h1           only i+1 inside          (class 2)
         (w[i,j] − w[i−1,j]) / h1           only i−1 inside          (class 1)
         0.0                                neither                  (class 0)

and gy alike in j with h2; outside the ellipse gx = gy = 0.0 whatever w is.

    integral = h1·h2·Σ_D w,  energy = h1·h2·Σ_D (gx² + gy²),  grad_max = sqrt(max_D (gx² + gy²)).

The comparison, from the report's own w: gx and gy bit for bit (one
subtraction and one true division per component, no contraction on any
backend), grad_max equal (a maximum has no order, one correctly rounded square
root), energy to rel 1e-12 (a sum of at most ~4 000 non-negative terms at the
shapes used, n·2⁻⁵³ < 5e-13: the project's bound for l2_err), integral to abs
1e-12·h1·h2·Σ_D|w| (its terms have mixed signs far from convergence)."""

import math

import numpy as np
import pytest

ENERGY_REL = 1e-12
INTEGRAL_REL = 1e-12
SOLVE_SAME = ("iters", "last_diff", "converged", "res_true", "res_rec", "b_norm", "max_outside", "algo", "init",
              "l2_err", "max_err")


def host(a):
    """An array of a report as numpy (a GPU tensor is copied)."""
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def inside_full(prob):
    """in(i, j) over i = 0..M, j = 0..N, false on the box boundary."""
    x = prob.A1 + np.arange(0, prob.M + 1, dtype=np.float64) * prob.h1
    y = prob.A2 + np.arange(0, prob.N + 1, dtype=np.float64) * prob.h2
    X, Y = x[:, None], y[None, :]
    m = (prob.cx * X * X + prob.cy * Y * Y) < 1.0
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    return m


def classes(prob):
    """(cx, cy): the difference class of every interior node in x and in y —
    0 neither, 1 only the lower, 2 only the upper, 3 both neighbours inside;
    −1 outside the ellipse."""
    m = inside_full(prob)
    c = m[1:-1, 1:-1]
    cx = np.where(c, m[:-2, 1:-1] * 1 + m[2:, 1:-1] * 2, -1)
    cy = np.where(c, m[1:-1, :-2] * 1 + m[1:-1, 2:] * 2, -1)
    return cx, cy


def class_counts(prob):
    """{(direction, class): nodes}, classes 0..3 in "x" and "y"."""
    cx, cy = classes(prob)
    return {(d, k): int((c == k).sum()) for d, c in (("x", cx), ("y", cy)) for k in range(4)}


def gradient(prob, w):
    """(g, integral, energy, grad_max) of the interior array w, g of shape (2, M−1, N−1)."""
    w = np.asarray(w, dtype=np.float64)
    M, N = prob.M, prob.N
    assert w.shape == (M - 1, N - 1)
    W = np.zeros((M + 1, N + 1))
    W[1:M, 1:N] = w
    cx, cy = classes(prob)
    c = W[1:-1, 1:-1]

    def diff(lo, hi, cls, h):
        with np.errstate(all="ignore"):
            both, up, dn = (hi - lo) / (2.0 * h), (hi - c) / h, (c - lo) / h
        return np.where(cls == 3, both, np.where(cls == 2, up, np.where(cls == 1, dn, 0.0)))

    gx = diff(W[:-2, 1:-1], W[2:, 1:-1], cx, prob.h1)
    gy = diff(W[1:-1, :-2], W[1:-1, 2:], cy, prob.h2)
    g2 = gx * gx + gy * gy
    hh = prob.h1 * prob.h2
    ins = cx >= 0
    return (np.stack((gx, gy)), hh * float(w[ins].sum()), hh * float(g2[ins].sum()),
            math.sqrt(float(g2[ins].max())) if ins.any() else 0.0)


def random_w(prob, seed=7):
    """A seeded random interior array, non-zero outside the ellipse too."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (prob.M - 1, prob.N - 1))


def check_values(tag, prob, w, g, integral, energy, grad_max):
    """g and the three figures against gradient(prob, w).  Prints the deviations, then asserts."""
    w = host(w)
    ref, ri, re, rm = gradient(prob, w)
    g = host(g)
    ins = classes(prob)[0] >= 0
    scale = prob.h1 * prob.h2 * float(np.abs(w[ins]).sum())
    print(f"grad-dev {tag} field_diff={float(np.abs(g - ref).max()):.2e} max_diff={abs(grad_max - rm):.2e} "
          f"energy_rel={abs(energy - re) / re if re else abs(energy):.2e} "
          f"integral_abs={abs(integral - ri):.2e} (bound {INTEGRAL_REL * scale:.2e}) grad_max={grad_max:.6e}")
    assert g.shape == ref.shape and g.dtype == np.float64, tag
    assert np.array_equal(g[0], ref[0]), tag
    assert np.array_equal(g[1], ref[1]), tag
    assert grad_max == rm, tag
    assert energy == pytest.approx(re, rel=ENERGY_REL), tag
    assert abs(integral - ri) <= INTEGRAL_REL * scale, tag


def check_stats(tag, prob, w, integral, energy, grad_max):
    """The three figures alone (return_grad="stats") against gradient(prob, w)."""
    w = host(w)
    _, ri, re, rm = gradient(prob, w)
    ins = classes(prob)[0] >= 0
    assert grad_max == rm, tag
    assert energy == pytest.approx(re, rel=ENERGY_REL), tag
    assert abs(integral - ri) <= INTEGRAL_REL * prob.h1 * prob.h2 * float(np.abs(w[ins]).sum()), tag


def check_report(tag, prob, rep, w=None, g=None):
    """A report with return_grad=True / "device" against its own w (or the
    assembled w and gradient of a multi-process job)."""
    check_values(tag, prob, rep.w if w is None else w, rep.grad if g is None else g, rep.integral, rep.energy,
                 rep.grad_max)


def same_solve(tag, rep, base):
    """return_grad never influences the solve: exact_checks.same_solve (every
    figure and w bit for bit), the errors as well, and the base carries nothing."""
    import exact_checks

    exact_checks.same_solve(tag, rep, base, keys=SOLVE_SAME)
    assert base.grad is None and (base.integral, base.energy, base.grad_max) == (-1.0, -1.0, -1.0), tag
