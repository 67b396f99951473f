"""The inputs and the one comparison of test_operator.py / test_operator_gpu.py:
A v and B − A w of a field of the caller's against the host definition
(native.apply_operator / native.residual_field, csrc/include/pe/fields.hpp).

Inputs are field_checks.w0 (the operand) and field_checks.rhs (the right-hand
side): asymmetric in x and y, non-zero outside the ellipse and next to the box.

Bounds.  Fields: |got − ref| ≤ 1e-13·max|ref|, the bound
test_gpu.test_device_operator_vs_torch_oracle holds the same expression tree
to.  Sums: h1·h2·Σ v·(A v) to abs 1e-12·h1·h2·Σ|v·(A v)| (a sum of terms of both
signs, reordered), h1·h2·Σ (B − A w)² to rel 1e-12 (positive terms)."""

import functools

import field_checks as fc
import numpy as np
import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, native

# the two stretched problems of test_gpu.test_device_operator_vs_torch_oracle: the circle in the square, cx = 0.25
STRETCHED = [(512, 512, dict(A2=-1.0, B2=1.0, cy=1.0)),
             (300, 200, dict(A1=-2.0, B1=2.0, A2=-1.0, B2=1.0, cx=0.25, cy=1.0))]


def problem(M, N, kw=None):
    return EllipseProblem(M, N, **(kw or {}))


def key(prob):
    return (prob.M, prob.N, prob.A1, prob.B1, prob.A2, prob.B2, prob.cx, prob.cy)


@functools.lru_cache(maxsize=None)
def _host(k, resid, user_rhs, f32):
    M, N = k[:2]
    prob = EllipseProblem(M, N, A1=k[2], B1=k[3], A2=k[4], B2=k[5], cx=k[6], cy=k[7])
    v = operand(M, N, f32)
    nat = native()
    if resid:
        s, f = nat.residual_field(prob.to_native(), v, fc.rhs(M, N) if user_rhs else None)
    else:
        s, f = nat.apply_operator(prob.to_native(), v)
    f = np.asarray(f)
    f.setflags(write=False)
    return f, float(s)


def operand(M, N, f32=False):
    """field_checks.w0, or its float32 rounding widened back (what a float32 tensor holds)."""
    v = fc.w0(M, N)
    return v.astype(np.float32).astype(np.float64) if f32 else v


def host(prob, resid=False, user_rhs=False, f32=False):
    """(field, sum) of the host definition for the operand of this grid; computed once, read-only."""
    return _host(key(prob), bool(resid), bool(user_rhs), bool(f32))


def sum_ok(prob, got, resid, user_rhs=False, f32=False):
    ref_f, ref_s = host(prob, resid, user_rhs, f32)
    if resid:
        return got == pytest.approx(ref_s, rel=1e-12)
    scale = prob.h1 * prob.h2 * float(np.abs(operand(prob.M, prob.N, f32) * ref_f).sum())
    return abs(got - ref_s) <= 1e-12 * scale


def compare(tag, prob, field, total, resid=False, user_rhs=False, f32=False):
    """A device (or backend) result against the host definition.  Prints the
    deviation and whether the bits are the host's, then asserts the bounds."""
    ref_f, ref_s = host(prob, resid, user_rhs, f32)
    if field is not None:
        field = np.asarray(field)
        assert field.shape == ref_f.shape and field.dtype == np.float64, (tag, field.shape, field.dtype)
        dev = float(np.abs(field - ref_f).max() / np.abs(ref_f).max())
        print(f"operator-dev {tag} {'resid' if resid else 'apply'} field={dev:.2e} bitwise={np.array_equal(field, ref_f)} "
              f"sum={total!r} host={ref_s!r}")
        assert dev <= 1e-13, (tag, dev)
    assert sum_ok(prob, total, resid, user_rhs, f32), (tag, total, ref_s)
