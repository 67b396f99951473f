"""The inputs, references and comparisons of test_shift.py / test_shift_gpu.py:
the shifted operator A + σI of EllipseProblem.shift (csrc/include/pe/fields.hpp),
(A + σI) w = B with the preconditioner D + σ.

Inputs are field_checks.w0 (operand, initial guess) and field_checks.rhs, as in
operator_checks; σ ∈ SIGMAS.  Shapes: the smallest at which the classic walk
(strips of 128 columns, 2 per lane; segments of 60 rows; items of 8 rows) can
go wrong.

Bounds (none taken from the code under test):
  fields    |got − ref| ≤ 1e-13·max|ref| against the host definition, and the
            sums of operator_checks.compare (abs 1e-12·h1·h2·Σ|v·(A_σ v)|, rel 1e-12);
  serial vs the torch recurrence: equal iterations, |w − w_ref| ≤ 1e-9 — the
            bound of the unshifted pair, tests/test_oracle.py:52;
  omp / ranks vs serial: equal iterations, |w − w_ref| ≤ 1e-9 — the bound
            tests/test_user_fields.py:104 holds the same backends to;
  hip vs serial: equal iterations, |w − w_ref| ≤ 1e-10 (test_gpu.py's
            classic-vs-CPU bound); l2_err / max_err to 1e-12 of numpy from the
            returned w (kError's bound); hip-group vs one rank: iterations ± 1,
            |w − w_ref| ≤ 1e-9.
A stop decision is only compared where it is no coin toss: stop_margin()
asserts |‖Δw‖ − δ| > 1e-3·δ at the stopping iteration and the one before it in
the serial history."""

import functools

import field_checks as fc
import numpy as np
import operator_checks as oc
import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, native, solve

SIGMAS = (0.75, 40.0)
STRETCHED_KW = oc.STRETCHED[1][2]  # cx = 0.25 in the box [-2, 2] × [-1, 1], here at 96 × 64
# (40, 40); ny = 129: a last strip of one column and an odd tail lane; ny = 128: exactly one full strip, nx = 69
# is nine items (at 8 rows per item no item reaches a second segment: test_classic_gpu.py forces the height for
# that); (65, 258); one stretched problem
SHAPES = [(40, 40, None), (9, 130, None), (70, 129, None), (65, 258, None), (96, 64, STRETCHED_KW)]
IDS = [f"{M}x{N}{'s' if kw else ''}" for M, N, kw in SHAPES]


def problem(M, N, kw=None, sigma=0.0, **more):
    return EllipseProblem(M, N, shift=sigma, **(kw or {}), **more)


def key(prob):
    return oc.key(prob) + (prob.shift,)


@functools.lru_cache(maxsize=None)
def _host(k, resid, user_rhs, f32):
    M, N = k[:2]
    prob = EllipseProblem(M, N, A1=k[2], B1=k[3], A2=k[4], B2=k[5], cx=k[6], cy=k[7], shift=k[8])
    v = oc.operand(M, N, f32)
    nat = native()
    if resid:
        s, f = nat.residual_field(prob.to_native(), v, fc.rhs(M, N) if user_rhs else None)
    else:
        s, f = nat.apply_operator(prob.to_native(), v)
    f = np.asarray(f)
    f.setflags(write=False)
    return f, float(s)


def host(prob, resid=False, user_rhs=False, f32=False):
    """(field, sum) of the host definition with prob.shift for the operand of this grid; computed once, read-only."""
    return _host(key(prob), bool(resid), bool(user_rhs), bool(f32))


def compare(tag, prob, field, total, resid=False, user_rhs=False, f32=False):
    """operator_checks.compare with the shift: a result against the host
    definition of A + σI at its bounds.  Prints the deviation and whether the
    bits are the host's, then asserts."""
    ref_f, ref_s = host(prob, resid, user_rhs, f32)
    if field is not None:
        field = np.asarray(field)
        assert field.shape == ref_f.shape and field.dtype == np.float64, (tag, field.shape, field.dtype)
        dev = float(np.abs(field - ref_f).max() / np.abs(ref_f).max())
        print(f"shift-operator-dev {tag} shift={prob.shift} {'resid' if resid else 'apply'} field={dev:.2e} "
              f"bitwise={np.array_equal(field, ref_f)} sum={total!r} host={ref_s!r}")
        assert dev <= 1e-13, (tag, dev)
    if resid:
        assert total == pytest.approx(ref_s, rel=1e-12), (tag, total, ref_s)
    else:
        scale = prob.h1 * prob.h2 * float(np.abs(oc.operand(prob.M, prob.N, f32) * ref_f).sum())
        assert abs(total - ref_s) <= 1e-12 * scale, (tag, total, ref_s)


def masked_rhs(prob, f=None):
    """B in numpy: f (None: F) inside the ellipse, 0 elsewhere — assemble()'s mask with its own products."""
    return np.where(fc.inside(prob), prob.F if f is None else f, 0.0)


@functools.lru_cache(maxsize=None)
def _serial(k, tol, max_iter, fields):
    M, N = k[:2]
    prob = EllipseProblem(M, N, A1=k[2], B1=k[3], A2=k[4], B2=k[5], cx=k[6], cy=k[7], shift=k[8], tol=tol,
                          max_iter=max_iter)
    kw = dict(rhs=fc.rhs(M, N), w0=fc.w0(M, N)) if fields else {}
    rep = solve(prob, backend="serial", return_w=True, keep_history=True, **kw)
    rep.w.setflags(write=False)
    return rep


def serial(prob, fields=True):
    """The serial solve of prob (with field_checks' rhs and w0), history kept; computed once, read-only."""
    return _serial(key(prob), prob.tol, prob.max_iter, bool(fields))


def stop_margin(prob, fields=True):
    """Asserts that the serial solve's stop test is no coin toss, and returns the solve."""
    ref = serial(prob, fields)
    assert ref.converged and len(ref.history) == ref.iters >= 2
    for d in ref.history[-2:]:
        assert abs(d - prob.tol) > 1e-3 * prob.tol, (prob.M, prob.N, prob.shift, ref.history[-2:])
    assert ref.history[-1] < prob.tol <= ref.history[-2]
    return ref


def errors_from_w(prob, w, u):
    """l2_err / max_err recomputed in numpy from an interior w against the exact field u, inside the ellipse."""
    e = np.where(fc.inside(prob), np.asarray(w) - u, 0.0)
    return float(np.sqrt(float((e * e).sum()) * prob.h1 * prob.h2)), float(np.abs(e).max())
