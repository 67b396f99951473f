"""The user-field inputs of test_user_fields.py / test_user_fields_gpu.py and
their comparisons: a right-hand side and an initial guess that are asymmetric
in x and in y (the built-in problem is symmetric in both, so a transposed,
flipped or mis-offset field would pass with a symmetric input),

    rhs = 1 + x + y,    w0 = 0.05 sin(3x + 1) cos(2y − 0.5)  (non-zero outside the ellipse on purpose),

the exact solution of −Δu = rhs on the reference ellipse,
u = (1 − x² − 4y²)(1/10 + x/14 + y/26), the fp64 references (ops/torch_ref.py
with the same fields; computed once, never modified), the end-of-solve
figures recomputed in fp64 with the user B (the sibling of
norm_checks.fp64_norms) and the sweep comparison with both fields set (the
sibling of sweep_checks.check_sweeps, its KINDS bounds unchanged).

All fields are interior arrays, shape (M−1, N−1), entry [i−1, j−1] at (x_i, y_j)."""

import functools
import math

import norm_checks
import numpy as np
import pytest
import sweep_checks
import torch

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

# grid -> iterations to δ = 1e-6 (weighted norm) from w⁰ = 0 / from w0: the fp64 plain recurrence, every stop
# decision with ≥ 6 % margin (40×40: 1.124 / 0.940 δ and 1.570 / 0.893 δ; 26×27: 1.095 / 0.901 and 1.396 / 0.934)
COUNTS = {(40, 40): (69, 83), (26, 27): (48, 56)}


def _xy(prob):
    x = prob.A1 + np.arange(1, prob.M, dtype=np.float64) * prob.h1
    y = prob.A2 + np.arange(1, prob.N, dtype=np.float64) * prob.h2
    return x[:, None] + 0.0 * y[None, :], 0.0 * x[:, None] + y[None, :]


@functools.lru_cache(maxsize=None)
def _fields(M, N):
    prob = EllipseProblem(M, N)
    X, Y = _xy(prob)
    out = (1.0 + X + Y, 0.05 * np.sin(3.0 * X + 1.0) * np.cos(2.0 * Y - 0.5),
           (1.0 - X * X - 4.0 * Y * Y) * (0.1 + X / 14.0 + Y / 26.0))
    for a in out:
        a.setflags(write=False)
    return out


def rhs(M, N):
    return _fields(M, N)[0]


def w0(M, N):
    return _fields(M, N)[1]


def exact(M, N):
    return _fields(M, N)[2]


def inside(prob):
    X, Y = _xy(prob)
    return (prob.cx * X * X + prob.cy * Y * Y) < 1.0


def l2_exact(prob, w):
    """h-weighted L2 error in D of the interior array w against the exact u."""
    e = np.where(inside(prob), np.asarray(w) - exact(prob.M, prob.N), 0.0)
    return math.sqrt(float((e * e).sum()) * prob.h1 * prob.h2)


@functools.lru_cache(maxsize=None)
def torch_solve(M, N, warm):
    """torch_ref.pcg of the user problem to convergence, from 0 or from w0."""
    return torch_ref.pcg(EllipseProblem(M, N), rhs=rhs(M, N), w0=w0(M, N) if warm else None, keep_history=True)


@functools.lru_cache(maxsize=None)
def reference(kind, M, N, count):
    """The fp64 recurrence of `kind` with both fields after `count` sweeps."""
    fn = {"three": torch_ref.three_step, "two": torch_ref.two_step, "single": torch_ref.single_sweep}[kind]
    return fn(EllipseProblem(M, N), count, rhs=rhs(M, N), w0=w0(M, N))


def fp64_norms(prob, w, f):
    """‖B − A w‖_E and ‖B‖_E with the user B (f masked by the ellipse) and
    max |w| outside D, in fp64 on the CPU, of the interior array w."""
    M, N = prob.M, prob.N
    a, b, _ = norm_checks.assembled(prob)
    B = torch_ref.assemble(prob, rhs=f)[2]
    W = torch.zeros(M + 1, N + 1, dtype=torch.float64)
    W[1:M, 1:N] = torch.from_numpy(np.ascontiguousarray(w))
    hh = prob.h1 * prob.h2
    rho = (B - torch_ref.apply_A(W, a, b, prob.h1, prob.h2))[1:-1, 1:-1]
    wo = np.abs(np.asarray(w))[~inside(prob)]
    return dict(res_true=math.sqrt(float((rho * rho).sum()) * hh), b_norm=math.sqrt(float((B * B).sum()) * hh),
                max_outside=float(wo.max()) if wo.size else 0.0)


def check_norms(tag, prob, rep, f, three):
    """A report of a user-rhs solve on a single-sweep layout against fp64 from
    its own w: res_true and b_norm to norm_checks.resid_tol, max_outside to
    1e-12, no analytic error, and (three-step) the triangle inequality among
    kResid's sums.  Prints the deviations, then asserts."""
    ref = fp64_norms(prob, rep.w, f)
    tol = norm_checks.resid_tol(prob)
    got = {k: getattr(rep, k) for k in ref}
    dev = {k: abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] else abs(got[k]) for k in ref}
    print(f"field-norm-dev {tag} tol={tol:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items())
          + f" res_true={got['res_true']:.6e} b_norm={got['b_norm']:.6e}")
    assert rep.l2_err == -1.0 and rep.max_err == -1.0
    assert got["res_true"] == pytest.approx(ref["res_true"], rel=tol)
    assert got["b_norm"] == pytest.approx(ref["b_norm"], rel=tol)
    assert got["max_outside"] == pytest.approx(ref["max_outside"], rel=1e-12)
    if three:
        assert abs(rep.res_true - rep.res_rec) <= rep.res_gap * rep.res_rec * (1 + 1e-9)
    return dev


def solver(nat, M, N, algo, variant=0, fields=True, prob=None):
    """A single-rank solver (convergence test off) with both fields set; prob:
    another M×N problem than the reference one (a shift, a family member)."""
    opt = nat.SolveOptions()
    opt.algo = algo
    opt.variant = variant
    opt.check_tol = False
    blk = D.block(M, N, 1, 0)
    s = nat.DeviceSolver((prob or EllipseProblem(M, N)).to_native(), blk, None, opt)
    if fields:
        set_fields(nat, s, M, N, rhs(M, N), w0(M, N))
    return s


def set_fields(nat, s, M, N, f, g):
    fl, gl = nat.block_fields(M, N, s.block, f, g)
    s.set_rhs(fl)
    s.set_w0(gl)


def check_sweeps(s, M, N, kind, count):
    """sweep_checks.check_sweeps on a solver with both fields set, against
    the recurrence with the same fields; the KINDS bounds unchanged."""
    _, steps, nsums, s_rel, s_abs, ab_rel, f_tol = sweep_checks.KINDS[kind]
    assert s.sweep_steps == steps and s.user_rhs and s.user_w0
    s.reset()
    s.run_iterations(steps * count, False)
    s.synchronize()
    st = s.state()
    assert st["iter"] == steps * count and st["status"] == 0, (st["iter"], st["status"])
    ref = reference(kind, M, N, count)
    par = (count - 1) & 1
    got, want = st["fs" if steps == 1 else "fs2"][par], ref.sums[count]
    last = (lambda v: v[-1]) if steps == 1 else (lambda v: v[-1][steps - 1])
    fields = {"r": s.field(0 if par == 0 else 4)[2:M + 1, 2:N + 1], "p": s.field(2 if par == 0 else 3)[2:M + 1, 2:N + 1],
              "w": s.w()}
    dev = {}
    for name, f in fields.items():
        want_f = getattr(ref, name)[1:M, 1:N].numpy()
        dev[name] = float(np.abs(f - want_f).max() / np.abs(want_f).max())
    scale = max(abs(x) for x in want)
    dev["sums"] = max(abs(got[n] - want[n]) / max(abs(want[n]), s_abs / s_rel * scale) for n in range(nsums))
    dev["alpha"] = abs(st["alpha"] - last(ref.alpha)) / abs(last(ref.alpha))
    dev["beta"] = abs(st["beta"] - last(ref.beta)) / abs(last(ref.beta))
    print(f"field-sweep-dev {kind} {M}x{N} count={count} ti={s.ti} resident={int(s.resident)} "
          + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    for n in range(nsums):
        assert got[n] == pytest.approx(want[n], rel=s_rel, abs=s_abs * scale), n
    assert st["alpha"] == pytest.approx(last(ref.alpha), rel=ab_rel)
    assert st["beta"] == pytest.approx(last(ref.beta), rel=ab_rel)
    for name, f in fields.items():
        want_f = getattr(ref, name)[1:M, 1:N].numpy()
        np.testing.assert_allclose(f, want_f, rtol=0, atol=f_tol * np.abs(want_f).max(), err_msg=name)
    return dev
