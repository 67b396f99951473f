"""CPU tests of the shifted operator A + σI (EllipseProblem.shift; −Δu + σu = f):
the definition on the host and in the torch oracle, the CPU solves against the
torch recurrence and against each other, the refusals, the CLI.  Inputs, shapes
and bounds: shift_checks.  Every test fails without the feature
(EllipseProblem has no `shift`)."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import operator_checks as oc
import pytest
import shift_checks as sc

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, apply_operator, residual, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BACKENDS = [("serial", {}), ("omp", dict(threads=3)), ("ranks", dict(ranks=4, decomp="2x2")),
                ("ranks", dict(ranks=3, decomp="3x1"))]


# ---- 1. the definition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("M,N,kw", sc.SHAPES, ids=sc.IDS)
def test_host_definition_is_the_unshifted_tree_plus_sigma_v(nat, M, N, kw, sigma):
    """A_σ v = (A v) + σ·v and B − A_σ w with the same tree, no contraction: the bits of numpy."""
    prob, base = sc.problem(M, N, kw, sigma), sc.problem(M, N, kw)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    hh = prob.h1 * prob.h2
    for threads in (1, 3):
        s0, a0 = nat.apply_operator(base.to_native(), v, True, threads)
        s, a = nat.apply_operator(prob.to_native(), v, True, threads)
        want = np.asarray(a0) + sigma * v
        assert np.array_equal(np.asarray(a), want)
        assert abs(s - hh * float((v * want).sum())) <= 1e-12 * hh * float(np.abs(v * want).sum()) and s > s0
        only, none = nat.apply_operator(prob.to_native(), v, False, threads)
        assert none is None and only == s
        for rhs in (None, f):
            rs, r = nat.residual_field(prob.to_native(), v, rhs, True, threads)
            rwant = sc.masked_rhs(prob, rhs) - want
            assert np.array_equal(np.asarray(r), rwant)
            assert rs == pytest.approx(hh * float((rwant * rwant).sum()), rel=1e-12)


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("M,N,kw", sc.SHAPES, ids=sc.IDS)
def test_torch_oracle_against_the_host(M, N, kw, sigma):
    prob = sc.problem(M, N, kw, sigma)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    a, b, _ = torch_ref.assemble(prob)
    V = torch_ref.embed(prob, v)
    Av = torch_ref.apply_A(V, a, b, prob.h1, prob.h2, prob.shift)[1:-1, 1:-1]
    sc.compare("torch", prob, Av.numpy(), prob.h1 * prob.h2 * float((V[1:-1, 1:-1] * Av).sum()))
    for user in (False, True):
        r = torch_ref.residual(prob, v, f if user else None)[1:-1, 1:-1]
        sc.compare("torch", prob, r.numpy(), prob.h1 * prob.h2 * float((r * r).sum()), True, user)
    # the public entry points, every CPU backend and the torch backend
    for backend, bkw in CPU_BACKENDS[:2] + [("torch", dict(device="cpu"))]:
        res = apply_operator(prob, v, backend=backend, **bkw)
        sc.compare(backend, prob, res.field, res.sum)
        res = residual(prob, v, rhs=f, backend=backend, **bkw)
        sc.compare(backend, prob, res.field, res.sum, True, True)


@pytest.mark.parametrize("backend,kw", CPU_BACKENDS + [("torch", dict(device="cpu"))])
def test_explicit_zero_shift_is_the_default(backend, kw):
    M = N = 40
    a = solve(EllipseProblem(M, N), backend=backend, return_w=True, rhs=fc.rhs(M, N), w0=fc.w0(M, N), **kw)
    b = solve(EllipseProblem(M, N, shift=0.0), backend=backend, return_w=True, rhs=fc.rhs(M, N), w0=fc.w0(M, N), **kw)
    assert a.iters == b.iters == fc.COUNTS[(M, N)][1] and np.array_equal(a.w, b.w) and a.last_diff == b.last_diff
    c, d = solve(EllipseProblem(M, N), backend=backend, **kw), solve(EllipseProblem(M, N, shift=0.0), backend=backend, **kw)
    assert c.iters == d.iters == 50 and c.l2_err == d.l2_err > 0 and "shift" not in d.to_dict()
    if backend != "torch":
        x = apply_operator(EllipseProblem(M, N), fc.w0(M, N), backend=backend, **kw)
        y = apply_operator(EllipseProblem(M, N, shift=0.0), fc.w0(M, N), backend=backend, **kw)
        assert np.array_equal(x.field, y.field) and x.sum == y.sum
        assert np.array_equal(x.field, oc.host(EllipseProblem(M, N))[0])


# ---- 2. CPU solves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("M,N,kw", sc.SHAPES, ids=sc.IDS)
def test_serial_against_the_torch_recurrence(M, N, kw, sigma):
    prob = sc.problem(M, N, kw, sigma)
    ref = sc.stop_margin(prob)
    t = torch_ref.pcg(prob, rhs=fc.rhs(M, N), w0=fc.w0(M, N), keep_history=True)
    print(f"shift-serial {M}x{N} shift={sigma} iters={ref.iters} torch={t.iters} "
          f"dw={np.abs(t.w[1:-1, 1:-1].numpy() - ref.w).max():.2e} last={ref.history[-2:]}")
    assert t.converged and t.iters == ref.iters
    np.testing.assert_allclose(t.w[1:-1, 1:-1].numpy(), ref.w, rtol=0, atol=1e-9)  # (tests/test_oracle.py:52)
    assert ref.l2_err == -1.0 and ref.max_err == -1.0 and t.l2_err == -1.0
    # the shift is in the system: the iterate is closer to solving (A + σI) w = B than A w = B
    assert (residual(prob, ref.w, rhs=fc.rhs(M, N), backend="serial").sum
            < residual(sc.problem(M, N, kw), ref.w, rhs=fc.rhs(M, N), backend="serial").sum)


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("backend,kw", CPU_BACKENDS[1:])
@pytest.mark.parametrize("M,N", [(40, 40), (37, 50)])
def test_cpu_backends_against_serial(M, N, backend, kw, sigma):
    prob = sc.problem(M, N, None, sigma)
    ref = sc.stop_margin(prob)
    rep = solve(prob, backend=backend, rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True, **kw)
    print(f"shift-cpu {backend} {kw} {M}x{N} shift={sigma} iters={rep.iters}/{ref.iters} dw={np.abs(rep.w - ref.w).max():.2e}")
    assert rep.converged and rep.iters == ref.iters and rep.l2_err == -1.0 and rep.max_err == -1.0
    np.testing.assert_allclose(rep.w, ref.w, rtol=0, atol=1e-9)  # (tests/test_user_fields.py:104)


def test_builtin_rhs_exact_and_iteration_cap():
    """The built-in F with a shift: no analytic error (−1) unless `exact` is given; max_iter caps as ever."""
    M, N, sigma = 40, 40, 40.0
    prob = sc.problem(M, N, None, sigma)
    sc.stop_margin(prob, fields=False)
    plain = solve(prob, backend="serial", return_w=True)
    assert plain.converged and plain.l2_err == -1.0 and plain.max_err == -1.0 and plain.max_outside >= 0
    assert plain.to_dict()["shift"] == sigma
    with_u = solve(prob, backend="serial", return_w=True, exact=fc.exact(M, N))
    l2, mx = sc.errors_from_w(prob, with_u.w, fc.exact(M, N))
    assert np.array_equal(with_u.w, plain.w) and with_u.iters == plain.iters
    assert with_u.l2_err == pytest.approx(l2, rel=1e-12) and with_u.max_err == pytest.approx(mx, rel=1e-12)
    capped = solve(sc.problem(M, N, None, sigma, max_iter=7), backend="omp", threads=3, return_w=True)
    assert capped.iters == 7 and not capped.converged


# ---- 6. refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -1e-300])
def test_bad_shift_is_refused_on_every_backend(nat, bad):
    prob = EllipseProblem(40, 40, shift=bad)
    v = fc.w0(40, 40)
    for backend, kw in CPU_BACKENDS + [("torch", dict(device="cpu")), ("dist-cpu", {}), ("hip", {}),
                                       ("hip-group", dict(ranks=2))]:
        with pytest.raises(ValueError, match="shift"):
            solve(prob, backend=backend, **kw)
        with pytest.raises(ValueError, match="shift"):
            apply_operator(prob, v, backend=backend, **kw)
        with pytest.raises(ValueError, match="shift"):
            residual(prob, v, backend=backend, **kw)
    with pytest.raises(ValueError, match="shift"):
        torch_ref.pcg(prob)
    # the native layer refuses on its own (a Problem filled in by hand)
    P = EllipseProblem(40, 40).to_native()
    P.shift = bad
    with pytest.raises(ValueError, match="shift"):
        nat.apply_operator(P, v, True, 1)
    with pytest.raises(ValueError, match="shift"):
        nat.residual_field(P, v, None, True, 1)
    from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D
    from poisson_ellipse_openmp_mpi_cuda_amd.solver import _options

    for ranks in (1, 4):
        with pytest.raises(ValueError, match="shift"):
            nat.cpu_solve_grid(P, D.grid(ranks, 40, 40, "2x2" if ranks == 4 else "reference"), _options(), False, None,
                               None, None)


def test_problem_carries_the_shift():
    p = EllipseProblem(40, 40, shift=2.5)
    assert EllipseProblem().shift == 0.0 and p.with_grid(26, 27).shift == 2.5
    assert p.to_native().shift == 2.5 and EllipseProblem().to_native().shift == 0.0


# ---- the command lines ----------------------------------------------------------------------------------------------
def _run(cmd):
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    return out.returncode, out.stdout, out.stderr


def test_cli_shift(tmp_path):
    py = [sys.executable, "-m", "poisson_ellipse_openmp_mpi_cuda_amd.cli", "--backend", "serial"]
    code, out, err = _run(py + ["--shift", "40", "--json", "--dump", str(tmp_path / "w.npy"), "40", "40"])
    assert code == 0, err
    ref = sc.serial(sc.problem(40, 40, None, 40.0), fields=False)
    assert f"Iter={ref.iters} " in out and "L2 error in D ~ n/a (shifted operator)" in out
    d = json.loads(out.strip().splitlines()[-1])
    assert d["shift"] == 40.0 and d["iters"] == ref.iters and d["l2_err"] == -1.0
    assert np.array_equal(np.load(tmp_path / "w.npy"), ref.w)
    code, out, err = _run(py + ["--json", "40", "40"])  # at zero: no "shift" key, the error line as ever
    assert code == 0 and "shift" not in out and "n/a" not in out and "Iter=50 " in out
    code, out, err = _run(py + ["--shift", "-1", "40", "40"])
    assert code == 2 and "shift" in err and out == ""
    exe = os.path.join(ROOT, "bin", "pe_cpu")
    code, out, err = _run([exe, "--shift", "40", "--json", "40", "40"])
    assert code == 0 and json.loads(out)["shift"] == 40.0 and json.loads(out)["iters"] == ref.iters
    code, out, err = _run([exe, "--shift", "40", "40", "40"])
    assert code == 0 and f"Iter={ref.iters} " in out and "L2 error in D ~ n/a (shifted operator)" in out
    code, out, err = _run([exe, "--json", "40", "40"])
    assert code == 0 and "shift" not in out and json.loads(out)["iters"] == 50
    code, out, err = _run([exe, "--shift", "nan", "40", "40"])
    assert code == 2 and "shift" in err
