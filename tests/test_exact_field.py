"""CPU tests of the user exact solution (solve(exact=), pe/fields.hpp): the
error a solve reports against it on the native CPU backends, the PyTorch
oracle, thread ranks and one process per rank, the tie to the built-in
analytic error, the refinement of a manufactured solution, the rules and
refusals, and the CLI's --exact.

Inputs: field_checks.rhs / w0 / exact (asymmetric in x and y; −Δ exact = rhs on
the reference ellipse).  The comparison (exact_checks.check_error): l2_err to
rel 1e-12 and max_err bit for bit against fp64 numpy from the report's own w.
Every test that passes `exact` fails without the feature: l2_err stays −1."""

import inspect
import json
import os
import subprocess
import sys

import exact_checks as xc
import field_checks as fc
import numpy as np
import pytest
import torch

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.solver import tensor_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SAME = ("iters", "last_diff", "converged", "init")
BACKENDS = [("serial", {}), ("omp", dict(threads=3)), ("torch", dict(device="cpu"))]


# ---- 1. serial, omp, torch ---------------------------------------------------------------------
@pytest.mark.parametrize("backend,kw", BACKENDS, ids=[b for b, _ in BACKENDS])
@pytest.mark.parametrize("M,N", sorted(fc.COUNTS))
def test_cpu_backends_with_exact(M, N, backend, kw):
    prob = EllipseProblem(M, N)
    f, g, u = fc.rhs(M, N), fc.w0(M, N), fc.exact(M, N)
    for warm in (False, True):
        base = solve(prob, backend=backend, rhs=f, w0=g if warm else None, return_w=True, **kw)
        rep = solve(prob, backend=backend, rhs=f, w0=g if warm else None, exact=u, return_w=True, **kw)
        tag = f"{backend} {M}x{N} {'w0' if warm else 'zero'}"
        assert base.l2_err == -1.0 and base.max_err == -1.0
        assert rep.converged and rep.iters == fc.COUNTS[(M, N)][warm], (tag, rep.iters)
        xc.same_solve(tag, rep, base, CPU_SAME)
        xc.check_error(tag, prob, rep, base=base)


# ---- 2. thread ranks and one process per rank ------------------------------------------------------
@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_thread_ranks_with_exact(M, N, ranks, decomp):
    """Every rank reads its nodes of the one global array; the sum and the max
    are reduced over ranks, so the one report is every rank's."""
    prob = EllipseProblem(M, N)
    kw = dict(backend="ranks", ranks=ranks, decomp=decomp, rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    base = solve(prob, **kw)
    rep = solve(prob, exact=fc.exact(M, N), **kw)
    assert f"{rep.Px}x{rep.Py}" == decomp and rep.converged
    if (M, N) in fc.COUNTS:
        assert rep.iters == fc.COUNTS[(M, N)][1]
    xc.same_solve(decomp, rep, base, CPU_SAME)
    xc.check_error(f"ranks {M}x{N} {decomp}", prob, rep, base=base)


def test_dist_cpu_with_exact(tmp_path):
    """Two processes over gloo, row slabs of 26×27 (13 + 12 rows): both ranks
    pass the same global arrays and report the same error; the comparison on
    the gathered w."""
    from conftest import free_port

    M, N = 26, 27
    paths = [str(tmp_path / n) for n in ("f.npy", "g.npy", "u.npy")]
    for p, a in zip(paths, (fc.rhs(M, N), fc.w0(M, N), fc.exact(M, N))):
        np.save(p, a)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "exact_field_job.py"),
           "dist-cpu", str(M), str(N), *paths, str(tmp_path / "out"), "2x1"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = []
    for r in range(2):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d.append(json.load(fh))
    assert d[0]["ranks"] == 2 and (d[0]["Px"], d[0]["Py"]) == (2, 1) and d[0]["converged"] and d[0]["iters"] == 56
    for k in ("l2_err", "max_err", "max_outside", "iters"):
        assert d[0][k] == d[1][k], k
    w = np.load(tmp_path / "out.r0.npy")
    l2, mx = xc.errors(EllipseProblem(M, N), w)
    print(f"exact-dev dist-cpu l2={d[0]['l2_err']:.6e} l2_rel={abs(d[0]['l2_err'] - l2) / l2:.2e} "
          f"max_diff={abs(d[0]['max_err'] - mx):.2e}")
    assert d[0]["l2_err"] == pytest.approx(l2, rel=xc.L2_REL) and d[0]["max_err"] == mx


# ---- 3. the tie to the built-in path ------------------------------------------------------------
@pytest.mark.parametrize("backend,kw", BACKENDS + [("ranks", dict(ranks=4, decomp="2x2"))],
                         ids=[b for b, _ in BACKENDS] + ["ranks"])
def test_analytic_array_is_the_builtin_error(backend, kw):
    """No rhs, exact = F (1 − x² − 4y²) / 10 built in numpy: the solve is the
    no-field solve, and the error the analytic one — max_err to 1e-15 absolute
    (|u| ≤ 0.1, ulp 1.4e-17; the host compiler may contract the analytic
    expression differently from numpy, a few ulp of u is the whole difference)."""
    M = N = 40
    prob = EllipseProblem(M, N)
    X, Y = fc._xy(prob)
    u = prob.F * (1.0 - X * X - 4.0 * Y * Y) / 10.0
    a = solve(prob, backend=backend, return_w=True, **kw)
    b = solve(prob, backend=backend, return_w=True, exact=u, **kw)
    print(f"exact-tie {backend} l2_rel={abs(a.l2_err - b.l2_err) / a.l2_err:.2e} "
          f"max_diff={abs(a.max_err - b.max_err):.2e}")
    assert a.iters == b.iters == 50 and np.array_equal(a.w, b.w)
    assert a.l2_err == pytest.approx(3.677e-3, rel=1e-3)
    assert b.l2_err == pytest.approx(a.l2_err, rel=1e-12)
    assert b.max_err == pytest.approx(a.max_err, rel=0, abs=1e-15)
    xc.check_error(f"tie {backend}", prob, b, u=u, base=a)


# ---- 4. refinement ------------------------------------------------------------------------------
def test_manufactured_solution_refines():
    """rhs = −Δ exact: the reported error is the discretisation error, and it
    falls with h.  The figures are torch_ref.pcg's in fp64 (69 iterations at
    40×40, 131 at 80×80); the backends agree on w to 1e-9, which carried
    through the norm is 9e-7 relative at 80×80 — the bound is ten times that."""
    want = {40: 4.027444e-3, 80: 1.834065e-3}
    got = {}
    for n in (40, 80):
        prob = EllipseProblem(n, n)
        rep = solve(prob, backend="serial", rhs=fc.rhs(n, n), exact=fc.exact(n, n))
        got[n] = rep.l2_err
        print(f"exact-refine {n}x{n} iters={rep.iters} l2={rep.l2_err:.6e} max={rep.max_err:.6e}")
        assert rep.converged and rep.l2_err == pytest.approx(want[n], rel=1e-5)
        assert rep.max_err > 0
    assert got[80] < got[40]


def test_torch_ref_reference_figure():
    """The 40×40 figure above is the oracle's own."""
    r = torch_ref.pcg(EllipseProblem(40, 40), rhs=fc.rhs(40, 40), exact=fc.exact(40, 40))
    assert r.iters == 69 and r.l2_err == pytest.approx(4.027444e-3, rel=1e-6)
    assert np.array_equal(r.w.numpy(), fc.torch_solve(40, 40, False).w.numpy())


# ---- 5. rules and refusals ----------------------------------------------------------------------
def test_none_keeps_todays_numbers():
    prob = EllipseProblem(26, 27)
    assert "exact" in inspect.signature(solve).parameters
    for backend, kw in BACKENDS:
        plain = solve(prob, backend=backend, **kw)
        none = solve(prob, backend=backend, exact=None, **kw)
        assert (none.l2_err, none.max_err, none.iters) == (plain.l2_err, plain.max_err, plain.iters)
        assert plain.l2_err > 0 and plain.max_err > 0
        user = solve(prob, backend=backend, rhs=fc.rhs(26, 27), exact=None, **kw)
        assert user.l2_err == -1.0 and user.max_err == -1.0
    r = torch_ref.pcg(prob, rhs=fc.rhs(26, 27), exact=None)
    assert r.l2_err == -1.0 and r.max_err == -1.0


def test_values_outside_the_ellipse_are_ignored():
    M, N = 26, 27
    prob = EllipseProblem(M, N)
    u = fc.exact(M, N)
    wild = np.where(fc.inside(prob), u, 1e30)
    for backend, kw in BACKENDS + [("ranks", dict(ranks=4, decomp="2x2"))]:
        a = solve(prob, backend=backend, rhs=fc.rhs(M, N), exact=u, **kw)
        b = solve(prob, backend=backend, rhs=fc.rhs(M, N), exact=wild, **kw)
        assert a.l2_err > 0 and (a.l2_err, a.max_err, a.max_outside) == (b.l2_err, b.max_err, b.max_outside), backend


@pytest.mark.parametrize("backend", ["serial", "ranks", "torch", "hip", "hip-group", "dist-cpu"])
def test_bad_exact_rejected(backend):
    """Refused before any solver, device or process group is touched."""
    prob = EllipseProblem(40, 40)
    good = fc.exact(40, 40)
    nan = good.copy()
    nan[3, 5] = np.nan
    big = np.full((39, 39), 2 ** 53 + 1, dtype=np.int64)  # not a float64
    for f in (good[:-1], good.T[:, :-1], nan, good.astype(complex), big):
        with pytest.raises(ValueError, match="exact"):
            solve(prob, backend=backend, ranks=2 if backend in ("ranks", "hip-group") else 1, exact=f)
    # float16 is no dtype of a tensor the device paths take (the host path widens any float loss-free)
    with pytest.raises(ValueError, match="exact"):
        tensor_spec("exact", torch.zeros(39, 39, dtype=torch.float16), prob)


# ---- 6. CLI -------------------------------------------------------------------------------------
def test_cli_exact(tmp_path):
    from poisson_ellipse_openmp_mpi_cuda_amd.utils.report import parse_legacy

    M, N = 26, 27
    f, u = str(tmp_path / "f.npy"), str(tmp_path / "u.npy")
    np.save(f, fc.rhs(M, N))
    np.save(u, fc.exact(M, N))
    base = [sys.executable, "-m", "poisson_ellipse_openmp_mpi_cuda_amd", "--backend", "serial", "--rhs", f]

    def run(extra):
        return subprocess.run(base + extra + [str(M), str(N)], cwd=ROOT, capture_output=True, text=True)

    api = solve(EllipseProblem(M, N), backend="serial", rhs=fc.rhs(M, N), exact=fc.exact(M, N))
    out = run(["--exact", u, "--json"])
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert parse_legacy(out.stdout)["iters"] == 48 and d["l2_err"] == api.l2_err and d["max_err"] == api.max_err
    assert f"L2 error in D ~ {api.l2_err:.6e} | max error in D ~ {api.max_err:.6e}" in out.stdout
    alone = run(["--json"])
    assert alone.returncode == 0 and "L2 error in D ~ n/a (user right-hand side)" in alone.stdout
    d0 = json.loads([ln for ln in alone.stdout.splitlines() if ln.startswith("{")][0])
    assert d0["l2_err"] == -1.0 and d0["max_err"] == -1.0
    assert set(d) == set(d0) and d["iters"] == d0["iters"] and d["max_outside"] == d0["max_outside"]  # no new fields
    missing = run(["--exact", str(tmp_path / "nothing.npy")])
    assert missing.returncode == 2 and "error:" in missing.stderr
    np.save(u, fc.exact(M, N)[:, :-1])
    shaped = run(["--exact", u])
    assert shaped.returncode == 2 and "--exact: expected the global interior" in shaped.stderr
    text = subprocess.run(base[:3] + ["--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    text = " ".join(text.split())  # (argparse wraps the help)
    assert "--exact" in text
