"""CPU tests of the user right-hand side and initial guess (solve(rhs=, w0=),
pe/fields.hpp): the slicing helper every backend shares, the CPU backends and
the PyTorch oracle on the asymmetric inputs of field_checks.py, the input
checks, and the CLI's --dump → --w0 round trip.

The iteration counts (field_checks.COUNTS) are equalities: every stop decision
of these solves has ≥ 6 % margin against a rounding of ~1e-9."""

import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# backend keywords of the native CPU solves: serial, OpenMP, thread-ranks
BACKENDS_40 = [("serial", {}), ("omp", dict(threads=3)), ("ranks", dict(ranks=4, decomp="2x2")),
               ("ranks", dict(ranks=3, decomp="3x1"))]
BACKENDS_26 = BACKENDS_40 + [("ranks", dict(ranks=3, decomp="1x3"))]  # 26×27: 25 rows, 26 columns — remainders
CASES = [(40, 40, b, kw) for b, kw in BACKENDS_40] + [(26, 27, b, kw) for b, kw in BACKENDS_26]


def _id(c):
    M, N, b, kw = c
    return f"{M}x{N}-{b}-{kw.get('decomp', kw.get('threads', 1))}"


# ---- the oracle ------------------------------------------------------------------
def test_torch_defaults_unchanged():
    """rhs=None, w0=None is today's path: the same bits as no keyword, the
    golden count and L2 error of 40×40, and — the user path on the built-in
    problem — the same bits again from an F-filled rhs and a zero w0."""
    prob = EllipseProblem(40, 40)
    F, Z = np.full((39, 39), prob.F), np.zeros((39, 39))
    a = torch_ref.pcg(prob)
    b = torch_ref.pcg(prob, rhs=None, w0=None)
    c = torch_ref.pcg(prob, rhs=F, w0=Z)
    assert a.iters == b.iters == c.iters == 50 and a.l2_err == b.l2_err == pytest.approx(3.677e-3, rel=1e-3)
    assert np.array_equal(a.w.numpy(), b.w.numpy()) and np.array_equal(a.w.numpy(), c.w.numpy())
    assert c.l2_err == -1.0 and c.max_err == -1.0
    for fn, n in ((torch_ref.single_sweep, 12), (torch_ref.two_step, 6), (torch_ref.three_step, 4)):
        x, y, z = fn(prob, n), fn(prob, n, rhs=None, w0=None), fn(prob, n, rhs=F, w0=Z)
        for name in ("r", "p", "w"):
            assert np.array_equal(getattr(x, name).numpy(), getattr(y, name).numpy()), (fn.__name__, name)
            assert np.array_equal(getattr(x, name).numpy(), getattr(z, name).numpy()), (fn.__name__, name)
        assert x.sums == y.sums == z.sums and x.alpha == y.alpha == z.alpha
    for u, v in zip(torch_ref.assemble(prob), torch_ref.assemble(prob, rhs=None)):
        assert np.array_equal(u.numpy(), v.numpy())


@pytest.mark.parametrize("M,N", sorted(fc.COUNTS))
def test_torch_counts_and_margins(M, N):
    """The reference figures are re-derived, not copied: the counts, and that
    each stop decision (‖Δw‖ at k−1 and at k) is ≥ 6 % away from δ."""
    prob = EllipseProblem(M, N)
    for warm in (False, True):
        r = fc.torch_solve(M, N, warm)
        assert r.converged and r.iters == fc.COUNTS[(M, N)][warm]
        assert r.history[-2] >= 1.06 * prob.tol and r.history[-1] <= 0.94 * prob.tol, r.history[-2:]
    if (M, N) == (40, 40):  # the discretisation error against the exact u (F = 1 at this grid: 3.68e-3)
        assert fc.l2_exact(prob, fc.torch_solve(M, N, False).w[1:-1, 1:-1].numpy()) == pytest.approx(4.027e-3, rel=1e-3)


def test_torch_recurrences_agree_with_fields():
    """The sweep recurrences with both fields follow the plain loop."""
    M, N, K = 40, 40, 12
    prob = EllipseProblem(M, N)
    ref = torch_ref.pcg(prob, rhs=fc.rhs(M, N), w0=fc.w0(M, N), max_iter=K)
    scale = float(ref.w.abs().max())
    for kind, n in (("single", K), ("two", K // 2), ("three", K // 3)):
        got = fc.reference(kind, M, N, n)
        assert float((got.w - ref.w).abs().max()) <= 1e-11 * scale, kind


# ---- the native CPU backends ---------------------------------------------------------
@pytest.mark.parametrize("backend,kw", [("serial", {}), ("ranks", dict(ranks=4, decomp="2x2"))])
def test_constant_rhs_is_the_builtin_path(backend, kw):
    prob = EllipseProblem(40, 40)
    a = solve(prob, backend=backend, return_w=True, **kw)
    b = solve(prob, backend=backend, return_w=True, rhs=np.full((39, 39), prob.F), **kw)
    assert a.iters == b.iters == 50 and np.array_equal(a.w, b.w)
    assert b.l2_err == -1.0 and b.max_err == -1.0 and b.max_outside == a.max_outside


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cpu_backends_with_fields(case):
    M, N, backend, kw = case
    prob = EllipseProblem(M, N)
    f, g = fc.rhs(M, N), fc.w0(M, N)
    for warm in (False, True):
        ref = fc.torch_solve(M, N, warm)
        rep = solve(prob, backend=backend, rhs=f, w0=g if warm else None, return_w=True, **kw)
        assert rep.converged and rep.iters == fc.COUNTS[(M, N)][warm] == ref.iters
        assert rep.init == ("field" if warm else "zero")
        assert rep.l2_err == -1.0 and rep.max_err == -1.0 and rep.max_outside > 0
        wref = ref.w[1:-1, 1:-1].numpy()
        np.testing.assert_allclose(rep.w, wref, rtol=0, atol=1e-9)  # (test_oracle.py's bound for the built-in problem)
        assert fc.l2_exact(prob, rep.w) == pytest.approx(fc.l2_exact(prob, wref), rel=1e-9)
        if "decomp" in kw:
            px, py = (int(v) for v in kw["decomp"].split("x"))
            assert (rep.Px, rep.Py) == (px, py)


@pytest.mark.parametrize("backend,kw", BACKENDS_40[:3] + [("torch", dict(device="cpu"))])
def test_restart_from_the_returned_w(backend, kw):
    prob = EllipseProblem(40, 40)
    first = solve(prob, backend=backend, rhs=fc.rhs(40, 40), return_w=True, **kw)
    again = solve(prob, backend=backend, rhs=fc.rhs(40, 40), w0=first.w, return_w=True, **kw)
    assert first.iters == 69 and again.converged and again.iters == 1 and again.init == "field"


def test_torch_backend_with_fields():
    prob = EllipseProblem(26, 27)
    rep = solve(prob, backend="torch", device="cpu", rhs=fc.rhs(26, 27), w0=fc.w0(26, 27), return_w=True)
    assert rep.iters == 56 and rep.init == "field" and rep.l2_err == -1.0
    assert np.array_equal(rep.w, fc.torch_solve(26, 27, True).w[1:-1, 1:-1].numpy())


# ---- the slicing helper -----------------------------------------------------------------
@pytest.mark.parametrize("px,py", [(2, 2), (3, 2), (1, 4)])
def test_block_fields_tile_and_ring(nat, px, py):
    """An array whose value encodes (i, j): the owned parts tile the interior
    exactly; the rings are the neighbours' edge values, zero on the box boundary."""
    M, N = 26, 27
    i, j = np.meshgrid(np.arange(1, M), np.arange(1, N), indexing="ij")
    g = (1000.0 * i + j).astype(np.float64)
    full = np.zeros((M + 1, N + 1))
    full[1:M, 1:N] = g
    seen = np.zeros((M - 1, N - 1), dtype=int)
    for r in range(px * py):
        blk = D.block(M, N, px * py, r, f"{px}x{py}")
        owned, ringed = nat.block_fields(M, N, blk, g, g)
        assert owned.shape == (blk.nx, blk.ny) and ringed.shape == (blk.nx + 2, blk.ny + 2)
        assert np.array_equal(owned, g[blk.i0 - 1:blk.i0 - 1 + blk.nx, blk.j0 - 1:blk.j0 - 1 + blk.ny])
        seen[blk.i0 - 1:blk.i0 - 1 + blk.nx, blk.j0 - 1:blk.j0 - 1 + blk.ny] += 1
        assert np.array_equal(ringed, full[blk.i0 - 1:blk.i0 + blk.nx + 1, blk.j0 - 1:blk.j0 + blk.ny + 1])
        assert np.array_equal(ringed[1:-1, 1:-1], owned)
        nbr = blk.nbr  # LEFT, RIGHT (x), DOWN, UP (y)
        for side, edge in ((0, ringed[0, 1:-1]), (1, ringed[-1, 1:-1]), (2, ringed[1:-1, 0]), (3, ringed[1:-1, -1])):
            assert (nbr[side] < 0) == bool((edge == 0).all()), (r, side)
    assert (seen == 1).all()
    assert nat.block_fields(M, N, D.block(M, N, 1, 0), None, None) == (None, None)
    with pytest.raises(ValueError):
        nat.block_fields(M, N, D.block(M, N, 1, 0), g[:, :-1], None)


# ---- input checks -----------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["serial", "ranks", "torch", "hip", "hip-group", "dist-cpu"])
@pytest.mark.parametrize("name", ["rhs", "w0"])
def test_bad_fields_rejected(backend, name):
    """Wrong shape, non-finite values and data float64 cannot hold are
    ValueErrors before any solver (or device, or process group) is touched."""
    import inspect

    # (a solve() that swallowed the keyword would go on to the device / process group with these backends)
    assert name in inspect.signature(solve).parameters
    prob = EllipseProblem(40, 40)
    good = fc.rhs(40, 40)
    nan = good.copy()
    nan[3, 5] = np.nan
    inf = good.copy()
    inf[0, 0] = np.inf
    big = np.full((39, 39), 2 ** 53 + 1, dtype=np.int64)        # not a float64
    wide = good.astype(np.longdouble) + np.longdouble(2) ** -60  # (x87 extended: bits float64 drops)
    bad = [good.T[:, :-1], good[:-1], good.ravel(), np.zeros((41, 41)), nan, inf, big, good.astype(complex),
           good.astype(str)]
    if np.finfo(np.longdouble).nmant > 52:
        bad.append(wide)
    for f in bad:
        with pytest.raises(ValueError):
            solve(prob, backend=backend, ranks=2 if backend in ("ranks", "hip-group") else 1, **{name: f})


def test_float32_is_converted_exactly():
    """float32 (like any dtype float64 holds exactly) is accepted: the solve is
    the float64 solve of the same values.  A float32 COPY of float64 data has
    lost bits before the solver sees it — that solve differs from the float64 one."""
    prob = EllipseProblem(26, 27)
    f32 = fc.rhs(26, 27).astype(np.float32)
    a = solve(prob, backend="serial", rhs=f32, return_w=True)
    b = solve(prob, backend="serial", rhs=f32.astype(np.float64), return_w=True)
    c = solve(prob, backend="serial", rhs=np.round(fc.rhs(26, 27)).astype(np.int32), return_w=True)
    assert a.iters == b.iters and np.array_equal(a.w, b.w) and c.converged
    assert not np.array_equal(a.w, solve(prob, backend="serial", rhs=fc.rhs(26, 27), return_w=True).w)


# ---- CLI -----------------------------------------------------------------------------------
def test_cli_dump_is_a_valid_w0(tmp_path):
    """--rhs, --dump → --w0 on --backend serial: the second run starts from
    the first run's solution and stops after one iteration; the L2 line says
    why there is no error figure; --help states the checkpoint rules."""
    from poisson_ellipse_openmp_mpi_cuda_amd.utils.report import parse_legacy

    f, w = str(tmp_path / "f.npy"), str(tmp_path / "w.npy")
    np.save(f, fc.rhs(40, 40))
    base = [sys.executable, "-m", "poisson_ellipse_openmp_mpi_cuda_amd", "--backend", "serial", "--rhs", f]
    out = subprocess.run(base + ["--dump", w, "40", "40"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert parse_legacy(out)["iters"] == 69 and "L2 error in D ~ n/a (user right-hand side)" in out
    assert np.load(w).shape == (39, 39)
    out = subprocess.run(base + ["--w0", w, "--json", "40", "40"], cwd=ROOT, capture_output=True, text=True,
                         check=True).stdout
    assert parse_legacy(out)["iters"] == 1 and '"init": "field"' in out and '"l2_err": -1.0' in out
    bad = subprocess.run(base + ["--w0", w, "41", "40"], cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "expected the global interior" in bad.stderr
    text = subprocess.run(base[:3] + ["--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    text = " ".join(text.split())  # (argparse wraps the help)
    assert "--rhs" in text and "--w0" in text and "needs the same" in text and "ignored with --resume" in text


# ---- the slicing helper under ASan + UBSan (a stand-alone host program) -----------------------
def test_slicing_helper_sanitizer_clean():
    import shutil

    if shutil.which("make") is None or shutil.which("g++") is None:
        pytest.skip("no host toolchain")
    r = subprocess.run(["make", "-s", "bin/pe_fields_asan"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    for grid in (("26", "27", "2", "2"), ("26", "27", "3", "2"), ("26", "27", "1", "4"), ("9", "9", "8", "8")):
        out = subprocess.run([os.path.join(ROOT, "bin", "pe_fields_asan"), *grid], capture_output=True, text=True,
                             timeout=120, env=env)
        text = out.stdout + out.stderr
        assert out.returncode == 0 and ": ok" in out.stdout, text[-2000:]
        assert "AddressSanitizer" not in text and "runtime error" not in text


# ---- one process per CPU rank (torch.distributed gloo) -------------------------------------------
def test_dist_cpu_with_fields(tmp_path):
    """Three processes, a 1x3 split of 26×27 (remainder columns): every rank
    loads the same global arrays and cpu_pcg cuts its slice; the count and
    the gathered w equal the serial solve's."""
    import json

    from conftest import free_port

    M, N = 26, 27
    f, g, outp = str(tmp_path / "f.npy"), str(tmp_path / "g.npy"), str(tmp_path / "w.npy")
    np.save(f, fc.rhs(M, N))
    np.save(g, fc.w0(M, N))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "-m", "poisson_ellipse_openmp_mpi_cuda_amd", "--backend",
           "dist-cpu", "--decomp", "1x3", "--json", "--quiet", "--rhs", f, "--w0", g, "--dump", outp, str(M), str(N)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    ref = solve(EllipseProblem(M, N), backend="serial", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    assert d["ranks"] == 3 and (d["Px"], d["Py"]) == (1, 3) and d["converged"] and d["iters"] == ref.iters == 56
    assert d["init"] == "field" and d["l2_err"] == -1.0
    np.testing.assert_allclose(np.load(outp), ref.w, rtol=0, atol=1e-12)
