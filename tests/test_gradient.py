"""CPU tests of the solution's gradient and its functionals (return_grad):
pe::gradient_field (native.gradient_field) and torch_ref.gradient against the
numpy definition in grad_checks.py bit for bit, the CPU backends end to end,
the refusals, the CLI, and the analytic tie ∫u = ∫|∇u|² = π/40 for F = 1.

Without the feature every test fails: native.gradient_field, torch_ref.gradient
and solve(return_grad=) do not exist."""

import json
import math
import os
import subprocess
import sys

import grad_checks as gc
import numpy as np
import pytest
import torch

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, native, solve
from poisson_ellipse_openmp_mpi_cuda_amd.cli import main as cli_main
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(cx=30.0, cy=30.0)  # a family member whose 12×12 grid has isolated inside nodes ("neither" class)
GRIDS = [(10, 50, {}), (40, 40, {}), (66, 49, {}), (12, 12, TINY)]


def test_difference_classes_are_all_covered():
    """On the built-in ellipse every inside node has an inside neighbour at
    these shapes (class 0 empty); the 12×12 member with cx = cy = 30 has nodes
    of all four classes in both directions."""
    seen = {}
    for M, N, fam in GRIDS:
        counts = gc.class_counts(EllipseProblem(M, N, **fam))
        print(f"grad-classes {M}x{N} {fam} {counts}")
        if not fam:
            assert counts[("x", 0)] == 0 and counts[("y", 0)] == 0
            assert all(counts[(d, k)] > 0 for d in "xy" for k in (1, 2, 3)), (M, N, counts)
        for key, n in counts.items():
            seen[key] = seen.get(key, 0) + n
    tiny = gc.class_counts(EllipseProblem(12, 12, **TINY))
    assert all(tiny[(d, k)] > 0 for d in "xy" for k in range(4)), tiny
    assert all(n > 0 for n in seen.values())


@pytest.mark.parametrize("M,N,fam", GRIDS)
def test_native_and_torch_match_the_definition(M, N, fam):
    """A seeded random w, non-zero outside the ellipse: both host twins give
    the definition's bits, and exact zeros outside."""
    prob = EllipseProblem(M, N, **fam)
    w = gc.random_w(prob, seed=M * 1000 + N)
    outside = gc.classes(prob)[0] < 0
    assert outside.any() and np.abs(w[outside]).min() > 0
    stats, g = native().gradient_field(prob.to_native(), w)
    gc.check_values(f"native {M}x{N}", prob, w, g, *stats)
    assert not g[:, outside].any()
    only, none = native().gradient_field(prob.to_native(), w, False)
    assert none is None and only == stats
    W = torch.zeros(M + 1, N + 1, dtype=torch.float64)
    W[1:M, 1:N] = torch.from_numpy(w)
    gt, *st = torch_ref.gradient(prob, W)
    gc.check_values(f"torch {M}x{N}", prob, w, gt.numpy(), *st)
    assert np.array_equal(gt.numpy(), np.asarray(g))


def test_outside_values_never_enter():
    """Other (huge) values outside the ellipse: the same field and figures —
    only values at inside nodes are ever used."""
    prob = EllipseProblem(40, 40)
    w = gc.random_w(prob)
    ins = gc.classes(prob)[0] >= 0
    w2 = np.where(ins, w, 1e6 * (1.0 + w))
    a, ga = native().gradient_field(prob.to_native(), w)
    b, gb = native().gradient_field(prob.to_native(), w2)
    assert a == b and np.array_equal(ga, gb)


@pytest.mark.parametrize("backend,kw", [("serial", {}), ("omp", dict(threads=2)), ("ranks", dict(ranks=4)),
                                        ("torch", {})])
def test_backends_end_to_end(backend, kw):
    prob = EllipseProblem(40, 40)
    base = solve(prob, backend=backend, return_w=True, **kw)
    rep = solve(prob, backend=backend, return_w=True, return_grad=True, **kw)
    assert rep.converged and rep.iters == 50
    gc.same_solve(backend, rep, base)
    gc.check_report(backend, prob, rep)
    assert isinstance(rep.grad, np.ndarray) and rep.grad.shape == (2, 39, 39)
    st = solve(prob, backend=backend, return_grad="stats", **kw)
    assert st.grad is None and st.w is None
    assert (st.integral, st.energy, st.grad_max) == (rep.integral, rep.energy, rep.grad_max)
    d = rep.to_dict()
    assert "grad" not in d and (d["integral"], d["energy"], d["grad_max"]) == (rep.integral, rep.energy, rep.grad_max)
    assert json.dumps(d)


def test_dist_cpu_gradient_of_the_gathered_w(tmp_path):
    """Two gloo processes, 2×1 blocks of 26×27, nine iterations from w0
    (gradient_job.py): rank 0 applies gradient_field to the gathered w; rank 1
    holds no gathered w and reports nothing."""
    import field_checks as fc
    from conftest import free_port

    M, N = 26, 27
    np.save(tmp_path / "f.npy", fc.rhs(M, N))
    np.save(tmp_path / "g.npy", fc.w0(M, N))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "gradient_job.py"), "dist-cpu",
           str(M), str(N), "9", str(tmp_path / "f.npy"), str(tmp_path / "g.npy"), str(tmp_path / "out"), "2x1"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = [json.load(open(tmp_path / f"out.r{r}.json")) for r in range(2)]
    prob = EllipseProblem(M, N)
    w, g = np.load(tmp_path / "out.r0.w.npy"), np.load(tmp_path / "out.r0.g.npy")
    assert d[0]["iters"] == 9 and not d[0]["converged"] and (d[0]["Px"], d[0]["Py"]) == (2, 1)
    gc.check_values("dist-cpu 2x1", prob, w, g, d[0]["integral"], d[0]["energy"], d[0]["grad_max"])
    assert not os.path.exists(tmp_path / "out.r1.g.npy") and d[1]["integral"] == -1.0


def test_refusals():
    prob = EllipseProblem(40, 40)
    for backend in ("serial", "omp", "ranks", "torch", "dist-cpu"):
        with pytest.raises(ValueError, match="return_grad"):
            solve(prob, backend=backend, return_grad="device")
    for bad in ("host", "Stats", ""):
        for backend in ("serial", "hip", "hip-group"):
            with pytest.raises(ValueError, match="return_grad"):
                solve(prob, backend=backend, return_grad=bad)
    nat = native()
    with pytest.raises(ValueError):
        nat.gradient_field(prob.to_native(), np.zeros((39, 40)))
    with pytest.raises(ValueError):
        nat.gradient_field(prob.to_native(), None)


def test_cli_grad_stats_and_dump(tmp_path, capsys):
    out = tmp_path / "g.npy"
    assert cli_main(["--backend", "serial", "--grad-stats", "--dump-grad", str(out), "--json", "40", "40"]) == 0
    text = capsys.readouterr().out
    rep = solve(EllipseProblem(40, 40), backend="serial", return_grad=True)
    g = np.load(out)
    assert g.shape == (2, 39, 39) and np.array_equal(g, rep.grad)
    lines = text.splitlines()
    at = [n for n, line in enumerate(lines) if "Integral of w in D" in line]
    legacy = [n for n, line in enumerate(lines) if "Process grid" in line]
    assert len(at) == 1 and legacy and at[0] > legacy[-1]  # after the legacy block, never inside it
    assert f"{rep.integral:.6e}" in lines[at[0]] and f"{rep.energy:.6e}" in lines[at[0]]
    d = json.loads([line for line in lines if line.startswith("{")][0])
    assert (d["integral"], d["energy"], d["grad_max"]) == (rep.integral, rep.energy, rep.grad_max)
    assert cli_main(["--backend", "serial", "--quiet", "--json", "40", "40"]) == 0
    d = json.loads([line for line in capsys.readouterr().out.splitlines() if line.startswith("{")][0])
    assert (d["integral"], d["energy"], d["grad_max"]) == (-1.0, -1.0, -1.0)


def tie(rep):
    """Relative deviations of (integral, energy) from π/40, both of which they stay below."""
    want = math.pi / 40.0
    assert rep.integral < want and rep.energy < want, (rep.integral, rep.energy)
    return (want - rep.integral) / want, (want - rep.energy) / want


def test_analytic_tie():
    """F = 1: ∫u = ∫|∇u|² = π/40 (∫|∇u|² = F∫u).  Measured on the PyTorch fp64
    oracle, zero init, δ = 1e-6: 40² integral 0.0743506 (−5.3 %), energy
    0.0766740 (−2.4 %); 200² 0.0776760 (−1.10 %), 0.0785249 (−0.019 %) —
    discretisation error, the same on every backend to about δ."""
    a = tie(solve(EllipseProblem(40, 40), backend="torch", return_grad="stats"))
    b = tie(solve(EllipseProblem(200, 200), backend="omp", threads=4, return_grad="stats"))
    print(f"grad-tie cpu 40x40 {a[0]:.3e} {a[1]:.3e}  200x200 {b[0]:.3e} {b[1]:.3e}")
    assert a[0] <= 6e-2 and a[1] <= 3e-2
    assert b[0] <= 1.3e-2 and b[1] <= 3e-4
    assert b[0] < a[0] and b[1] < a[1]
