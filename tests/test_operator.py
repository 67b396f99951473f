"""CPU tests of apply_operator / residual: the host definition
(native.apply_operator / native.residual_field, csrc/include/pe/fields.hpp)
bit for bit against the torch oracle, its sums, the operator's symmetry and
definiteness, every CPU backend of pe.apply_operator / pe.residual, a
two-process gloo job, the tie to a converged solve, validation and the CLI.
Inputs: operator_checks (field_checks.w0 / rhs).  Every test fails without the
feature: the names do not exist."""

import json
import math
import os
import subprocess
import sys

import field_checks as fc
import norm_checks
import numpy as np
import operator_checks as oc
import pytest
import torch
from conftest import free_port

import poisson_ellipse_openmp_mpi_cuda_amd as pe
from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, cli
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(10, 10, None), (40, 40, None), (257, 129, None)] + oc.STRETCHED


def torch_Av(prob, v):
    a, b, _ = torch_ref.assemble(prob)
    return torch_ref.apply_A(torch_ref.embed(prob, v), a, b, prob.h1, prob.h2)[1:-1, 1:-1].numpy()


@pytest.mark.parametrize("M,N,kw", SHAPES)
def test_host_definition_is_the_torch_oracle(nat, M, N, kw):
    prob = oc.problem(M, N, kw)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    ref = torch_Av(prob, v)
    hh = prob.h1 * prob.h2
    for threads in (1, 3):
        s, got = nat.apply_operator(prob.to_native(), v, True, threads)
        assert np.array_equal(got, ref), (M, N, threads)
        assert abs(s - hh * float((v * ref).sum())) <= 1e-12 * hh * float(np.abs(v * ref).sum())
        assert nat.apply_operator(prob.to_native(), v, False, threads) == (s, None)
        for rhs in (None, f):
            B = torch_ref.assemble(prob, rhs=rhs)[2][1:-1, 1:-1].numpy()
            inside = fc.inside(prob)
            assert np.array_equal(B, np.where(inside, 1.0 if rhs is None else f, 0.0))  # rhs inside, 0 outside; None: F
            sr, r = nat.residual_field(prob.to_native(), v, rhs, True, threads)
            assert np.array_equal(r, B - ref), (M, N, threads)
            assert sr == pytest.approx(hh * float((r * r).sum()), rel=1e-12)
            assert nat.residual_field(prob.to_native(), v, rhs, False, threads) == (sr, None)
    t = torch_ref.residual(prob, v, f)[1:-1, 1:-1].numpy()
    assert np.array_equal(t, nat.residual_field(prob.to_native(), v, f)[1])


def test_symmetric_and_positive_definite(nat):
    prob = EllipseProblem(40, 40)
    u, v = fc.rhs(40, 40), fc.w0(40, 40)
    P = prob.to_native()
    Au, Av = nat.apply_operator(P, u)[1], nat.apply_operator(P, v)[1]
    assert abs(float((u * Av).sum()) - float((Au * v).sum())) <= 1e-12 * float(np.abs(u * Av).sum())
    assert nat.apply_operator(P, v)[0] > 0 and nat.apply_operator(P, u)[0] > 0


def test_cpu_backends_agree():
    M = N = 40
    prob = EllipseProblem(M, N)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    runs = [dict(backend="serial"), dict(backend="omp", threads=4), dict(backend="ranks", ranks=4, decomp="2x2"),
            dict(backend="torch", device="cpu")]
    for kw in runs:
        a = pe.apply_operator(prob, v, **kw)
        oc.compare(kw["backend"], prob, a.field, a.sum)
        assert isinstance(a, pe.FieldResult) and a.origin is None
        assert np.array_equal(a.field, oc.host(prob)[0]), kw
        for user in (False, True):
            r = pe.residual(prob, v, rhs=f if user else None, **kw)
            oc.compare(kw["backend"], prob, r.field, r.sum, True, user)
            assert np.array_equal(r.field, oc.host(prob, True, user)[0]), kw
        only = pe.apply_operator(prob, v, out="sum", **kw)
        assert only.field is None and only.sum == a.sum
    # a CPU torch tensor and a float32 array are fields too
    a = pe.apply_operator(prob, torch.from_numpy(np.array(v)), backend="serial")
    assert np.array_equal(a.field, oc.host(prob)[0])
    a32 = pe.apply_operator(prob, v.astype(np.float32), backend="serial")
    assert np.array_equal(a32.field, oc.host(prob, f32=True)[0])


def test_two_process_gloo_job(tmp_path):
    M, N = 26, 27
    prob = EllipseProblem(M, N)
    paths = [str(tmp_path / n) for n in ("v.npy", "f.npy")]
    for p, a in zip(paths, (fc.w0(M, N), fc.rhs(M, N))):
        np.save(p, a)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "operator_job.py"),
           "dist-cpu", str(M), str(N), *paths, str(tmp_path / "out"), "aspect"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    d = []
    for r in range(2):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d.append(json.load(fh))
    assert d[0]["apply_sum"] == d[1]["apply_sum"] == oc.host(prob)[1]
    assert d[0]["resid_sum"] == d[1]["resid_sum"] == oc.host(prob, True, True)[1]
    assert np.array_equal(np.load(tmp_path / "out.r0.a.npy"), oc.host(prob)[0])
    assert np.array_equal(np.load(tmp_path / "out.r0.r.npy"), oc.host(prob, True, True)[0])
    assert not (tmp_path / "out.r1.a.npy").exists()


def test_converged_solve_residual_norm():
    prob = EllipseProblem(40, 40)
    rep = pe.solve(prob, backend="serial", return_w=True)
    assert rep.converged
    res = pe.residual(prob, rep.w, backend="serial")
    ref = norm_checks.fp64_norms(prob, rep.w)["res_true"]
    assert math.sqrt(res.sum) == pytest.approx(ref, rel=norm_checks.resid_tol(prob))
    assert math.sqrt(pe.residual(prob, rep.w, backend="serial", out="sum").sum) == math.sqrt(res.sum)


def test_validation():
    prob = EllipseProblem(10, 10)
    v = fc.w0(10, 10)
    for fn in (pe.apply_operator, pe.residual):
        with pytest.raises(ValueError, match="shape"):
            fn(prob, v[:-1], backend="serial")
        with pytest.raises(ValueError, match="dtype"):
            fn(prob, v.astype(np.complex128), backend="serial")
        with pytest.raises(ValueError, match="device"):
            fn(prob, v, backend="serial", out="device")
        with pytest.raises(ValueError, match="out"):
            fn(prob, v, backend="serial", out="gpu")
        with pytest.raises(ValueError):
            fn(prob, None, backend="serial")
        with pytest.raises(ValueError, match="backend"):
            fn(prob, v, backend="cuda")
    with pytest.raises(ValueError, match="rhs"):
        pe.residual(prob, v, rhs=v[:, :-1], backend="serial")
    bad = v.copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        pe.apply_operator(prob, bad, backend="serial")


def test_cli_dump_resid(tmp_path, capsys):
    M = N = 40
    prob = EllipseProblem(M, N)
    w, r, f = (str(tmp_path / n) for n in ("w.npy", "r.npy", "f.npy"))
    np.save(f, fc.rhs(M, N))
    assert cli.main(["--backend", "serial", "--rhs", f, "--dump", w, "--dump-resid", r, str(M), str(N)]) == 0
    out = capsys.readouterr().out
    from poisson_ellipse_openmp_mpi_cuda_amd.utils import dump

    wv = dump.load(w)
    wv = wv[0] if isinstance(wv, tuple) else wv
    got = np.load(r)
    s, ref = pe.native().residual_field(prob.to_native(), np.asarray(wv), fc.rhs(M, N))
    assert got.shape == (M - 1, N - 1) and np.array_equal(got, ref)
    line = [ln for ln in out.splitlines() if "||B - A w||_E" in ln]
    assert len(line) == 1 and float(line[0].split("~")[1]) == pytest.approx(math.sqrt(s), rel=1e-6)
