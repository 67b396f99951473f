"""MI355X tests of the four marching sweeps — kS3 (fused3.hip), kS2
(fused2.hip), kS (fused.hip) and kResident (resident.hip) — against the
PyTorch fp64 recurrence at strip and item edges: a last strip of exactly one
output column and one exactly full (strips are 48 / 120 / 124 output
columns), blocks of the minimum 8 rows (shorter than kS3's seven-stage
pipeline is deep plus one), a short last item, and items forced shorter than
the pipeline (PE_TI) under every static layout.  Strip masks, halo lanes
dropped from the sums, clamped loads at the last rows and the pipelines' fill
and drain are what these shapes reach; the comparison (the reduced sums, the
last α / β, the r / p planes and w, node for node) and its tolerances are
sweep_checks.check_sweeps, the one the 300×420 / 257×129 / 130×1000 tests
use.  test_oracle.py holds the references of every shape here to each other
ten times tighter, without a device.

Two virtual-rank solves sit at the multi-step threshold: 2x2 blocks of
exactly 12×12 run the three-step sweep, 11×11 the single sweep."""

import numpy as np
import pytest
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M,N,J", sweep_checks.THREE_EDGES)
def test_three_step_edges(gpu, nat, M, N, J):
    s = sweep_checks.solver(nat, M, N, "three")
    sweep_checks.check_sweeps(s, M, N, "three", J)


@pytest.mark.parametrize("M,N,J", sweep_checks.TWO_EDGES)
def test_two_step_edges(gpu, nat, M, N, J):
    s = sweep_checks.solver(nat, M, N, "two")
    assert s.two_step
    sweep_checks.check_sweeps(s, M, N, "two", J)


@pytest.mark.parametrize("M,N,K", sweep_checks.SINGLE_EDGES)
def test_single_sweep_edges(gpu, nat, M, N, K, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", "0")
    s = sweep_checks.solver(nat, M, N, "single")
    assert not s.resident
    sweep_checks.check_sweeps(s, M, N, "single", K)


@pytest.mark.parametrize("M,N,K", sweep_checks.SINGLE_EDGES)
def test_resident_edges(gpu, nat, M, N, K, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", "1")
    s = sweep_checks.solver(nat, M, N, "single")
    assert s.resident
    sweep_checks.check_sweeps(s, M, N, "single", K)


@pytest.mark.parametrize("layout", sweep_checks.SHORT_THREE[2])
@pytest.mark.parametrize("ti", sweep_checks.SHORT_THREE[1])
def test_three_step_short_items(gpu, nat, ti, layout, monkeypatch):
    """Items of 4, 7 and 13 rows: below, at and above the seven stages in
    flight, and either side of the six-step unrolled group."""
    M, N = sweep_checks.SHORT_GRID
    monkeypatch.setenv("PE_TI", str(ti))
    monkeypatch.setenv("PE_LAYOUT", layout)
    s = sweep_checks.solver(nat, M, N, "three")
    assert s.ti == ti and s.layout_name == layout
    sweep_checks.check_sweeps(s, M, N, "three", sweep_checks.SHORT_THREE[0])


@pytest.mark.parametrize("ti", sweep_checks.SHORT_TWO[1])
def test_two_step_short_items(gpu, nat, ti, monkeypatch):
    M, N = sweep_checks.SHORT_GRID
    monkeypatch.setenv("PE_TI", str(ti))
    s = sweep_checks.solver(nat, M, N, "two")
    assert s.two_step and s.ti == ti
    sweep_checks.check_sweeps(s, M, N, "two", sweep_checks.SHORT_TWO[0])


@pytest.mark.parametrize("ti", sweep_checks.SHORT_SINGLE[1])
def test_single_sweep_short_items(gpu, nat, ti, monkeypatch):
    M, N = sweep_checks.SHORT_GRID
    monkeypatch.setenv("PE_TI", str(ti))
    monkeypatch.setenv("PE_RESIDENT", "0")
    s = sweep_checks.solver(nat, M, N, "single")
    assert not s.resident and s.ti == ti
    sweep_checks.check_sweeps(s, M, N, "single", sweep_checks.SHORT_SINGLE[0])


@pytest.mark.parametrize("M,algo", [(25, "three-step"), (23, "fused")])
def test_virtual_ranks_at_multi_step_threshold(gpu, M, algo):
    """2x2 virtual ranks on blocks of exactly 12×12 (the smallest the
    three-step sweep takes on a 2-D split) and of 11×11 (the single sweep)."""
    prob = EllipseProblem(M, M)
    rep = solve(prob, backend="hip-group", ranks=4, decomp="2x2", return_w=True)
    ref = solve(prob, backend="serial", return_w=True)
    assert rep.Px == 2 and rep.Py == 2 and rep.algo == algo
    assert rep.converged and abs(rep.iters - ref.iters) <= 1
    np.testing.assert_allclose(rep.w, ref.w, rtol=0, atol=1e-9)
