"""The references of test_classic_gpu.py (classic_checks.REFERENCES) before a
device sees them: torch_ref.classic — the reference loop without a stop test,
the state the classic two-kernel path holds after K iterations — against the
capped reference loop, the native serial backend (an independent C++
implementation that carries the shift) and, unshifted, the single-sweep
recurrence; and the block sizes the multi-rank shapes are there for
(classic_checks.BLOCKS).  The rule of test_oracle.test_edge_shape_references_agree:
a case whose references disagree is not compared on a device."""

import classic_checks as cc
import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D


def _id(c):
    M, N, k, sigma, member, with_fields = c
    return f"{M}x{N}-K{k}-s{sigma:g}-{member or 'ref'}-{'fields' if with_fields else 'builtin'}"


@pytest.mark.parametrize("case", cc.REFERENCES, ids=_id)
def test_classic_references_agree(case):
    """w of the three loops within 1e-13·max|w| — ten times inside the device
    bound — with the capped loops ending at K unconverged (K is short of
    convergence); σ = 0: r, p, w of the single-sweep recurrence within 1e-13
    of each plane's maximum; the last sums, α and β consistent with the
    planes they belong to."""
    M, N, k, sigma, member, with_fields = case
    prob = cc.problem(M, N, sigma, member)
    kw = cc.fields(M, N, with_fields)
    ref = cc.reference(M, N, k, sigma, member, with_fields)
    assert ref.iters == k == len(ref.alpha) == len(ref.beta) == len(ref.sums)
    wmax = float(ref.w.abs().max())

    loop = torch_ref.pcg(prob, max_iter=k, **kw)
    assert loop.iters == k and not loop.converged
    assert float((ref.w - loop.w).abs().max()) <= 1e-13 * wmax

    prob.max_iter = k
    ser = solve(prob, backend="serial", return_w=True, **kw)
    assert ser.iters == k and not ser.converged
    assert abs(ser.w - ref.w[1:M, 1:N].numpy()).max() <= 1e-13 * wmax

    if sigma == 0.0:
        one = torch_ref.single_sweep(cc.problem(M, N, 0.0, member), k, **kw)
        for name in ("r", "p", "w"):
            a, b = getattr(ref, name), getattr(one, name)
            assert float((a - b).abs().max()) <= 1e-13 * float(b.abs().max()), name
        assert ref.alpha[-1] == pytest.approx(one.alpha[-1], rel=1e-12)
        assert ref.beta[-1] == pytest.approx(one.beta[-1], rel=1e-12)
        assert ref.sums[-1][2] == pytest.approx(one.sums[k][0], rel=1e-12)  # Σ z·r
        assert ref.sums[-1][1] == pytest.approx(one.sums[k][6], rel=1e-12)  # Σ p·p
        assert ref.sums[-1][0] == pytest.approx(one.sums[k][3], rel=1e-12)  # Σ Ap·p

    # the sums belong to the planes returned: Σ p·p from p, α_K from the sums before it
    inner = lambda u, v: float((u[1:-1, 1:-1] * v[1:-1, 1:-1]).sum())  # noqa: E731
    assert ref.sums[-1][1] == inner(ref.p, ref.p)
    assert ref.alpha[-1] == pytest.approx(ref.sums[-2][2] / ref.sums[-1][0], rel=1e-13)
    assert ref.beta[-1] == pytest.approx(ref.sums[-2][2] / ref.sums[-3][2], rel=1e-13)


def test_every_device_case_has_a_reference():
    """The tables test_classic_gpu.py is parametrised with name references listed above only."""
    have = set(cc.REFERENCES)
    for M, N, k in cc.EDGES:
        assert {(M, N, k, s, None, True) for s in cc.SIGMAS} <= have
    assert {cc.BUILTIN + (s, None, False) for s in cc.SIGMAS} <= have
    assert {cc.FORCED_GRID + (s, None, True) for s in cc.FORCED_SIGMAS} <= have
    for M, N, k, s, _, m in cc.family_cases():
        assert (M, N, k, s, m, True) in have
        assert m != "cut_xy" or M > 10
    for M, N, ranks, decomp in cc.VIRTUAL + cc.PROCESSES:
        assert (M, N, ranks, decomp) in cc.BLOCKS and ranks <= 4
        assert {(M, N, cc.K, s, None, True) for s, _ in cc.RANK_SIGMAS} <= have
    for M, N, ranks, decomp, m in cc.VIRTUAL_FAMILY:
        assert (M, N, cc.K, 40.0, m, True) in have
    # (tiny converges in one iteration on grids of 4 or fewer interior rows: not among the members on 5×130)
    assert all(c[4] != "tiny" or c[0] > 5 for c in have)


@pytest.mark.parametrize("M,N,ranks,decomp", sorted(cc.BLOCKS))
def test_classic_case_blocks(M, N, ranks, decomp):
    """The decomposition gives the multi-rank cases the block widths they are
    there for: 129 / 128 (a one-column last strip in front of an UP
    neighbour), 128 / 128 (a full last strip), 128 / 127 / 127 (the halo
    column in lane 63), one-row slabs."""
    rows, cols = cc.BLOCKS[(M, N, ranks, decomp)]
    blks = D.blocks(M, N, ranks, decomp)
    assert (blks[0].Px, blks[0].Py) == (len(rows), len(cols))
    assert sorted({(b.i0, b.nx) for b in blks}) == [(1 + sum(rows[:i]), rows[i]) for i in range(len(rows))]
    assert sorted({(b.j0, b.ny) for b in blks}) == [(1 + sum(cols[:j]), cols[j]) for j in range(len(cols))]
    assert sum(rows) == M - 1 and sum(cols) == N - 1
