"""MI355X tests of multi-rank execution at the smallest slabs and blocks,
against the PyTorch fp64 recurrence: the 4- and 6-deep halos of the two- and
three-step sweeps (kS2, kS3), kPack / kUnpack, the peer put (p2p.hip kPut),
the in-sweep push and the cross-rank sums, each halo path forced, with and
without the halo/interior overlap, and the replay launch across ranks (a cap
on a sweep's first or second iteration).  Several processes share the one GPU
through the host-staged transport.

Every case runs a fixed 9-14 iterations, far from convergence, and is held
node for node to the bounds of the single-rank sweep tests
(sweep_checks.KINDS): w to 1e-11 of its maximum (1e-12 for the single sweep),
the recurrence's ‖r_K‖_E to the same bound carried through the norm, and the
end-of-solve figures to norm_checks.check_norms.  The converged multi-rank
solves of test_gpu.py (iterations ±1, w to 1e-9) would let a stale halo node
through.  Shapes, paths and the comparison: halo_checks.py; test_oracle.py
holds every reference used here to the others without a device, and the
decomposition to the block sizes the shapes are chosen for."""

import halo_checks
import pytest

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [halo_checks.case_id(c) for c in cases]


@pytest.mark.parametrize("case", halo_checks.TWO_SLABS, ids=_ids(halo_checks.TWO_SLABS))
def test_two_step_slabs(gpu, tmp_path, case):
    """Row slabs of 8-11 rows per rank take the two-step sweep under --algo
    auto: the depth-4 halo through the exchange, the put and the push."""
    halo_checks.check_case(case, tmp_path)


@pytest.mark.parametrize("case", halo_checks.THREE_SLABS, ids=_ids(halo_checks.THREE_SLABS))
def test_three_step_slabs(gpu, tmp_path, case):
    """Row slabs of exactly 12 rows per rank: the pushed edge rows 1..6 and
    nx−5..nx are the whole slab."""
    halo_checks.check_case(case, tmp_path)


@pytest.mark.parametrize("case", halo_checks.THREE_2D, ids=_ids(halo_checks.THREE_2D))
def test_three_step_2d_blocks(gpu, tmp_path, case):
    """2-D blocks of 12-13 rows: y strips, corners through the x phase, a
    one-column last strip whose other lanes are the UP neighbour's columns."""
    halo_checks.check_case(case, tmp_path)


@pytest.mark.parametrize("case", halo_checks.SINGLE_2D, ids=_ids(halo_checks.SINGLE_2D))
def test_single_sweep_2d_blocks(gpu, tmp_path, case):
    """11×11 blocks, below the multi-step threshold: the single sweep."""
    halo_checks.check_case(case, tmp_path)


@pytest.mark.parametrize("M,N,ranks,decomp,K,expect", halo_checks.VIRTUAL)
def test_virtual_ranks_fixed_count(gpu, M, N, ranks, decomp, K, expect):
    """The same 2-D shapes on virtual ranks of one process: the group driver's
    own pack, exchange and sums."""
    halo_checks.check_virtual(M, N, ranks, decomp, K, expect)
