"""The cases of test_band_pins.py: what each runs and which arrays it pins.

The three-step sweep's band march (items that hold a boundary-band row) was
changed without changing a floating-point operation or the order of a sum:
the middle six-step groups run without row tests, on running row pointers,
and a row's class and coefficients are taken once, when it enters the
pipeline.  Its outputs are pinned bit for bit against fixtures recorded on the
commit before that change (tests/golden/band_pins/*.npz, written by
tools/record_band_pins.py).  A case returns a dict of arrays; the test
compares every one of them with np.array_equal.  The helpers are
pin_checks.py's.

A band item of `rows` rows marches rows + 12 steps; its steady groups are the
six-step groups from step 12 on that end by step rows + 5, as a uniform
item's (pin_checks.steady_groups).

Shapes — the smallest that reach each part of the band march:
  band-ti7 .. ti61      the reference ellipse at 130×97 (two strips, a band
                        node in every row: band items only), whole items
                        ("fill" layout) of 7 rows (no steady group), 13 and 19
                        (the first heights with one and two) and 61 (73 steps:
                        the 7-slot face ring against the 6-step group over
                        more than their common period of 42)
  band-ti96 / ti130     96 and 129 rows: the 64-row class window is reloaded
                        inside steady groups
  band-ti19-K10         a fourth sweep that applies one iteration (the cap
                        inside a sweep)
  ref-40x200            five strips: band items of 19-39 rows next to a
                        uniform one
  cut_xy / offc / tiny  66×49, one strip with box-boundary columns: interior
                        coefficients at the box edge; tiny: isolated inside
                        nodes, a band item next to a uniform one
  laststrip-66x50       49 columns: a second strip with one output column
  up-2x2-66x99          2x2 virtual ranks, blocks of 33/32 rows × 49 columns:
                        the one-column last strip of ranks 0 and 1 faces an UP
                        neighbour (the column mask of the sums)
  push-loop-band        kS3<PUSH>: rank 1 of a 4x1 split of 260×97 with the
                        in-sweep push in loopback; the slab's first and last
                        items are band items with steady groups
  solve-* / cap-*       a converged solve (the launch that resolves the stop
                        test, the fix-up) and solves capped on a sweep's first
                        and second iteration (the replay): iteration count, w
                        and the recurrence's residual norm
"""

import os

import numpy as np
import pin_checks
import sweep_checks
from pin_checks import environment, steady_groups

from poisson_ellipse_openmp_mpi_cuda_amd import solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

GOLDEN = os.path.join(pin_checks.ROOT, "tests", "golden", "band_pins")
BAND_BIT, UNI_BIT = sweep_checks.BAND_BIT, sweep_checks.UNI_BIT
THREE = pin_checks.THREE

FILL = {"PE_LAYOUT": "fill"}  # whole items of the forced height
LPT48 = {"PE_TI": "48", "PE_LAYOUT": "lpt"}
# name -> (M, N, member, iterations, environment, steady groups of the tallest band item, uniform items in the list)
SWEEPS = {
    "band-ti7": (130, 97, None, 9, dict(FILL, PE_TI="7"), 0, False),
    "band-ti13": (130, 97, None, 9, dict(FILL, PE_TI="13"), 1, False),
    "band-ti19": (130, 97, None, 9, dict(FILL, PE_TI="19"), 2, False),
    "band-ti61": (130, 97, None, 9, dict(FILL, PE_TI="61"), 9, False),
    "band-ti96": (130, 97, None, 9, dict(FILL, PE_TI="96"), 14, False),
    "band-ti130": (130, 97, None, 9, dict(FILL, PE_TI="130"), 20, False),
    "band-ti19-K10": (130, 97, None, 10, dict(FILL, PE_TI="19"), 2, False),
    "ref-40x200": (40, 200, None, 9, LPT48, 5, True),
    "cut_xy-66x49": (66, 49, "cut_xy", 9, LPT48, 2, False),
    "offc-66x49": (66, 49, "offc", 9, LPT48, 2, False),
    "tiny-66x49": (66, 49, "tiny", 9, LPT48, 2, True),
    "laststrip-66x50": (66, 50, None, 9, LPT48, 2, False),
}
RELOADS = ("band-ti96", "band-ti130")  # the march passes the first 64-row class window inside steady groups
# name -> (M, N, iteration cap or None)
SOLVES = {"solve-ref-66x49": (66, 49, None), "cap-ref-66x49-31": (66, 49, 31), "cap-ref-66x49-32": (66, 49, 32)}
UP = "up-2x2-66x99"
PUSH_LOOP = "push-loop-band"
NAMES = list(SWEEPS) + list(SOLVES) + [UP, PUSH_LOOP]


def band_rows(entries):
    return [rows for _ib, rows, _strip, flags in entries if rows > 0 and flags & BAND_BIT]


def run_sweeps(nat, name):
    M, N, member, K, env, groups, has_uniform = SWEEPS[name]
    with environment(env):
        s = sweep_checks.solver(nat, M, N, "three", member)
        assert s.sweep_steps == 3 and s.layout_name == env["PE_LAYOUT"]
        band = band_rows(s.layout_entries)
        assert band, (name, "no band item in the list")
        assert max(map(steady_groups, band)) == groups, (name, sorted(band))
        assert bool(pin_checks.uniform_rows(s.layout_entries)) == has_uniform, (name, s.layout_entries)
        if name in RELOADS:
            assert max(band) + 12 > 64 + 6
        s.reset()
        s.run_iterations(K, False)
        s.synchronize()
        st, out = pin_checks._planes(s, M, N)
        assert st["iter"] == K and st["status"] == 0, (st["iter"], st["status"])
    return out


def run_solve(nat, name):
    M, N, cap = SOLVES[name]
    with environment(LPT48):
        s = sweep_checks.solver(nat, M, N, "three")
        band = band_rows(s.layout_entries)
        assert band and max(map(steady_groups, band)) >= 1, (name, sorted(band))
        del s
        prob = sweep_checks.problem(M, N)
        if cap:
            prob.max_iter = cap
        rep = solve(prob, backend="hip", algo=THREE, return_w=True)
    assert rep.algo == THREE
    assert (rep.iters == cap and not rep.converged) if cap else rep.converged
    return {"iters": np.array([rep.iters], dtype=np.int64), "w": np.array(rep.w),
            "res_rec": np.array([rep.res_rec], dtype=np.float64)}


def run_up(nat):
    M, N, K = 66, 99, 9
    with environment(LPT48):
        prob = sweep_checks.problem(M, N)
        for rank in (0, 1):  # the lists of the blocks under an UP neighbour, from the host planner
            blk = nat.decompose(M, N, D.grid(4, M, N, "2x2"), rank)
            assert blk.ny == 49 and blk.nbr[3] >= 0, (rank, blk.ny, list(blk.nbr))
            lay = nat.item_layout(prob.to_native(), blk, 3, 48, layout="lpt")
            last = [rows for _ib, rows, strip, flags in lay["entries"] if rows > 0 and flags & BAND_BIT and strip == 1]
            assert last and max(map(steady_groups, last)) >= 1, (rank, lay["entries"])
        prob.max_iter = K
        rep = solve(prob, backend="hip-group", ranks=4, decomp="2x2", check_tol=False, return_w=True)
    assert rep.Px == 2 and rep.Py == 2 and rep.algo == THREE, (rep.Px, rep.Py, rep.algo)
    assert rep.iters == K and not rep.converged, (rep.iters, rep.converged)
    return {"w": np.array(rep.w)}


def run_push_loop(nat):
    M, N = 261, 98
    prob = sweep_checks.problem(M, N)
    blk = nat.decompose(M, N, D.grid(4, M, N, "4x1"), 1)
    with environment(dict(LPT48, PE_PUSH_LOOPBACK="1", PE_HALO="push")):
        opt = nat.SolveOptions()
        opt.algo = 4
        opt.check_tol = False
        comm = nat.make_delay_comm(4, 0.0, 0.0, True)
        s = nat.DeviceSolver(prob.to_native(), blk, comm, opt)
        assert s.sweep_steps == 3 and s.ti == 48
        assert s.halo_push and s.push_status.startswith("loopback"), (s.halo_path, s.push_status)
        for edge in (lambda ib, rows: ib == 1, lambda ib, rows: ib + rows - 1 == blk.nx):
            rows_e = [rows for ib, rows, _s, flags in s.layout_entries if rows > 0 and flags & BAND_BIT and edge(ib, rows)]
            assert rows_e and max(map(steady_groups, rows_e)) >= 1, s.layout_entries
        s.reset()
        s.run_iterations(9, False)
        s.synchronize()
        st = s.state()
        assert st["iter"] == 9 and st["status"] == 0, (st["iter"], st["status"])
        out = {"w": np.array(s.w()), "sums": np.array(st["fs2"][int(st["wpar"])][:19], dtype=np.float64)}
        del s, comm
    return out


def run_case(nat, name):
    if name in SWEEPS:
        return run_sweeps(nat, name)
    if name in SOLVES:
        return run_solve(nat, name)
    if name == UP:
        return run_up(nat)
    assert name == PUSH_LOOP
    return run_push_loop(nat)


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".npz")
