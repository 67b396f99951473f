"""MI355X tests of the three-step sweep's row addressing (kS3, fused3.hip):
the steady groups of a uniform item address their rows through running
64-bit row bases and 32-bit lane offsets, the fill and drain steps around
them through row·pitch products.  The shapes are the smallest at which the
two can disagree: items tall enough to reload their 58-row class window
inside steady groups, the first item heights with one and two steady groups
(the hand-over in both directions), a sweep cut short by the iteration cap
and the fix-up / replay launches after it, the push variant of the kernel,
and one grid whose planes pass 4 GiB.

Which items take the steady path is a property of the layout, so the tests
read it back (DeviceSolver.layout_entries) and assert what they rely on: on
260×97 the third strip (one output column, y ≥ 0.49) holds band rows only
for |x| < 0.25, and its items above and below them are uniform.  66×49 — one
strip over the whole y range, a band node in every row — has no uniform item:
it is here as the plain partial-sweep shape, next to 260×97.

References: the PyTorch fp64 recurrence (ops/torch_ref.py) through
sweep_checks.reference (computed once per shape, shared, never modified),
the comparison and its bounds sweep_checks.check_sweeps ("three") and
norm_checks.check_norms."""

import numpy as np
import pytest
import sweep_checks
from norm_checks import check_norms

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu

UNI_BIT = 1 << 29     # item_layout.hpp kUniBit: every row of the item's window is of one class in its strip
GRID = (261, 98)      # 260 rows × 97 columns: two full strips and a one-column strip
SWEEPS = 8
THREE = "three-step"
F_TOL = sweep_checks.KINDS["three"][6]  # fields and w: 1e-11 of the maximum


def uniform_rows(s):
    """Rows of every uniform item of solver s's layout."""
    return [rows for _ib, rows, _strip, flags in s.layout_entries if rows > 0 and flags & UNI_BIT]


def steady_groups(rows):
    """Steady six-step groups of a uniform item of `rows` rows (march3: group
    starts n0 = 12, 18, … ≤ rows − 1)."""
    return 0 if rows < 13 else (rows - 1 - 12) // 6 + 1


@pytest.mark.parametrize("layout", [None, "lpt"])
@pytest.mark.parametrize("M,ti", [(261, 96), (261, 112), (351, 112)])
def test_window_reload_in_steady_groups(gpu, nat, M, ti, layout, monkeypatch):
    """Items of 96 and 112 rows: taller than the 58-row class window, which
    load_seg reloads between steady groups.  260 rows at 96 per item leave a
    uniform last item of 68 rows below the band rows of the third strip; at
    112 per item every tall item reaches them (band items: the reload in
    generic groups only), so 350 rows carry a whole 112-row uniform item.
    Whole items need the LPT layout: the default of a block this small (the
    equal-cost layout) cuts them into pieces of 8-9 rows, one per wave."""
    N = GRID[1]
    monkeypatch.setenv("PE_TI", str(ti))
    if layout:
        monkeypatch.setenv("PE_LAYOUT", layout)
    s = sweep_checks.solver(nat, M, N, "three")
    assert s.ti == ti
    uni = uniform_rows(s)
    print(f"addr-layout {M}x{N} ti={ti} layout={s.layout_name} uniform item rows={sorted(uni)}")
    if layout == "lpt" and (M, ti) != (261, 112):
        assert max(uni, default=0) + 12 > 64, uni  # the march passes the first window inside steady groups
    sweep_checks.check_sweeps(s, M, N, "three", SWEEPS)


@pytest.mark.parametrize("layout", ["equal", "lpt", "fill"])
@pytest.mark.parametrize("ti", [13, 18, 19])
def test_steady_entry_thresholds(gpu, nat, ti, layout, monkeypatch):
    """13, 18 and 19 rows per item: one steady group right after the fill,
    one followed by a partial drain group, and the first height with two; the
    260 rows also leave a short last item without any."""
    M, N = GRID
    monkeypatch.setenv("PE_TI", str(ti))
    monkeypatch.setenv("PE_LAYOUT", layout)
    s = sweep_checks.solver(nat, M, N, "three")
    assert s.ti == ti and s.layout_name == layout
    groups = sorted({steady_groups(r) for r in uniform_rows(s)})
    print(f"addr-layout {M}x{N} ti={ti} layout={layout} steady groups per uniform item={groups}")
    if layout == "lpt":  # (whole items; the other two cut them to fill the waves)
        assert (2 if ti == 19 else 1) in groups, groups
    sweep_checks.check_sweeps(s, M, N, "three", SWEEPS)


@pytest.mark.parametrize("M,N", [(66, 49), GRID])
@pytest.mark.parametrize("K", [3 * 4 + 1, 3 * 4 + 2])
def test_partial_sweep(gpu, nat, M, N, K, monkeypatch):
    """An iteration cap inside a sweep: the last launch applies one or two
    iterations (identity steps after them).  w against the fp64 recurrence
    after K iterations, at the bound of the whole sweeps."""
    monkeypatch.setenv("PE_LAYOUT", "lpt")  # whole 48-row items
    s = sweep_checks.solver(nat, M, N, "three")
    if (M, N) == GRID:
        assert max(map(steady_groups, uniform_rows(s)), default=0) >= 1, s.layout_entries
    s.reset()
    s.run_iterations(K, False)
    s.synchronize()
    st = s.state()
    assert st["iter"] == K and st["status"] == 0, (st["iter"], st["status"])
    want = sweep_checks.reference("single", M, N, K).w[1:M, 1:N].numpy()
    dev = float(np.abs(s.w() - want).max() / np.abs(want).max())
    print(f"addr-partial {M}x{N} K={K} ti={s.ti} w_rel={dev:.2e}")
    assert dev <= F_TOL, dev


@pytest.mark.parametrize("M,N", [(66, 49), GRID])
@pytest.mark.parametrize("cap", [None, 3 * 10 + 1, 3 * 10 + 2])
def test_fixup_and_replay_norms(gpu, M, N, cap, monkeypatch):
    """A solve with the convergence test on (the fix-up launch when it stops
    inside a sweep) and solves capped on a sweep's first and second iteration:
    the replay launch then recomputes the recurrence's r of the returned w,
    and the end-of-solve figures are held to fp64 from that w."""
    monkeypatch.setenv("PE_LAYOUT", "lpt")  # whole 48-row items: steady groups on 260×97
    prob = EllipseProblem(M, N)
    if cap:
        prob.max_iter = cap
    rep = solve(prob, backend="hip", algo=THREE, return_w=True)
    assert rep.algo == THREE
    assert (rep.iters == cap and not rep.converged) if cap else rep.converged
    got = {k: getattr(rep, k) for k in ("res_true", "b_norm", "l2_err", "max_err", "max_outside", "res_rec", "res_gap")}
    check_norms(f"addr {M}x{N} cap={cap} iters={rep.iters}", prob, got, rep.w, True)


def test_push_variant_steady_against_generic(gpu, nat, monkeypatch):
    """kS3<PUSH>: rank 2 of a 4x1 split of 260×97 (65 rows, LEFT and RIGHT
    neighbours), the in-sweep push in loopback (PE_PUSH_LOOPBACK=1: the pushed
    rows land in the rank's own receive buffer and come back as its halo —
    the real stores and loads, not the neighbours' values, so no fp64
    reference applies).  At 13 rows per item the slab's last item is uniform:
    its one steady group loads the halo rows nx+1 .. nx+2 from the receive
    buffer by the halo's own row formula, and stores and pushes rows through
    the running bases.  At 12 rows no item has a steady group: the same job
    through the fill / drain addressing only.  The two layouts sum in another
    order and agree to the bound between layouts (1e-11 of max |w|, the sums
    to check_sweeps' bounds)."""
    M, N = GRID
    prob = EllipseProblem(M, N)
    blk = nat.decompose(M, N, D.grid(4, M, N, "4x1"), 2)
    monkeypatch.setenv("PE_PUSH_LOOPBACK", "1")
    monkeypatch.setenv("PE_HALO", "push")
    monkeypatch.setenv("PE_LAYOUT", "lpt")  # whole items
    out = {}
    for ti in (13, 12):
        monkeypatch.setenv("PE_TI", str(ti))
        opt = nat.SolveOptions()
        opt.algo = 4
        opt.check_tol = False
        comm = nat.make_delay_comm(4, 0.0, 0.0, True)
        s = nat.DeviceSolver(prob.to_native(), blk, comm, opt)
        assert s.sweep_steps == 3 and s.ti == ti
        assert s.halo_push and s.push_status.startswith("loopback"), (s.halo_path, s.push_status)
        nx = blk.nx
        last = [(ib, rows) for ib, rows, _s, flags in s.layout_entries if rows > 0 and flags & UNI_BIT and ib + rows - 1 == nx]
        if ti == 13:
            assert any(steady_groups(rows) >= 1 for _ib, rows in last), s.layout_entries
        else:
            assert max(map(steady_groups, uniform_rows(s)), default=0) == 0
        s.reset()
        s.run_iterations(3 * 4, False)
        s.synchronize()
        st = s.state()
        assert st["iter"] == 12 and st["status"] == 0, (st["iter"], st["status"])
        out[ti] = (st["fs2"][1], s.w())
        del s, comm
    (sa, wa), (sb, wb) = out[13], out[12]
    assert np.isfinite(wa).all() and np.abs(wb).max() > 0
    dev = float(np.abs(wa - wb).max() / np.abs(wb).max())
    print(f"addr-push w_rel={dev:.2e}")
    _, _, nsums, s_rel, s_abs, _, f_tol = sweep_checks.KINDS["three"]
    scale = max(abs(x) for x in sb)
    for n in range(nsums):
        assert sa[n] == pytest.approx(sb[n], rel=s_rel, abs=s_abs * scale), n
    assert dev <= f_tol, dev


def test_plane_offsets_beyond_4gib(gpu, nat):
    """16384²: the interleaved r / p rows (2 × 16432 doubles each: 342 strips)
    pass 4 GiB from their base in the block's last ≈50 rows — the one place where a
    32-bit row offset would show (it would wrap onto the first rows).  Two
    three-step sweeps against six iterations of the classic path on the same
    device, on the seeded node sample that `bench.py --dump-outputs` writes
    (one node in 64, ≈12000 of them in those rows), to 1e-10 of max |w|: the
    bound the project holds between sweep kinds.  The one long case of the
    sweep tests (two 16384² constructions)."""
    import bench

    M = N = 16384
    idx = np.random.default_rng(bench.DUMP_SAMPLE_SEED).integers(0, (M - 1) * (N - 1), size=bench.DUMP_SAMPLE_NODES,
                                                                 dtype=np.int64)
    idx.sort()
    first_past = (1 << 32) // (2 * 16432 * 8) + 1  # first local row wholly past 4 GiB of x
    assert int((idx // (N - 1) + 1 >= first_past).sum()) > 1000
    got = {}
    for algo in (4, 1):
        opt = nat.SolveOptions()
        opt.algo = algo
        opt.check_tol = False
        s = nat.DeviceSolver(EllipseProblem(M, N).to_native(), D.block(M, N, 1, 0), None, opt)
        assert algo == 1 or s.sweep_steps == 3
        s.reset()
        s.run_iterations(6, False)
        s.synchronize()
        st = s.state()
        assert st["iter"] == 6 and st["status"] == 0, (st["iter"], st["status"])
        got[algo] = s.w().reshape(-1)[idx]
        del s
    scale = float(np.abs(got[1]).max())
    dev = float(np.abs(got[4] - got[1]).max() / scale)
    print(f"addr-16384 w_rel={dev:.2e} max|w|={scale:.3e}")
    assert scale > 0 and dev <= 1e-10, dev
