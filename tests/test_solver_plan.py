"""CPU tests of the host-only solver plan (csrc/core/solver_plan.cpp:
native.solver_plan / resident_tiling / halo_candidates).  What a DeviceSolver
decides for a block — kernel family, iterations per sweep, rows per item,
order, tuning, chunk — is pinned against tests/golden/solver_plans.json,
recorded from live solvers on an MI355X on the commit before those decisions
moved out of the constructor (tools/record_solver_plans.py), and against the
requests of tests/golden/layouts.json.  No device is needed."""

import json
import os
import shutil
import subprocess

import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "solver_plans.json")) as _f:
    PLANS = json.load(_f)
RECORDS = {r["name"]: r for r in PLANS["records"]}
with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as _f:
    LAYOUTS = {c["name"]: c for c in json.load(_f)["cases"]}

KNOBS = {"PE_RESIDENT": "pe_resident", "PE_STEPS": "pe_steps", "PE_TI": "pe_ti", "PE_ORDER": "pe_order",
         "PE_TI_TUNE": "pe_ti_tune"}


def _plan(nat, M, N, P, spec, rank, comm_size, algo=0, variant=0, shift=0.0, chunk=0, env=None, prob=None, **kw):
    if prob is None:
        prob = EllipseProblem(M, N, shift=shift).to_native()
    blk = nat.decompose(M, N, D.grid(P, M, N, spec), rank)
    opt = nat.SolveOptions()
    opt.algo, opt.variant, opt.chunk = algo, variant, chunk
    knobs = {KNOBS[k]: int(v) for k, v in (env or {}).items() if k in KNOBS}
    return blk, nat.solver_plan(prob, blk, comm_size, opt, **knobs, **kw)


def _facts(obs):
    """The device facts a record's solver had: the CU count and the blocks per
    CU its wave caps came from (4 waves per block)."""
    if "wave_caps" not in obs:
        return {}
    cus = obs["cus"]
    return dict(cus=cus, per_cu=obs["wave_caps"][0] // (4 * cus), per_cu0=obs["wave_caps"][1] // (4 * cus))


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_recorded_decisions(nat, name):
    """Field for field what the live solver decided before the split."""
    r = RECORDS[name]
    obs = r["observed"]
    blk, pl = _plan(nat, r["M"], r["N"], r["P"], r["spec"], r["rank"], r["comm_size"], r["algo"], r["variant"], r["shift"],
                    r.get("chunk", 0), r["env"], resident=obs["resident"], **_facts(obs))
    assert (blk.nx, blk.ny) == (obs["nx"], obs["ny"])
    assert (pl["fused"], pl["steps"], pl["order"], pl["chunk"], pl["strips"]) == \
        (obs["fused"], obs["steps"], obs["order"], obs["chunk"], obs["strips"])
    assert not obs["resident"] or pl["resident_likely"]
    # the tuning runs where the plan asks for it and the resident kernel does not take the block
    assert (pl["tune_ti"] and not obs["resident"]) == obs["tuned"]
    if "wave_caps" in obs:
        assert list(pl["wave_caps"]) == obs["wave_caps"]
    if obs["tuned"]:
        assert pl["candidates"] == obs["candidates"]
        return
    assert (pl["ti"], pl["layout"]) == (obs["ti"], obs["layout_name"])
    if "request_layout" in obs:
        assert pl["layout"] == obs["request_layout"]
        # the list the planner lays out for the plan: its item-sum slots and grid
        lay = nat.item_layout(EllipseProblem(r["M"], r["N"]).to_native(), blk, pl["steps"], pl["ti"], order=pl["order"],
                              layout=pl["layout"], wave_caps=tuple(pl["wave_caps"]), cus=obs["cus"])
        assert (lay["nslots"], lay["nblocks"]) == (obs["nitems"], obs["blocks"])


def test_records_sit_on_both_sides_of_every_threshold():
    """The fixture's coverage, so a re-recording cannot quietly drop a side."""
    o = {n: r["observed"] for n, r in RECORDS.items()}
    assert (o["single-7-nores"]["steps"], o["single-8-nores"]["steps"]) == (1, 3)
    assert [o[f"slab4-{m}"]["steps"] for m in (31, 32, 45, 48)] == [1, 2, 2, 3]
    assert [o[f"2x2-{k}-{m}"]["steps"] for k in ("comm", "virtual") for m in (24, 25)] == [1, 3, 1, 3]
    assert not o["slab4-one-row"]["fused"] and not o["variant1"]["fused"] and not o["shift40"]["fused"]
    assert [o[f"algo{a}-40"]["steps"] for a in (1, 2, 3, 4)] == [1, 1, 2, 3]
    assert [o[f"slab4-48-steps{s}"]["steps"] for s in (1, 2)] == [1, 2]
    assert o["400x600"]["resident"] and o["800x1200"]["resident"] and not o["1600x2400"]["resident"]
    assert (o["tile-64"]["steps"], o["tile-65"]["steps"]) == (1, 3)  # (the estimate holds 64 rows per tile, not 65)
    assert not o["400x600-nores"]["resident"] and o["400x600-nores"]["steps"] == 3
    assert not o["2p20-less"]["tuned"] and o["2p20-tuned"]["tuned"] and o["2p24-tuned"]["tuned"]
    assert (o["2p24-less-algo0"]["ti"], o["2p24-algo0"]["ti"]) == (48, 80)
    assert (o["2p24-less-algo2"]["ti"], o["2p24-algo2"]["ti"]) == (10, 24)
    assert (o["2p24-less-algo3"]["ti"], o["2p24-algo3"]["ti"]) == (24, 40)
    assert o["ti13-algo2"]["ti"] == 13 and o["bands-algo2"]["ti"] == 1
    assert (o["order3-single"]["order"], o["order3-three"]["order"]) == (3, 0)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layout_cases_follow_the_plan(nat, name):
    """The live solvers of tests/golden/layouts.json: rows per item, order,
    iterations per sweep and the starting layout name of their requests.
    (Every one of them was recorded with PE_TI set: the untuned heights of the
    large classes are pinned through test_untuned_heights_by_size below.)"""
    c = LAYOUTS[name]
    q = c["request"]
    cus = q["cus"]
    _, pl = _plan(nat, c["M"], c["N"], c["P"], c["spec"], c["rank"], c["P"], c["algo"], env=c["env"], cus=cus,
                  per_cu=q["wave_caps"][0] // (4 * cus), per_cu0=q["wave_caps"][1] // (4 * cus))
    assert (pl["steps"], pl["ti"], pl["order"], pl["layout"], list(pl["wave_caps"])) == \
        (c["steps"], c["ti"], c["order"], q["layout"], q["wave_caps"])
    assert not pl["tune_ti"]


@pytest.mark.parametrize("M,N,algo,ti,layout,order", [
    (8192, 8192, 4, 112, "lpt", 0),      # >= 2^25 and >= 5e7 nodes
    (5794, 5794, 4, 112, "fill", 0),     # 2^25 <= 3.36e7 < 5e7
    (5001, 5001, 4, 80, "fill", 0),      # 2.5e7 nodes: the filling layout starts
    (5000, 5001, 4, 80, "equal", 0),     # just under
    (8193, 8193, 4, 112, "lpt", 0),      # 2^26 nodes is not yet "huge" ...
    (8193, 8193, 2, 24, "lpt", 0),
    (8194, 8193, 4, 448, "lpt", 0),      # ... one row more is
    (8194, 8193, 2, 18, "lpt", 3),
    (8194, 8193, 3, 40, "lpt", 0),
])
def test_untuned_heights_by_size(nat, M, N, algo, ti, layout, order):
    """The size classes above the recorded ones, from the constructor's table:
    three-step 48 / 80 (2^24) / 112 (2^25) / 448 (> 2^26) rows, two-step 24 /
    40, single sweep 10 / 24 / 18 with the dynamic order past 2^26; the
    three-step layout equal / fill (2.5e7) / lpt (5e7).  tests/golden/
    layouts.json holds 8192^2 at 112 rows on the lpt layout from a live solver."""
    _, pl = _plan(nat, M, N, 1, "device", 0, 1, algo, env={"PE_TI_TUNE": "0"})
    assert (pl["ti"], pl["order"]) == (ti, order)
    if algo == 4:
        assert pl["layout"] == layout


SPLITS = [(3, "rows"), (4, "rows"), (4, "2x2"), (6, "2x3"), (8, "4x2")]


@pytest.mark.parametrize("M,N", [(46, 46), (49, 98), (131, 98)])
@pytest.mark.parametrize("P,spec", SPLITS)
@pytest.mark.parametrize("comm", [True, False])
def test_every_rank_decides_the_same(nat, M, N, P, spec, comm):
    """fused and steps come from global inputs only: ranks that disagreed
    would run different kernels against each other's halos."""
    got = {(pl["fused"], pl["steps"]) for pl in (_plan(nat, M, N, P, spec, r, P if comm else 1)[1] for r in range(P))}
    assert len(got) == 1, got


def test_recorded_multi_rank_blocks_decide_the_same_on_every_rank(nat):
    for r in RECORDS.values():
        if r["P"] == 1:
            continue
        got = {(pl["fused"], pl["steps"]) for pl in
               (_plan(nat, r["M"], r["N"], r["P"], r["spec"], k, r["comm_size"], r["algo"], r["variant"], r["shift"],
                      env=r["env"])[1] for k in range(r["P"]))}
        assert got == {(r["observed"]["fused"], r["observed"]["steps"])}, r["name"]


def test_uneven_slab_is_two_step_on_every_rank(nat):
    """45 rows over 4 ranks: 12 / 11 / 11 / 11 — the rank with 12 rows must not take the three-step sweep alone."""
    blocks = [_plan(nat, 46, 40, 4, "rows", r, 4) for r in range(4)]
    assert [b.nx for b, _ in blocks] == [12, 11, 11, 11]
    assert [pl["steps"] for _, pl in blocks] == [2, 2, 2, 2]


# ---- the halo-path candidates --------------------------------------------------------------------------------------

EX, PUT, PUSH = "exchange", "put", "push"


def _cands(nat, **kw):
    l, late = nat.halo_candidates(**kw)
    return [tuple(c) for c in l], late


def test_halo_candidates_pins(nat):
    h3 = [64, 80, 96]
    # 8-rank slab, everything available: the put's overlap is timed late, at the exchange overlap's best height
    assert _cands(nat, steps=3, put_ok=True, push_ok=True, nheights=3, heights=h3) == \
        ([(EX, False, 0), (PUT, False, 0), (PUSH, False, 0), (EX, True, 64), (EX, True, 80), (EX, True, 96)], True)
    # 2-D split: no push
    assert _cands(nat, steps=3, put_ok=True, nheights=1, heights=[48]) == \
        ([(EX, False, 0), (PUT, False, 0), (EX, True, 48)], True)
    assert _cands(nat, steps=3, put_ok=True, push_ok=True, nheights=3, heights=h3, pe_overlap=0) == \
        ([(EX, False, 0), (PUT, False, 0), (PUSH, False, 0)], False)
    # (PE_HALO=push: the put is not set up)
    assert _cands(nat, steps=3, push_ok=True, nheights=3, heights=h3, pe_halo="push") == ([(PUSH, False, 0)], False)
    # the delay transport of the one-process tests: neither put nor push
    assert _cands(nat, steps=1, nheights=1, heights=[10]) == ([(EX, False, 0), (EX, True, 10)], False)
    # a rank with fewer heights than the job agreed on times the construction's (0) for the rest
    assert _cands(nat, steps=3, nheights=3, heights=[48]) == \
        ([(EX, False, 0), (EX, True, 48), (EX, True, 0), (EX, True, 0)], False)


def test_halo_candidates_rules(nat):
    h = [48, 64]
    # the forced path is unavailable: the exchange (overlapped at every height when PE_OVERLAP=1)
    assert _cands(nat, steps=3, nheights=2, heights=h, pe_halo="put") == ([(EX, False, 0)], False)
    assert _cands(nat, steps=3, nheights=2, heights=h, pe_halo="put", pe_overlap=1) == \
        ([(EX, True, 48), (EX, True, 64)], False)
    # PE_OVERLAP=1 drops the push (it never overlaps)
    l, late = _cands(nat, steps=3, put_ok=True, push_ok=True, nheights=2, heights=h, pe_overlap=1)
    assert l == [(EX, True, 48), (EX, True, 64)] and late
    # ranks sharing a GPU: no put+overlap unless both are forced
    l, late = _cands(nat, steps=3, put_ok=True, shared_dev=True, nheights=2, heights=h)
    assert l == [(EX, False, 0), (PUT, False, 0), (EX, True, 48), (EX, True, 64)] and not late
    assert _cands(nat, steps=3, put_ok=True, shared_dev=True, nheights=2, heights=h, pe_halo="put", pe_overlap=1) == \
        ([(PUT, True, 48), (PUT, True, 64)], False)
    assert _cands(nat, steps=3, put_ok=True, nheights=2, heights=h, pe_halo="put") == \
        ([(PUT, False, 0), (PUT, True, 48), (PUT, True, 64)], False)


@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("put_ok", [False, True])
@pytest.mark.parametrize("push_ok", [False, True])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("halo", [None, "exchange", "put", "push"])
@pytest.mark.parametrize("ov", [None, 0, 1])
def test_halo_candidates_invariants(nat, steps, put_ok, push_ok, shared, halo, ov):
    for nh in (1, 3):
        kw = dict(steps=steps, put_ok=put_ok, push_ok=push_ok, shared_dev=shared, nheights=nh, heights=[40, 56, 72][:nh],
                  pe_halo=halo, pe_overlap=ov)
        l, late = _cands(nat, **kw)
        assert (l, late) == _cands(nat, **kw) and l  # a function of its inputs only; never empty
        flags = [c[1] for c in l]
        assert flags == sorted(flags)  # the plain candidates precede the overlapped ones
        if steps == 2:
            assert not any(flags) and not late  # no boundary-item signal in the two-step sweep
        for path in (EX, PUT):  # as many overlapped entries per path as heights agreed
            n = sum(1 for c in l if c[0] == path and c[1])
            assert n in (0, nh)
        assert all(c[2] == 0 for c in l if not c[1])
        if ov == 1:
            assert all(c[0] != PUSH for c in l)
        if shared and not (halo == "put" and ov == 1):
            assert (PUT, True) not in [(c[0], c[1]) for c in l] and not late
        if late:
            assert l[-1][0] == EX and l[-1][1]


# ---- the resident tile geometry ----------------------------------------------------------------------------------------

def _old_estimate(nx, ny, cus):
    """The constructor's resident_likely before the split, verbatim (PE_RESIDENT and the variant apart)."""
    ns = (ny + 124 - 1) // 124
    if ns <= cus:
        ntr = max(1, min(cus // ns, nx // 8))
        return nx >= 2 * ntr and (nx + ntr - 1) // ntr <= 64 and ntr * ns <= 256
    return False


def _old_setup(nx, ny, cus):
    """setup_resident's geometry before the split, verbatim: (strips, bands, rowstart, rcap) or None."""
    nstrips = (ny + 124 - 1) // 124  # (KParams::nstrips of the single sweep)
    if nstrips > cus:
        return None
    ntr = max(1, min(cus // nstrips, nx // 8))
    if nx < 2 * ntr:
        return None
    rs = [1 + t * nx // ntr for t in range(ntr + 1)]
    rcap = 0
    for t in range(ntr):
        rcap = max(rcap, rs[t + 1] - rs[t])
    if rcap > 64:
        return None
    return nstrips, ntr, rs, rcap


SWEEP = sorted(set(range(1, 141)) | set(range(1, 2001, 53)) | {2000})


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_resident_tiling_agrees_with_both_former_copies(nat, cus):
    bad = []
    for nx in SWEEP:
        for ny in SWEEP:
            t = nat.resident_tiling(nx, ny, cus)
            got = None if t is None else (t["strips"], t["bands"], t["rowstart"], t["rcap"])
            if got != _old_setup(nx, ny, cus) or (got is not None and got[0] * got[1] <= 256) != _old_estimate(nx, ny, cus):
                bad.append((nx, ny))
    assert not bad, bad[:20]


def test_resident_estimate_in_the_plan(nat):
    for M, N, want in ((400, 600, True), (800, 1200, True), (1600, 2400, False), (1601, 1200, True), (1602, 1200, False)):
        assert _plan(nat, M, N, 1, "device", 0, 1)[1]["resident_likely"] == want, (M, N)
        assert _plan(nat, M, N, 1, "device", 0, 1)[1]["resident_likely"] == _old_estimate(M - 1, N - 1, 256)
    assert not _plan(nat, 400, 600, 1, "device", 0, 1, env={"PE_RESIDENT": "0"})[1]["resident_likely"]
    assert _plan(nat, 400, 600, 1, "device", 0, 1, env={"PE_RESIDENT": "1"})[1]["resident_likely"]
    assert not _plan(nat, 400, 600, 1, "device", 0, 1, variant=1)[1]["resident_likely"]


# ---- refusals --------------------------------------------------------------------------------------------------------

ALGO = "algo: 0 auto, 1 classic, 2 fused, 3 two-step, 4 three-step (got {})"
SHIFT = "DeviceSolver: shift must be finite and >= 0 (got -1.000000): a negative shift makes the system indefinite"
SHIFTED = ("algo fused / two-step / three-step: the single-sweep kernels implement the unshifted operator only; a problem "
           "with shift != 0 (got 40.000000) runs algo auto or classic")
SINGLE = "single-sweep algorithm needs variant 0 and >= 2 rows/columns per split block"
TWO = "two-step sweep: single-rank blocks of >= 8 x 8 nodes or row slabs of >= 8 rows"
THREE = "three-step sweep: single-rank blocks of >= 8 x 8 nodes, row slabs of >= 12 rows or 2-D blocks of >= 12 x 12"


def _refusal(nat, M, N, P=1, spec="device", comm_size=1, shift=0.0, **kw):
    prob = EllipseProblem(M, N).to_native()
    prob.shift = shift  # (past the Python model's own check)
    with pytest.raises(ValueError) as e:
        _plan(nat, M, N, P, spec, 0, comm_size, prob=prob, **kw)
    return str(e.value)


def test_refusals_and_their_order(nat):
    assert _refusal(nat, 40, 40, algo=5) == ALGO.format(5)
    assert _refusal(nat, 40, 40, algo=-1) == ALGO.format(-1)
    assert _refusal(nat, 40, 40, shift=-1.0) == SHIFT
    assert _refusal(nat, 40, 40, shift=40.0, algo=2) == SHIFTED
    assert _refusal(nat, 40, 40, algo=2, variant=1) == SINGLE
    assert _refusal(nat, 8, 40, 4, "rows", 4, algo=2) == SINGLE  # one row per block
    assert _refusal(nat, 8, 8, algo=3) == TWO  # 7 x 7 nodes
    assert _refusal(nat, 32, 40, 4, "rows", 4, algo=3) == TWO  # slabs of 7 rows
    assert _refusal(nat, 8, 8, algo=4) == THREE
    assert _refusal(nat, 46, 40, 4, "rows", 4, algo=4) == THREE  # slabs of 11 rows
    assert _refusal(nat, 24, 24, 4, "2x2", 4, algo=4) == THREE  # 2-D blocks of 11
    assert _refusal(nat, 24, 24, 4, "2x2", 1, algo=4) == THREE  # the same as virtual ranks
    assert _refusal(nat, 25, 25, 4, "2x2", 4, algo=3) == TWO  # the two-step sweep takes no 2-D split
    # two conditions violated: the first in the constructor's order
    assert _refusal(nat, 40, 40, shift=-1.0, algo=7) == ALGO.format(7)
    assert _refusal(nat, 40, 40, shift=-1.0, algo=2) == SHIFT
    assert _refusal(nat, 40, 40, shift=40.0, algo=3, variant=1) == SHIFTED
    assert _refusal(nat, 8, 8, algo=4, variant=1) == SINGLE
    assert _refusal(nat, 8, 8, algo=3, variant=1) == SINGLE


@pytest.fixture(scope="module")
def plan_asan():
    if shutil.which("make") is None or shutil.which("g++") is None:
        pytest.skip("no host toolchain")
    r = subprocess.run(["make", "-s", "bin/pe_plan_asan"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return os.path.join(ROOT, "bin", "pe_plan_asan")


def _asan_run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out
    return out


def test_plan_asan_ubsan_clean(nat, plan_asan):
    """The plan as a stand-alone program built with ASan + UBSan from the host
    sources alone: the tiling's row-start arrays and the candidate lists over
    the sweep of shapes and inputs, and three recorded blocks whose printed
    decisions are the fixture's."""
    out = _asan_run(plan_asan, "sweep")
    n = sum(1 for cus in (64, 256, 304) for nx in SWEEP for ny in SWEEP if nat.resident_tiling(nx, ny, cus) is not None)
    assert f"tilings {n} " in out
    for name, knobs in (("2p24-tuned", ()), ("slab4-48-steps2", ("-", 2)), ("bands-algo2", (0, "-", -1))):
        r, o = RECORDS[name], RECORDS[name]["observed"]
        out = _asan_run(plan_asan, r["M"], r["N"], r["P"], r["spec"], r["rank"], r["comm_size"], r["algo"], 256, 2, 2, *knobs)
        assert f" steps {o['steps']} " in out and f" strips {o['strips']} " in out and f" chunk {o['chunk']}" in out
        if o["tuned"]:
            assert "[" + ",".join(str(c) for c in o["candidates"]) + "]" in out
        else:
            assert f" ti {o['ti']} " in out


def test_algo_names(nat):
    """SolveResult::algo of the solve and of the group driver."""
    names = {(a, res): _plan(nat, 400, 600, 1, "device", 0, 1, a, resident=res)[1]["algo"] for a in (1, 2, 3, 4)
             for res in (False, True)}
    assert [names[a, False] for a in (1, 2, 3, 4)] == ["classic", "fused", "two-step", "three-step"]
    assert names[2, True] == "resident"
