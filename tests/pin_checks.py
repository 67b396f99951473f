"""The cases of test_sweep_pins.py: what each runs and which arrays it pins.

The three-step sweep's uniform march was changed without changing a single
floating-point operation or the order of a sum (the lateral differences are
taken from the neighbouring lane, the row coefficients once per item), so its
outputs are pinned bit for bit against fixtures recorded on the commit before
that change (tests/golden/sweep_pins/*.npz, written by
tools/record_sweep_pins.py).  A case returns a dict of arrays; the test
compares every one of them with np.array_equal.

Shapes — the smallest that reach each part of the uniform march:
  ref-40x200-K9 / K10   five strips, uniform items on inner and edge strips;
                        three whole sweeps, and a fourth applying one iteration
  cover-40x200          the covering ellipse on five strips: interior-class
                        uniform items on INNER strips (no lane mask), which the
                        reference problem holds only on large grids — fill,
                        five steady groups, drain
  cover-ti7 .. ti96     130×97 under the covering ellipse (uniform items
                        only), whole items (LPT layout) of 7 rows (fill and
                        drain steps only), 13 (one steady group), 19 (two) and
                        96 (past the first 64-row class window inside steady
                        groups)
  offc / cut_y          130×97, whole 48-row items: uniform items (six steady
                        groups) next to band items, interior coefficients next
                        to the box edge
  solve-*               converged solves: the launch that resolves the stop
                        test, the fix-up and the replay; iteration count, w
                        and the recurrence's residual norm.  (The reference
                        problem at 130×97 — two strips over the whole y range
                        — has a band node in every row and no uniform item
                        under any layout: it pins the kernel's other kinds
                        through the same launches; the covering ellipse at
                        66×49 is uniform items only.)
  push-loop-ti13        kS3<PUSH>: rank 2 of a 4x1 split of 260×97 with the
                        in-sweep push in loopback, a 13-row uniform last item
                        (the push variant's steady group)
  push-3proc            three processes, row slabs of 12 rows of 37×1000 on
                        the host-staged transport, push forced: the gathered w
                        (12 rows are fill and drain steps only; strips past
                        |y| = 0.5 hold uniform items)
"""

import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_pins")
UNI_BIT = sweep_checks.UNI_BIT
THREE = "three-step"

# (rows per item and layout forced: a list the construction's timing cannot change)
# name -> (M, N, member, iterations, environment, steady groups a uniform item must reach (None: any uniform item))
SWEEPS = {
    "ref-40x200-K9": (40, 200, None, 9, {"PE_TI": "48"}, None),
    "ref-40x200-K10": (40, 200, None, 10, {"PE_TI": "48"}, None),
    "cover-40x200": (40, 200, "cover", 9, {"PE_TI": "48", "PE_LAYOUT": "lpt"}, 5),
    "cover-ti7": (130, 97, "cover", 9, {"PE_TI": "7", "PE_LAYOUT": "lpt"}, 0),
    "cover-ti13": (130, 97, "cover", 9, {"PE_TI": "13", "PE_LAYOUT": "lpt"}, 1),
    "cover-ti19": (130, 97, "cover", 9, {"PE_TI": "19", "PE_LAYOUT": "lpt"}, 2),
    "cover-ti96": (130, 97, "cover", 9, {"PE_TI": "96", "PE_LAYOUT": "lpt"}, 14),
    "offc-130x97": (130, 97, "offc", 9, {"PE_TI": "48", "PE_LAYOUT": "lpt"}, 6),
    "cut_y-130x97": (130, 97, "cut_y", 9, {"PE_TI": "48", "PE_LAYOUT": "lpt"}, 6),
}
# name -> (M, N, member, the list holds uniform items)
SOLVES = {"solve-ref-130x97": (130, 97, None, False), "solve-cover-66x49": (66, 49, "cover", True)}
PUSH_LOOP = "push-loop-ti13"
PUSH_PROC = "push-3proc"
NAMES = list(SWEEPS) + list(SOLVES) + [PUSH_LOOP, PUSH_PROC]

TUNING = ("PE_HALO", "PE_OVERLAP", "PE_STEPS", "PE_TI", "PE_TI_TUNE", "PE_LAYOUT", "PE_PUSH_LOOPBACK")


@contextlib.contextmanager
def environment(env):
    """The tuning variables set to `env` and nothing else, restored afterwards."""
    old = {k: os.environ.get(k) for k in TUNING}
    for k in TUNING:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def steady_groups(rows):
    """Steady six-step groups of a uniform item of `rows` rows (march3)."""
    return 0 if rows < 13 else (rows - 1 - 12) // 6 + 1


def uniform_rows(entries):
    return [rows for _ib, rows, _strip, flags in entries if rows > 0 and flags & UNI_BIT]


def _planes(s, M, N):
    st = s.state()
    par = int(st["wpar"])
    return st, {"r": np.array(s.field(0 if par == 0 else 4)[2:M + 1, 2:N + 1]),
                "p": np.array(s.field(2 if par == 0 else 3)[2:M + 1, 2:N + 1]),
                "w": np.array(s.w()), "sums": np.array(st["fs2"][par][:19], dtype=np.float64)}


def run_sweeps(nat, name):
    M, N, member, K, env, groups = SWEEPS[name]
    with environment(env):
        s = sweep_checks.solver(nat, M, N, "three", member)
        assert s.sweep_steps == 3
        uni = uniform_rows(s.layout_entries)
        assert uni, (name, "no uniform item in the list")
        if "PE_TI" in env:
            assert s.ti == int(env["PE_TI"])
        if "PE_LAYOUT" in env:
            assert s.layout_name == env["PE_LAYOUT"]
        if groups is not None:
            assert max(map(steady_groups, uni)) == groups, (name, sorted(uni))
        if name == "cover-ti96":
            assert max(uni) + 12 > 64  # the march passes the first class window inside steady groups
        s.reset()
        s.run_iterations(K, False)
        s.synchronize()
        st, out = _planes(s, M, N)
        assert st["iter"] == K and st["status"] == 0, (st["iter"], st["status"])
    return out


def run_solve(nat, name):
    M, N, member, has_uniform = SOLVES[name]
    with environment({"PE_TI": "48", "PE_LAYOUT": "lpt"}):  # whole 48-row items: steady groups
        s = sweep_checks.solver(nat, M, N, "three", member)
        uni = uniform_rows(s.layout_entries)
        assert bool(uni) == has_uniform and (not uni or max(map(steady_groups, uni)) >= 1), (name, sorted(uni))
        del s
        rep = solve(sweep_checks.problem(M, N, member), backend="hip", algo=THREE, return_w=True)
    assert rep.algo == THREE and rep.converged
    return {"iters": np.array([rep.iters], dtype=np.int64), "w": np.array(rep.w),
            "res_rec": np.array([rep.res_rec], dtype=np.float64)}


def run_push_loop(nat):
    M, N = 261, 98
    prob = sweep_checks.problem(M, N)
    blk = nat.decompose(M, N, D.grid(4, M, N, "4x1"), 2)
    with environment({"PE_PUSH_LOOPBACK": "1", "PE_HALO": "push", "PE_LAYOUT": "lpt", "PE_TI": "13"}):
        opt = nat.SolveOptions()
        opt.algo = 4
        opt.check_tol = False
        comm = nat.make_delay_comm(4, 0.0, 0.0, True)
        s = nat.DeviceSolver(prob.to_native(), blk, comm, opt)
        assert s.sweep_steps == 3 and s.ti == 13
        assert s.halo_push and s.push_status.startswith("loopback"), (s.halo_path, s.push_status)
        last = [rows for ib, rows, _s, flags in s.layout_entries if rows > 0 and flags & UNI_BIT and ib + rows - 1 == blk.nx]
        assert any(steady_groups(rows) >= 1 for rows in last), s.layout_entries
        s.reset()
        s.run_iterations(9, False)
        s.synchronize()
        st = s.state()
        assert st["iter"] == 9 and st["status"] == 0, (st["iter"], st["status"])
        out = {"w": np.array(s.w()), "sums": np.array(st["fs2"][int(st["wpar"])][:19], dtype=np.float64)}
        del s, comm
    return out


def run_push_proc(nat, tmp_path):
    from conftest import free_port

    M, N, nproc, K = 37, 1000, 3, 9
    # the slabs' lists, from the host planner: 12 rows each, uniform items on the strips outside the ellipse
    for rank in range(nproc):
        blk = nat.decompose(M, N, D.grid(nproc, M, N, "rows"), rank)
        assert blk.nx == 12
        lay = nat.item_layout(sweep_checks.problem(M, N).to_native(), blk, 3, 48, layout="equal")
        assert uniform_rows(lay["entries"]), rank
    outp = os.path.join(str(tmp_path), "w.npy")
    base = {k: v for k, v in os.environ.items() if k not in TUNING}
    env = dict(base, PE_COMM="host", PE_ALLREDUCE="p2p", PE_P2P_TIMEOUT_S="60", PE_XR="1", PE_HALO="push", PE_OVERLAP="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "poisson_ellipse_openmp_mpi_cuda_amd",
           "--json", "--quiet", "--decomp", "rows", "--algo", "auto", "--max-iter", str(K), "--dump", outp, str(M), str(N)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["ranks"] == nproc and d["Px"] == nproc and d["Py"] == 1, d
    assert d["algo"] == THREE and d["iters"] == K and not d["converged"], d
    assert d["halo_push"] and d["halo_path"].startswith("push") and d["push_status"] == "available", d
    assert d["comm"] == "p2p-allreduce+host-staged", d["comm"]
    return {"w": np.load(outp)}


def run_case(nat, name, tmp_path):
    if name in SWEEPS:
        return run_sweeps(nat, name)
    if name in SOLVES:
        return run_solve(nat, name)
    if name == PUSH_LOOP:
        return run_push_loop(nat)
    assert name == PUSH_PROC
    return run_push_proc(nat, tmp_path)


def fixture_path(name):
    return os.path.join(GOLDEN, name + ".npz")
