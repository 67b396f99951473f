"""Cost of the gradient pass (DeviceSolver.gradient_device, kGradField) next to
the end-of-solve residual pass (docs/PERFORMANCE.md "The gradient pass").

    python tools/gradient_probe.py M [check]

One process: a DeviceSession at M × M capped at 9 iterations.  Per round one
session.solve() (its timers["check"] is the residual pass: kWtoP + kResid and
the state read), then the solver's gradient_device into a preallocated
(2, M−1, M−1) tensor (STORE) and, after another solve, without destinations
(the functionals only).  Each call is timed on the host between two device
synchronisations (the call ends with its own state read) and by events on the
current stream; medians of 6 rounds after 2 warm-up rounds, one JSON line.
`check`: only the solves and timers["check"] — what a build without the
gradient can run.  Run it under `rocprofv3 --kernel-trace --stats` (a run of
its own) for kGradField / kWtoP / kResid themselves."""

import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0), a.elapsed_time(b)


def main(argv) -> int:
    M, check_only = int(argv[1]), len(argv) > 2 and argv[2] == "check"
    prob = EllipseProblem(M, M)
    prob.max_iter = 9
    session = DeviceSession(prob)
    s = session.solver
    g = None if check_only else torch.empty((2, M - 1, M - 1), dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    t = {k: [] for k in ("check", "store_wall", "store_event", "stats_wall", "stats_event")}
    rep = stats = None
    for k in range(8):
        rep = session.solve()
        rows = {"check": 1e3 * rep.timers["check"]}
        if not check_only:
            stats, rows["store_wall"], rows["store_event"] = timed(
                lambda: s.gradient_device(g[0].data_ptr(), g[1].data_ptr(), g.stride(1), g.stride(2), 0, 0, stream))
            session.solve()
            only, rows["stats_wall"], rows["stats_event"] = timed(lambda: s.gradient_device(0, 0, 0, 0, 0, 0, 0))
            assert only == stats, (only, stats)
        if k >= 2:  # (two warm-up rounds: lazy kernel loading)
            for name, v in rows.items():
                t[name].append(v)
    nodes = (M - 1) * (M - 1)
    out = dict(M=M, algo=rep.algo, iters=rep.iters, nodes=nodes, stats=stats,
               bytes_per_node=dict(kWtoP=16, kGradField_store=24, kGradField_stats=8, kResid=24))
    for name, v in t.items():
        if v:
            out[name + "_ms"] = round(statistics.median(v), 4)
    session.close()
    print("PROBE " + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
