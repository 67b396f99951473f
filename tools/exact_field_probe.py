"""Cost of the end-of-solve error pass against a user exact solution given as
a GPU tensor (docs/PERFORMANCE.md "Fields in device memory").

    python tools/exact_field_probe.py M [plain|exact|both]

One process: a DeviceSession at M × M capped at 9 iterations, rhs = 1 + x + y
and exact = (1 − x² − 4y²)(1/10 + x/14 + y/26) computed on the GPU, then
solves alternating without (`plain`: rhs alone, no error pass input) and with
`exact` (one kSliceField<double, 0> + kErrorField instead of nothing: with a
user rhs the plain solve still runs kError, whose figures are dropped).  Per
solve: hipEvent time around session.solve() on the current stream and
timers["solver"]; the medians and their difference are printed as one JSON
line.  Run it under `rocprofv3 --kernel-trace --stats` (a run of its own) for
kError / kErrorField / kSliceField themselves."""

import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem  # noqa: E402


def main(argv) -> int:
    M, variant = int(argv[1]), argv[2] if len(argv) > 2 else "both"
    if variant not in ("plain", "exact", "both"):
        raise SystemExit(__doc__)
    prob = EllipseProblem(M, M)
    prob.max_iter = 9
    x = torch.from_numpy(prob.A1 + np.arange(1, M, dtype=np.float64) * prob.h1).cuda()[:, None]
    y = torch.from_numpy(prob.A2 + np.arange(1, M, dtype=np.float64) * prob.h2).cuda()[None, :]
    f = 1.0 + x + y
    u = (1.0 - x * x - 4.0 * y * y) * (0.1 + x / 14.0 + y / 26.0)
    session = DeviceSession(prob)
    runs = {"plain": dict(rhs=f), "exact": dict(rhs=f, exact=u)}
    names = [n for n in runs if variant in (n, "both")]
    ev, solver, rep = {n: [] for n in names}, {n: [] for n in names}, None
    for k in range(8):
        for n in names:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            rep = session.solve(**runs[n])
            b.record()
            torch.cuda.synchronize()
            if k >= 2:  # (two warm-up rounds: lazy kernel loading, the first plane's allocation)
                ev[n].append(a.elapsed_time(b))
                solver[n].append(1e3 * (rep.timers["solver"] - rep.timers["construct"]))
    out = dict(M=M, algo=rep.algo, iters=rep.iters, l2_err=rep.l2_err)
    for n in names:
        out[n] = dict(event_ms=round(statistics.median(ev[n]), 4), solver_ms=round(statistics.median(solver[n]), 4))
    if len(names) == 2:
        out["exact_minus_plain_event_ms"] = round(out["exact"]["event_ms"] - out["plain"]["event_ms"], 4)
    session.close()
    print("PROBE " + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
