"""Command-line front end (Python).  Positional ``M N`` as in the reference
(``prog [M N]``, default 40 40: stage2-mpi/poisson_mpi_decomp.cpp:470-474).

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli 800 1200                    # 1 GPU
    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --backend omp --threads 8 400 600
    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --backend ranks --ranks 4 --threads 2 800 1200
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m poisson_ellipse_openmp_mpi_cuda_amd.cli 8192 8192
    torchrun --nproc-per-node 4 --master-addr 127.0.0.1 -m poisson_ellipse_openmp_mpi_cuda_amd.cli --backend dist-cpu 400 600

Prints the reference's result lines (``--legacy``, default) and/or a JSON
report (``--json``), the L2/max error against the analytic solution, and
optionally dumps w (``--dump w.npy``, plus ``--pgm w.pgm``).

``--rhs FILE.npy`` / ``--w0 FILE.npy`` solve for a user right-hand side from
a user initial guess: float64 arrays of the global interior, shape
(M-1, N-1), entry [i-1, j-1] at node (x_i, y_j) — what ``--dump`` writes, so
the dump of one run is a valid ``--w0`` of the next:

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --rhs f.npy --dump w.npy 400 600
    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --rhs f.npy --w0 w.npy 400 600

``--exact FILE.npy`` (same form) is the solution the reported L2 / max error
is measured against inside the ellipse, e.g. a manufactured u with
``--rhs`` = −Δu; with ``--rhs`` alone the error line reads ``n/a``:

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --rhs f.npy --exact u.npy 400 600

``--dump-grad FILE.npy`` writes the gradient of w inside the ellipse, float64
of shape (2, M-1, N-1), [0] = d/dx, [1] = d/dy (one-sided differences at the
boundary of the ellipse, 0 outside); ``--grad-stats`` prints h1 h2 Σ_D w,
h1 h2 Σ_D |∇w|² and max_D |∇w| on a line of their own after the result lines
(``--json`` carries them as ``integral``, ``energy``, ``grad_max``):

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --grad-stats --dump-grad g.npy 400 600

``--dump-resid FILE.npy`` writes the residual field B − A w of the solve's w
(float64 (M-1, N-1), the shape of ``--dump``) and prints ‖B − A w‖_E on a line
of its own — the stop test is the step size, so this is where to look for
what the iterate still misses.

``--shift S`` (finite, >= 0) solves the shifted problem −Δu + S·u = f,
(A + S·I) w = B — an implicit heat step with S = 1/dt, say.  The analytic
solution does not apply: the error line reads ``n/a`` unless ``--exact`` is
given, and ``--json`` carries ``"shift"``.  The device backends run the classic
two-kernel iteration (``--algo auto`` or ``classic``):

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --shift 40 --rhs f.npy --w0 u.npy --dump u1.npy 400 600

``--stop residual`` stops on the preconditioned residual instead of the step
size: sqrt(g_k) <= max(tol·sqrt(g_0), ``--atol``), g = h1·h2·(z, r) — the rule
for warm starts (``--w0``) and time stepping, where a step-size test stops
early.  ``--json`` then carries ``"stop"``, ``"atol"``, ``"res_nat0"``,
``"res_nat"`` and ``"stop_thr"``; the device backends run one iteration per
launch (``--algo auto``, ``classic`` or ``fused``):

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --stop residual --shift 40 --rhs f.npy --w0 u.npy --atol 1e-7 400 600

``--reaction FILE.npy`` solves −Δu + c(x, y)·u = f, (A + diag(c)) w = B, with the
per-node coefficient c >= 0 of the file, float64 (M-1, N-1) like ``--rhs`` — one
Newton step of a semilinear problem, an absorption that differs between
regions.  Not together with ``--shift`` (add the constant to the field); the
error line reads ``n/a`` unless ``--exact`` is given, ``--json`` carries
``"reaction": true``, and the device backends run ``--algo auto`` / ``classic``:

    python -m poisson_ellipse_openmp_mpi_cuda_amd.cli --reaction c.npy --rhs f.npy --dump u.npy 400 600

Checkpoints hold the iteration state, not the fields: ``--resume`` needs the
same ``--rhs`` (and ``--exact``), the same ``--shift`` and the same ``--reaction``
again, and ignores ``--w0``.
"""

from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

from .models.ellipse import PRESETS, EllipseProblem
from .solver import BACKENDS, reaction_problem, residual, solve, user_field
from .utils import dump as _dump
from .utils.report import json_report, legacy_lines


def build_parser():
    ap = argparse.ArgumentParser(prog="pe", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("M", nargs="?", type=int, default=None)
    ap.add_argument("N", nargs="?", type=int, default=None)
    ap.add_argument("--preset", choices=sorted(PRESETS), default=None)
    ap.add_argument("--backend", choices=BACKENDS, default=os.environ.get("PE_BACKEND", "hip"))
    ap.add_argument("--ranks", type=int, default=1, help="thread-ranks (ranks) or virtual ranks (hip-group)")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "1") or 1))
    ap.add_argument("--decomp", default=None,
                    help="aspect | reference | rows | cols | device | <Px>x<Py> (e.g. 4x2); "
                         "default: device for the GPU backends, aspect otherwise")
    ap.add_argument("--init", choices=("zero", "random"), default="zero")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rhs", default=None, metavar="FILE.npy",
                    help="user right-hand side: float64 (M-1, N-1) array of the interior (masked by the ellipse; "
                         "the L2 / max error is then reported only with --exact); a resumed solve "
                         "(--resume) needs the same --rhs again: checkpoints do not hold it")
    ap.add_argument("--w0", default=None, metavar="FILE.npy",
                    help="user initial guess: float64 (M-1, N-1) array, e.g. the --dump of an earlier run; "
                         "overrides --init; ignored with --resume")
    ap.add_argument("--exact", default=None, metavar="FILE.npy",
                    help="user exact solution: float64 (M-1, N-1) array the L2 / max error in D is measured against "
                         "(in place of the analytic solution; values outside the ellipse are ignored); never enters "
                         "the solve")
    ap.add_argument("--shift", type=float, default=0.0, metavar="S",
                    help="constant shift S >= 0 of the operator: solve -Laplace(u) + S u = f, (A + S I) w = B (default 0: "
                         "the unshifted solve); the L2 / max error is then reported only with --exact; device backends "
                         "run --algo auto / classic; a resumed solve (--resume) needs the same --shift again")
    ap.add_argument("--reaction", default=None, metavar="FILE.npy",
                    help="per-node reaction coefficient c >= 0: float64 (M-1, N-1) array; solve -Laplace(u) + c u = f, "
                         "(A + diag(c)) w = B; not together with --shift; the L2 / max error is then reported only with "
                         "--exact; device backends run --algo auto / classic; a resumed solve needs it again")
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--stop", choices=("step", "residual"), default="step",
                    help="stop rule: step (default) — the step size ||w_{k+1} - w_k|| < tol; residual — the "
                         "preconditioned residual sqrt(g_k) <= max(tol sqrt(g_0), atol), tested before iteration k + 1")
    ap.add_argument("--atol", type=float, default=0.0, metavar="A",
                    help="absolute floor of the residual rule's threshold (finite, >= 0; only with --stop residual)")
    ap.add_argument("--max-iter", type=int, default=-1)
    ap.add_argument("--norm", choices=("weighted", "unweighted"), default="weighted")
    ap.add_argument("--variant", type=int, default=0, help="device arithmetic: 0 fast (default), 1 reference-exact")
    ap.add_argument("--algo", choices=("auto", "classic", "fused", "two-step", "three-step"), default="auto",
                    help="device iteration: fused single-sweep (1 kernel, 1 reduction), two-step / three-step (2 / 3 "
                         "iterations per sweep, 1 reduction per sweep) or classic (2 + 2)")
    ap.add_argument("--timing", action="store_true", help="per-phase device event timers")
    ap.add_argument("--checkpoint", default=None, help="hip: checkpoint file prefix (one file per rank: PREFIX.r<rank>)")
    ap.add_argument("--checkpoint-every", type=int, default=0, help="hip: iterations between checkpoints")
    ap.add_argument("--resume", default=None, help="hip: resume from checkpoint prefix")
    ap.add_argument("--log-every", type=int, default=0, help="print ||dw|| every K iterations (hip: chunk-granular)")
    ap.add_argument("--no-graph", action="store_true", help="(default) eager launches")
    ap.add_argument("--graph", action="store_true", help="replay chunks of iterations from hipGraphs")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--quiet", action="store_true", help="suppress the legacy lines")
    ap.add_argument("--dump", default=None, help="write w (interior) to this .npy")
    ap.add_argument("--pgm", default=None, help="write a grey-scale image of w")
    ap.add_argument("--dump-grad", default=None, metavar="FILE.npy",
                    help="write the gradient of w inside the ellipse, float64 (2, M-1, N-1): [0] d/dx, [1] d/dy")
    ap.add_argument("--grad-stats", action="store_true",
                    help="print h1 h2 sum_D w, h1 h2 sum_D |grad w|^2 and max_D |grad w| after the result lines")
    ap.add_argument("--dump-resid", default=None, metavar="FILE.npy",
                    help="write the residual field B - A w of the solve's w, float64 (M-1, N-1) like --dump, and "
                         "print its E-norm on a line of its own")
    return ap


def main(argv=None) -> int:
    a = build_parser().parse_args(argv)
    prob = PRESETS[a.preset] if a.preset else EllipseProblem()
    if a.M is not None and a.N is not None:
        prob = prob.with_grid(a.M, a.N)
    prob.tol = a.tol
    prob.max_iter = a.max_iter
    prob.norm = a.norm
    prob.shift = a.shift
    prob.stop = a.stop
    prob.atol = a.atol
    want_w = bool(a.dump or a.pgm or a.dump_resid)
    try:
        prob.check_shift()
        prob.check_stop()
        rhs = None if a.rhs is None else user_field("--rhs", np.load(a.rhs, allow_pickle=False), prob)
        w0 = None if a.w0 is None else user_field("--w0", np.load(a.w0, allow_pickle=False), prob)
        exact = None if a.exact is None else user_field("--exact", np.load(a.exact, allow_pickle=False), prob)
        reaction = None
        if a.reaction is not None:
            reaction = reaction_problem(prob, user_field("--reaction", np.load(a.reaction, allow_pickle=False), prob),
                                        False, a.algo)[1]
    except (OSError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    rep = solve(prob, backend=a.backend, ranks=a.ranks, threads=a.threads, decomp=a.decomp, init=a.init,
                seed=a.seed, return_w=want_w, variant=a.variant, timing=a.timing, graph=a.graph and not a.no_graph,
                algo=a.algo, checkpoint=a.checkpoint, checkpoint_every=a.checkpoint_every, resume=a.resume,
                log_every=a.log_every, rhs=rhs, w0=w0, exact=exact, reaction=reaction,
                return_grad=True if a.dump_grad else "stats" if a.grad_stats else False)
    if rep.rank != 0:
        return 0
    if not a.quiet:
        print(legacy_lines(rep, a.tol))
        if (rhs is None and prob.shift == 0.0 and reaction is None) or exact is not None:
            err = f"L2 error in D ~ {rep.l2_err:.6e} | max error in D ~ {rep.max_err:.6e}"
        elif rhs is not None:
            err = "L2 error in D ~ n/a (user right-hand side)"
        elif reaction is not None:
            err = "L2 error in D ~ n/a (reaction field)"
        else:
            err = "L2 error in D ~ n/a (shifted operator)"
        print(f"   Process grid {rep.Px}x{rep.Py} | iters/s ~ {rep.iters_per_s:.1f} | {err}")
    if a.grad_stats:
        print(f"   Integral of w in D ~ {rep.integral:.6e} | energy ~ {rep.energy:.6e} | max |grad w| in D ~ "
              f"{rep.grad_max:.6e}")
    if a.dump_resid and rep.w is not None:
        # the backend's own operator pass where this process is the whole job; the host definition otherwise (the
        # gathered w lives on rank 0 only)
        from .parallel.dist import env_rank_world

        alone = a.backend not in ("hip", "dist-cpu") or env_rank_world()[1] == 1
        res = residual(prob, rep.w, rhs, backend=a.backend if alone else "omp", ranks=a.ranks, threads=a.threads,
                       decomp=a.decomp, reaction=reaction)
        np.save(a.dump_resid, res.field)
        print(f"   Residual ||B - A w||_E ~ {math.sqrt(res.sum):.6e}")
    if a.json:
        print(json_report(rep))
    if a.dump_grad and rep.grad is not None:
        np.save(a.dump_grad, rep.grad)
    if want_w and rep.w is not None:
        if a.dump:
            _dump.save(a.dump, rep.w, prob, rep)
        if a.pgm:
            _dump.write_pgm(a.pgm, rep.w)
    sys.stdout.flush()
    if rep.nonfinite:
        print("error: a reduced scalar became NaN/Inf; solve stopped", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())
