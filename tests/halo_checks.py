"""The multi-rank cases of test_halo_edges.py and their one comparison: a
fixed number of iterations across ranks — row slabs and 2-D blocks at the
smallest sizes each sweep and each halo path accept — against the PyTorch
fp64 recurrence (ops/torch_ref.py) of the whole grid, node for node.  A fixed
count well short of convergence, because a converged solve heals a halo that
is subtly wrong: a stale corner or a row from the wrong parity buffer moves the
iteration count by one and still ends within 1e-9.

A case is (M, N, nproc, decomp, algo, K, env, expect_algo): nproc processes on
the one GPU through the host-staged transport with P2P sums, `--algo algo
--max-iter K`, env the forced halo path (PE_HALO, PE_OVERLAP).  The CPU test
of the references (test_oracle.py) walks REFERENCE_CASES and BLOCKS.

Strips are 48 output columns (kS3), 120 (kS2), 124 (kS); the halo is 6 / 4 / 2
deep, the in-sweep push needs slabs of twice that."""

import json
import os
import subprocess
import sys

import numpy as np
import sweep_checks
from norm_checks import check_norms

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREE, TWO, SINGLE = "three-step", "two-step", "fused"
KIND = {THREE: "three", TWO: "two", SINGLE: "single"}  # -> sweep_checks.KINDS
TUNING = ("PE_HALO", "PE_OVERLAP", "PE_STEPS", "PE_TI", "PE_TI_TUNE")  # stripped from the inherited environment


def _case(M, N, nproc, decomp, algo, K, halo, overlap, expect):
    return (M, N, nproc, decomp, algo, K, {"PE_HALO": halo, "PE_OVERLAP": overlap}, expect)


# Two-step row slabs (kS2, depth-4 halo; the sweep has no overlap variant).
TWO_SLABS = (
    # 8 rows per rank (the minimum, and 2 halo depths: the pushed rows are the whole slab), one exactly full strip
    [_case(33, 121, 4, "rows", "auto", 12, h, "0", TWO) for h in ("exchange", "put", "push")]
    # a cap on a sweep's first iteration
    + [_case(33, 121, 4, "rows", "auto", 13, h, "0", TWO) for h in ("exchange", "push")]
    # slabs of 12/11/11/11 rows, a second strip with one output column
    + [_case(46, 122, 4, "rows", "auto", 12, h, "0", TWO) for h in ("exchange", "put")]
    # 32 rows per rank, where auto would take three steps
    + [_case(97, 50, 3, "rows", "two-step", 12, h, "0", TWO) for h in ("exchange", "put", "push")])

PATHS = [("exchange", "0"), ("put", "0"), ("push", "0"), ("exchange", "1"), ("put", "1")]
# Three-step row slabs (kS3, depth-6 halo): 12 rows per rank and one exactly
# full strip; 13/12/12 rows and 49 columns; 32 rows per rank.
THREE_SLABS = (
    [_case(M, N, 3, "rows", "auto", 12, h, o, THREE) for M, N in ((37, 49), (38, 50), (97, 98)) for h, o in PATHS]
    # caps on a sweep's first and second iteration: the replay launch across ranks
    + [_case(38, 50, 3, "rows", "auto", K, h, "0", THREE) for K in (13, 14) for h in ("push", "put", "exchange")])

PATHS_2D = [("exchange", "0"), ("put", "0"), ("exchange", "1"), ("put", "1")]
# Three-step 2-D splits: 12×12 blocks; 13/12 rows × 49 columns (a one-column
# last strip in front of an UP neighbour); 2x3, whose middle blocks have DOWN
# and UP neighbours on such strips.  (No put + overlap on the six processes:
# choose_halo_path documents a stall of that job on a shared GPU.)
THREE_2D = (
    [_case(25, 25, 4, "2x2", "auto", 9, h, o, THREE) for h, o in PATHS_2D]
    + [_case(26, 99, 4, "2x2", "auto", K, h, o, THREE) for K in (12, 13) for h, o in PATHS_2D]
    + [_case(27, 148, 6, "2x3", "auto", 12, h, o, THREE) for h, o in PATHS_2D if (h, o) != ("put", "1")])

# The single sweep under the 12×12 threshold: 11×11 blocks.
SINGLE_2D = [_case(23, 23, 4, "2x2", "auto", 9, "exchange", o, SINGLE) for o in ("0", "1")]

# In-process virtual ranks (the group driver's own pack, exchange and sums): (M, N, ranks, decomp, K, expect_algo)
VIRTUAL = [(25, 25, 4, "2x2", 9, THREE), (26, 99, 4, "2x2", 12, THREE), (26, 99, 4, "2x2", 13, THREE),
           (27, 148, 6, "2x3", 12, THREE), (23, 23, 4, "2x2", 9, SINGLE)]

# Virtual ranks on family members (test_sweep_family.py): block seams and the one-column last strip in front of an
# UP neighbour, through nodes with interior coefficients at the box edge
FAMILY_VIRTUAL = [v + (m,) for m in sweep_checks.SHORT_MEMBERS for v in (VIRTUAL[0], VIRTUAL[1], VIRTUAL[4])]

CASES = TWO_SLABS + THREE_SLABS + THREE_2D + SINGLE_2D

# every (kind, M, N, K) whose reference a case above is compared with
REFERENCE_CASES = sorted({(KIND[c[7]], c[0], c[1], c[5]) for c in CASES} | {(KIND[v[5]], v[0], v[1], v[4]) for v in VIRTUAL})

FAMILY_REFERENCE_CASES = sorted({(KIND[v[5]], v[0], v[1], v[4], v[6]) for v in FAMILY_VIRTUAL})

# (M, N, ranks, decomp) -> rows per block along x, columns per block along y: what each shape is there for
BLOCKS = {
    (33, 121, 4, "rows"): ([8, 8, 8, 8], [120]),
    (46, 122, 4, "rows"): ([12, 11, 11, 11], [121]),
    (97, 50, 3, "rows"): ([32, 32, 32], [49]),
    (37, 49, 3, "rows"): ([12, 12, 12], [48]),
    (38, 50, 3, "rows"): ([13, 12, 12], [49]),
    (97, 98, 3, "rows"): ([32, 32, 32], [97]),
    (25, 25, 4, "2x2"): ([12, 12], [12, 12]),
    (26, 99, 4, "2x2"): ([13, 12], [49, 49]),
    (27, 148, 6, "2x3"): ([13, 13], [49, 49, 49]),
    (23, 23, 4, "2x2"): ([11, 11], [11, 11]),
}


def case_id(c):
    M, N, nproc, decomp, algo, K, env, _ = c
    return f"{M}x{N}-{nproc}-{decomp}-{algo}-K{K}-{env['PE_HALO']}-ov{env['PE_OVERLAP']}"


def _w_deviation(tag, M, N, K, kind, w, member=None):
    """max |w − w_ref| against the bound f_tol · max |w_ref|; returns (relative
    deviation, bound, reference).  member: a sweep_checks.FAMILY name (None:
    the reference problem)."""
    f_tol = sweep_checks.KINDS[kind][6]
    ref = sweep_checks.reference("single", M, N, K, member)
    want = ref.w[1:M, 1:N].numpy()
    assert w.shape == want.shape, (tag, w.shape)
    return float(np.abs(w - want).max() / np.abs(want).max()), f_tol, ref


def check_case(case, tmp_path):
    """Runs the case's job, checks what it reports it ran, prints the worst
    deviations ("halo-dev"), then asserts them; returns them."""
    from conftest import free_port

    M, N, nproc, decomp, algo, K, env, expect = case
    tag = case_id(case)
    outp = str(tmp_path / "w.npy")
    base = {k: v for k, v in os.environ.items() if k not in TUNING}
    full = dict(base, PE_COMM="host", PE_ALLREDUCE="p2p", PE_P2P_TIMEOUT_S="60", PE_XR="1", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m", "poisson_ellipse_openmp_mpi_cuda_amd",
           "--json", "--quiet", "--decomp", decomp, "--algo", algo, "--max-iter", str(K), "--dump", outp, str(M), str(N)]
    out = subprocess.run(cmd, cwd=ROOT, env=full, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    # what ran: the decomposition, the sweep, the halo path — no silent fallback
    rows, cols = BLOCKS[(M, N, nproc, decomp)]
    assert d["ranks"] == nproc and d["Px"] == len(rows) and d["Py"] == len(cols), d
    assert d["algo"] == expect, d["algo"]
    assert d["iters"] == K and not d["converged"], (d["iters"], d["converged"])
    halo, overlap = env["PE_HALO"], env["PE_OVERLAP"] == "1"
    path = d["halo_path"]
    assert path.startswith(halo) and ("+overlap" in path) == overlap, path
    assert d["overlap"] == overlap, path
    assert d["halo_push"] == (halo == "push") and d["halo_put"] == (halo == "put"), d
    assert d["xr"] and d["comm"] == "p2p-allreduce+host-staged", d["comm"]
    assert d["push_status"] == ("available" if halo == "push" else "off: 2-D blocks" if len(cols) > 1
                                else f"off: PE_HALO={halo}"), d["push_status"]
    assert d["put_status"] == ("available" if halo == "put" else f"off: PE_HALO={halo}"), d["put_status"]

    kind = KIND[expect]
    prob = EllipseProblem(M, N)
    w = np.load(outp)
    dev_w, f_tol, ref = _w_deviation(tag, M, N, K, kind, w)
    dev = {"w": dev_w / f_tol}
    three = expect == THREE
    if three:  # the recurrence's ‖r_K‖_E (after a replay, when K is inside a sweep)
        r = ref.r[1:M, 1:N].numpy()
        hh = prob.h1 * prob.h2
        rec_ref = float(np.sqrt((r * r).sum() * hh))
        rec_bound = f_tol * float(np.abs(r).max()) * float(np.sqrt((M - 1) * (N - 1) * hh))
        dev["res_rec"] = abs(d["res_rec"] - rec_ref) / rec_bound
    # (w and res_rec in units of their bounds: 1 is the bound)
    print(f"halo-dev {tag} algo={d['algo']} path={path!r} w/bound={dev['w']:.2e} w_rel={dev_w:.2e}"
          + (f" res_rec/bound={dev['res_rec']:.2e} res_gap={d['res_gap']:.2e}" if three else ""))
    dev.update(check_norms(tag, prob, d, w, three))
    assert dev["w"] <= 1.0, (tag, dev_w, f_tol)
    if three:
        assert dev["res_rec"] <= 1.0, (tag, d["res_rec"], rec_ref, rec_bound)
    else:  # no moment recurrence to check: not reported
        assert d["res_rec"] == -1.0 and d["res_gap"] == -1.0
    return dev


def check_virtual(M, N, ranks, decomp, K, expect, member=None):
    """K iterations on virtual ranks of one process (backend hip-group): w
    against the same reference and bound."""
    rows, cols = BLOCKS[(M, N, ranks, decomp)]
    prob = sweep_checks.problem(M, N, member)
    prob.max_iter = K
    rep = solve(prob, backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False, return_w=True)
    assert rep.Px == len(rows) and rep.Py == len(cols) and rep.algo == expect, (rep.Px, rep.Py, rep.algo)
    assert rep.iters == K and not rep.converged, (rep.iters, rep.converged)
    tag = f"{M}x{N}{'-' + member if member else ''}-{ranks}-{decomp}-K{K}-virtual"
    dev_w, f_tol, _ = _w_deviation(tag, M, N, K, KIND[expect], rep.w, member)
    print(f"halo-dev {tag} algo={rep.algo} path='virtual ranks' w/bound={dev_w / f_tol:.2e} w_rel={dev_w:.2e}")
    assert dev_w <= f_tol, (tag, dev_w, f_tol)
    return dev_w / f_tol
