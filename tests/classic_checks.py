"""The cases of test_classic_gpu.py and their comparisons: a fixed number of
iterations of the classic two-kernel path (csrc/hip/kernels.hip kF + kG,
started by kInit / kInitField) — the only device path of a shifted problem, of
variant 1 and of thin 2-D blocks — against the fp64 reference loop
(torch_ref.classic), node for node and far from convergence: a converged solve
heals a strip edge or a halo column that is subtly wrong and still ends within
1e-9 (halo_checks.py).  The CPU test of the references (test_classic_oracle.py)
walks REFERENCES and BLOCKS: a case whose references disagree is not compared
on a device.

Grids are M×N, the interior nx×ny = (M−1)×(N−1).  The classic walk: strips of
128 columns, 2 per lane (lane l owns columns c0 = j0 + 2l and c1 = c0 + 1);
items of 8 rows (PE_TI forces another height); inside an item, segments of 60
rows whose row classes and strip-edge columns hL / hR live one row per lane.

User fields are field_checks.rhs / w0 (asymmetric in x and y), the shifts
SIGMAS, the ellipses sweep_checks.FAMILY.  Bounds (none taken from the code
under test): one rank sweep_checks.KINDS["single"] — r, p, w within 1e-12 of
the plane's maximum, sums rel 1e-10 / abs 1e-13·scale, α and β rel 1e-12;
several ranks w within 1e-12·max|w_ref|."""

import functools
import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (0.0, 0.75, 40.0)
VARIANTS = (0, 1)
K = 12
_, _, _, S_REL, S_ABS, AB_REL, F_TOL = sweep_checks.KINDS["single"]

# One rank, both user fields (kInitField): (M, N, K)
EDGES = [
    (9, 129, K),    # 128 columns: exactly one full strip, one 8-row item
    (10, 130, K),   # 129 columns: a second strip of one column (the single-element stores); 9 rows: a one-row item
    (9, 128, K),    # 127 columns: the last lane owns c0 only
    (9, 258, K),    # 257 columns: two full strips + 1, hL and hR both from owned columns
    (130, 9, K),    # 17 items down one strip of 8 columns
    (9, 9, 4),      # the smallest grid (converges in 10-20 iterations)
]
BUILTIN = (10, 130, K)  # the same without user fields: kInit rather than kInitField

# Forced item heights on 130 rows × 129 columns: (PE_TI, PE_ORDER) -> one-row items (ib == ie); a 60 + 1 row segment
# pair in each item; three segments in one item; the default height dealt strip-major
FORCED_GRID = (131, 130, K)
FORCED = [("1", None), ("61", None), ("130", None), (None, "1")]
FORCED_SIGMAS = (0.0, 40.0)

# The ellipse family (band and interior coefficients at the box edge): shapes per member, σ ∈ FAMILY_SIGMAS on
# variant 0, variant 1 at the first shape.  cut_xy only from M > 10 (at M ≤ 10 the same nodes as cover).
FAMILY_SHAPES = [(10, 130, K), (9, 258, K), (66, 130, K)]
FAMILY_SIGMAS = (0.0, 40.0)


def family_cases():
    """(M, N, K, σ, variant, member) of the family on one rank."""
    out = []
    for member in sweep_checks.FAMILY:
        for n, (M, N, k) in enumerate(FAMILY_SHAPES):
            if member == "cut_xy" and M <= 10:
                continue
            for sigma in FAMILY_SIGMAS:
                out += [(M, N, k, sigma, v, member) for v in ((0, 1) if n == 0 else (0,))]
    return out


# Several ranks: (M, N, ranks, decomp); σ = 0 runs --algo classic, σ = 40 auto.
VIRTUAL = [
    (9, 258, 2, "1x2"),    # 129 / 128 columns: halo column = c1 of lane 0 of a one-column strip; send_up from c0 == ny
    (9, 257, 2, "1x2"),    # 128 / 128: halo column = hR of a full strip (jr == ny + 1); send_up from c1 == ny
    (9, 383, 3, "1x3"),    # 128 / 127 / 127: the middle block has DOWN and UP neighbours; halo column = c1 of lane 63
    (5, 130, 4, "rows"),   # 1 row each: every row's neighbours are halo rows
    (26, 27, 4, "2x2"),    # 13/12 × 13/13: small 2-D seams
    (27, 259, 4, "2x2"),   # 13/13 × 129/129: 2-D seams with a one-column last strip in front of an UP neighbour
]
VIRTUAL_FAMILY = [v + (m,) for m in sweep_checks.SHORT_MEMBERS for v in (VIRTUAL[0], VIRTUAL[5])]  # at σ = 40
PROCESSES = [(37, 130, 3, "rows"), VIRTUAL[0], VIRTUAL[2], VIRTUAL[5], VIRTUAL[3]]
PROCESS_VARIANT1 = (VIRTUAL[5], 40.0)  # one shape once more with --variant 1
RANK_SIGMAS = ((0.0, "classic"), (40.0, "auto"))

# (M, N, ranks, decomp) -> rows per block along x, columns per block along y: what each shape is there for
BLOCKS = {
    (9, 258, 2, "1x2"): ([8], [129, 128]),
    (9, 257, 2, "1x2"): ([8], [128, 128]),
    (9, 383, 3, "1x3"): ([8], [128, 127, 127]),
    (5, 130, 4, "rows"): ([1, 1, 1, 1], [129]),
    (26, 27, 4, "2x2"): ([13, 12], [13, 13]),
    (27, 259, 4, "2x2"): ([13, 13], [129, 129]),
    (37, 130, 3, "rows"): ([12, 12, 12], [129]),
}


def _references():
    """Every (M, N, K, σ, member, fields) whose reference a device test compares with."""
    out = {(M, N, k, s, None, True) for M, N, k in EDGES for s in SIGMAS}
    out |= {BUILTIN + (s, None, False) for s in SIGMAS}
    out |= {FORCED_GRID + (s, None, True) for s in FORCED_SIGMAS}
    out |= {(M, N, k, s, m, True) for M, N, k, s, _, m in family_cases()}
    out |= {(M, N, K, s, None, True) for M, N, _, _ in VIRTUAL + PROCESSES for s, _ in RANK_SIGMAS}
    out |= {(M, N, K, 40.0, m, True) for M, N, _, _, m in VIRTUAL_FAMILY}
    return sorted(out, key=lambda c: (c[4] or "",) + c[:4] + (c[5],))


REFERENCES = _references()


def problem(M, N, sigma=0.0, member=None):
    return EllipseProblem(M, N, shift=sigma, **(sweep_checks.FAMILY[member] if member else {}))


def fields(M, N, on=True):
    """dict(rhs=, w0=) of the case (field_checks' arrays, read-only), or none."""
    return dict(rhs=fc.rhs(M, N), w0=fc.w0(M, N)) if on else {}


@functools.lru_cache(maxsize=None)
def reference(M, N, k, sigma=0.0, member=None, with_fields=True):
    """torch_ref.classic after k iterations; computed once, never modified."""
    return torch_ref.classic(problem(M, N, sigma, member), k, **fields(M, N, with_fields))


def case_tag(M, N, k, sigma, variant, member=None, with_fields=True):
    return (f"{M}x{N}{' ' + member if member else ''} K={k} shift={sigma:g} v{variant}"
            + ("" if with_fields else " builtin"))


def check_single(nat, M, N, k, sigma, variant, member=None, with_fields=True, ti=None, order=None):
    """k iterations of kF + kG on one rank against the reference loop: r, p_k
    (the plane kF wrote last), w, the three sums, α, β, the iteration count.
    ti / order: what the solver must report it runs (forced by the caller's
    environment).  Prints the deviations ("classic-dev"), and for variant 1
    whether each plane has the reference's bits, then asserts; returns them."""
    prob = problem(M, N, sigma, member)
    s = fc.solver(nat, M, N, 1, variant, fields=with_fields, prob=prob)
    assert not s.fused and s.user_rhs == with_fields and s.user_w0 == with_fields
    if ti is not None:
        assert s.ti == ti, (s.ti, ti)
    if order is not None:
        assert s.order == order, (s.order, order)
    s.reset()
    s.run_iterations(k, False)
    s.synchronize()
    st = s.state()
    ref = reference(M, N, k, sigma, member, with_fields)
    par = (k - 1) & 1  # iteration k writes p[(k − 1) & 1]
    got = {"r": s.field(0)[1:M, 1:N], "p": s.field(2 + par)[1:M, 1:N], "w": s.w()}
    want = {name: getattr(ref, name)[1:M, 1:N].numpy() for name in got}
    dev = {name: float(np.abs(got[name] - want[name]).max() / np.abs(want[name]).max()) for name in got}
    sums_got = list(st["red_F"]) + [st["red_G"]]
    sums_want = ref.sums[-1]
    scale = max(abs(x) for x in sums_want)
    # (the sums' worst deviation in units in which the bound below is S_REL)
    dev["sums"] = max(abs(g - x) / max(abs(x), S_ABS / S_REL * scale) for g, x in zip(sums_got, sums_want))
    dev["alpha"] = abs(st["alpha"] - ref.alpha[-1]) / abs(ref.alpha[-1])
    dev["beta"] = abs(st["beta"] - ref.beta[-1]) / abs(ref.beta[-1])
    bits = "".join(f" {n}_bits={int(np.array_equal(got[n], want[n]))}" for n in got) if variant == 1 else ""
    print(f"classic-dev {case_tag(M, N, k, sigma, variant, member, with_fields)} ti={s.ti} order={s.order} "
          + " ".join(f"{n}={v:.2e}" for n, v in dev.items()) + bits)
    assert st["iter"] == k and st["status"] == 0, (st["iter"], st["status"])
    for n, (g, x) in enumerate(zip(sums_got, sums_want)):
        assert g == pytest.approx(x, rel=S_REL, abs=S_ABS * scale), n
    assert st["alpha"] == pytest.approx(ref.alpha[-1], rel=AB_REL)
    assert st["beta"] == pytest.approx(ref.beta[-1], rel=AB_REL)
    for name in got:
        np.testing.assert_allclose(got[name], want[name], rtol=0, atol=F_TOL * np.abs(want[name]).max(), err_msg=name)
    return dev


def _check_w(tag, w, M, N, sigma, member=None):
    want = reference(M, N, K, sigma, member).w[1:M, 1:N].numpy()
    assert w.shape == want.shape, (tag, w.shape)
    dev = float(np.abs(w - want).max() / np.abs(want).max())
    print(f"classic-dev {tag} w={dev:.2e}")
    assert dev <= F_TOL, (tag, dev)
    return dev


def check_virtual(M, N, ranks, decomp, sigma, algo, member=None):
    """K iterations on virtual ranks of one process (backend hip-group) with
    both fields: what ran, and the gathered w against the whole-grid loop."""
    rows, cols = BLOCKS[(M, N, ranks, decomp)]
    prob = problem(M, N, sigma, member)
    prob.max_iter = K
    rep = solve(prob, backend="hip-group", ranks=ranks, decomp=decomp, algo=algo, check_tol=False, return_w=True,
                **fields(M, N))
    assert rep.algo == "classic" and rep.Px == len(rows) and rep.Py == len(cols), (rep.algo, rep.Px, rep.Py)
    assert rep.iters == K and not rep.converged, (rep.iters, rep.converged)
    tag = f"{M}x{N}{' ' + member if member else ''} K={K} shift={sigma:g} {ranks}-{decomp}-virtual algo={algo}"
    return _check_w(tag, rep.w, M, N, sigma, member)


def check_processes(M, N, ranks, decomp, sigma, algo, variant, tmp_path):
    """The same through `ranks` processes on the one GPU (host-staged
    transport, one job under its own time limit): what the job reports it ran,
    and the w it gathered against the whole-grid loop."""
    from conftest import free_port

    rows, cols = BLOCKS[(M, N, ranks, decomp)]
    assert ranks <= 4
    f, g, outp = (str(tmp_path / n) for n in ("f.npy", "g.npy", "w.npy"))
    np.save(f, fc.rhs(M, N))
    np.save(g, fc.w0(M, N))
    env = dict({k: v for k, v in os.environ.items() if k not in ("PE_TI", "PE_ORDER")}, PE_COMM="host",
               PE_HALO="exchange", PE_OVERLAP="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m",
           "poisson_ellipse_openmp_mpi_cuda_amd", "--json", "--quiet", "--decomp", decomp, "--algo", algo, "--shift",
           repr(sigma), "--variant", str(variant), "--rhs", f, "--w0", g, "--max-iter", str(K), "--dump", outp,
           str(M), str(N)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["algo"] == "classic" and d["ranks"] == ranks and d["Px"] == len(rows) and d["Py"] == len(cols), d
    assert d["iters"] == K and not d["converged"], (d["iters"], d["converged"])
    assert d.get("shift", 0.0) == sigma and d["init"] == "field", d
    tag = f"{M}x{N} K={K} shift={sigma:g} v{variant} {ranks}-{decomp}-processes algo={algo}"
    return _check_w(tag, np.load(outp), M, N, sigma)
