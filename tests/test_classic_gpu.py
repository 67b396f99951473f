"""MI355X tests of the classic two-kernel path (csrc/hip/kernels.hip: kInit /
kInitField, kF, kG and their SHIFT instantiations) — the only device path of a
shifted problem, of variant 1 and of 2-D blocks too thin for a sweep — node
for node against the fp64 reference loop after a fixed number of iterations,
far from convergence: r, the p plane kF wrote last, w, the three reduced sums,
α and β on one rank; the gathered w on virtual ranks and across processes.
Cases, references, bounds and comparisons: classic_checks.py (gated on the CPU
by test_classic_oracle.py).

Shapes are the smallest that reach the code they are there for (strip edges at
128 columns, the second segment at 61 rows, the UP-neighbour halo column in
each of the three lanes it can fall into, one-row blocks); every test takes
seconds."""

import classic_checks as cc
import pytest

pytestmark = pytest.mark.gpu


def _free(monkeypatch):
    """No item height or order inherited from the caller's environment."""
    monkeypatch.delenv("PE_TI", raising=False)
    monkeypatch.delenv("PE_ORDER", raising=False)


# ---- 1. one rank -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", cc.VARIANTS)
@pytest.mark.parametrize("sigma", cc.SIGMAS)
@pytest.mark.parametrize("M,N,K", cc.EDGES, ids=[f"{M}x{N}" for M, N, _ in cc.EDGES])
def test_strip_and_item_edges(gpu, nat, M, N, K, sigma, variant, monkeypatch):
    """Both user fields through kInitField; default items of 8 rows."""
    _free(monkeypatch)
    cc.check_single(nat, M, N, K, sigma, variant, ti=8, order=0)


@pytest.mark.parametrize("variant", cc.VARIANTS)
@pytest.mark.parametrize("sigma", cc.SIGMAS)
def test_builtin_rhs_zero_start(gpu, nat, sigma, variant, monkeypatch):
    """No user field: kInit<EXACT, SHIFT> rather than kInitField."""
    _free(monkeypatch)
    M, N, K = cc.BUILTIN
    cc.check_single(nat, M, N, K, sigma, variant, with_fields=False, ti=8, order=0)


@pytest.mark.parametrize("variant", cc.VARIANTS)
@pytest.mark.parametrize("sigma", cc.FORCED_SIGMAS)
@pytest.mark.parametrize("ti,order", cc.FORCED, ids=[f"ti{t or 8}-order{o or 0}" for t, o in cc.FORCED])
def test_forced_item_heights(gpu, nat, ti, order, sigma, variant, monkeypatch):
    """130 rows: one-row items (ib == ie), items of 60 + 1 rows (the segment
    loop's second turn reloads SegData and recomputes hL / hR), one item of
    three segments, and the default height dealt strip-major.  The classic
    path takes the forced height as it is: the solver reports it."""
    _free(monkeypatch)
    if ti:
        monkeypatch.setenv("PE_TI", ti)
    if order:
        monkeypatch.setenv("PE_ORDER", order)
    M, N, K = cc.FORCED_GRID
    cc.check_single(nat, M, N, K, sigma, variant, ti=int(ti or 8), order=int(order or 0))


@pytest.mark.parametrize("M,N,K,sigma,variant,member", cc.family_cases(),
                         ids=[f"{m}-{M}x{N}-s{s:g}-v{v}" for M, N, _, s, v, m in cc.family_cases()])
def test_ellipse_family(gpu, nat, M, N, K, sigma, variant, member, monkeypatch):
    """Band and interior coefficients at the box edge and on strip edges, with
    and without the shift: σ enters the band in cset / cset_mem, the uniform
    classes through the host's D_in / D_out / dinv_in / dinv_out."""
    _free(monkeypatch)
    cc.check_single(nat, M, N, K, sigma, variant, member, ti=8, order=0)


# ---- 2. virtual ranks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,algo", cc.RANK_SIGMAS, ids=[f"s{s:g}-{a}" for s, a in cc.RANK_SIGMAS])
@pytest.mark.parametrize("M,N,ranks,decomp", cc.VIRTUAL, ids=[f"{M}x{N}-{d}" for M, N, _, d in cc.VIRTUAL])
def test_virtual_ranks(gpu, M, N, ranks, decomp, sigma, algo, monkeypatch):
    """The UP-neighbour halo column as c1 of lane 0 of a one-column strip, as
    hR of a full strip, as c1 of lane 63; send_up from c0 and from c1; one-row
    blocks; 2-D seams."""
    _free(monkeypatch)
    cc.check_virtual(M, N, ranks, decomp, sigma, algo)


@pytest.mark.parametrize("M,N,ranks,decomp,member", cc.VIRTUAL_FAMILY,
                         ids=[f"{m}-{M}x{N}-{d}" for M, N, _, d, m in cc.VIRTUAL_FAMILY])
def test_virtual_ranks_family_shifted(gpu, M, N, ranks, decomp, member, monkeypatch):
    """σ = 40 with band and interior coefficients on the block seams."""
    _free(monkeypatch)
    cc.check_virtual(M, N, ranks, decomp, 40.0, "auto", member)


# ---- 3. processes on one GPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,algo", cc.RANK_SIGMAS, ids=[f"s{s:g}-{a}" for s, a in cc.RANK_SIGMAS])
@pytest.mark.parametrize("M,N,ranks,decomp", cc.PROCESSES, ids=[f"{M}x{N}-{d}" for M, N, _, d in cc.PROCESSES])
def test_processes(gpu, M, N, ranks, decomp, sigma, algo, tmp_path):
    cc.check_processes(M, N, ranks, decomp, sigma, algo, 0, tmp_path)


def test_processes_variant1(gpu, tmp_path):
    (M, N, ranks, decomp), sigma = cc.PROCESS_VARIANT1
    cc.check_processes(M, N, ranks, decomp, sigma, "auto", 1, tmp_path)
