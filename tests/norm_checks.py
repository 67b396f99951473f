"""The end-of-solve figures — kResid's ‖B − A w‖_E and ‖B‖_E, kError's L2 /
max error and max |w| outside the ellipse — recomputed in plain fp64 on the
CPU (torch_ref.assemble / apply_A / error_vs_analytic) from the w a solve
returned, and the one comparison of a report with them.  Shared by
test_residual.py and halo_checks.py."""

import functools
import math

import numpy as np
import pytest
import torch

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref


@functools.lru_cache(maxsize=None)
def _assembled(M, N, A1, B1, A2, B2, cx, cy, F):
    return torch_ref.assemble(EllipseProblem(M, N, A1=A1, B1=B1, A2=A2, B2=B2, cx=cx, cy=cy, F=F))


def assembled(prob):
    """a, b, B of the problem's own box and ellipse; computed once per problem."""
    assert prob.shift == 0.0  # (A + σI is shift_checks' subject)
    return _assembled(prob.M, prob.N, prob.A1, prob.B1, prob.A2, prob.B2, prob.cx, prob.cy, prob.F)


def fp64_norms(prob, w):
    """‖B − A w‖_E, ‖B‖_E, the L2 and max error in D and max |w| over the
    interior nodes outside D, in fp64 on the CPU, of the interior array w."""
    M, N = prob.M, prob.N
    a, b, B = assembled(prob)
    W = torch.zeros(M + 1, N + 1, dtype=torch.float64)
    W[1:M, 1:N] = torch.from_numpy(np.ascontiguousarray(w))
    hh = prob.h1 * prob.h2
    rho = (B - torch_ref.apply_A(W, a, b, prob.h1, prob.h2))[1:-1, 1:-1]
    l2, mx = torch_ref.error_vs_analytic(prob, W)
    x = prob.A1 + np.arange(M + 1, dtype=np.float64) * prob.h1
    y = prob.A2 + np.arange(N + 1, dtype=np.float64) * prob.h2
    outside = ~((prob.cx * x[:, None] * x[:, None] + prob.cy * y[None, :] * y[None, :]) < 1.0)
    wo = np.abs(W.numpy())[1:M, 1:N][outside[1:M, 1:N]]
    return dict(res_true=math.sqrt(float((rho * rho).sum()) * hh), b_norm=math.sqrt(float((B * B).sum()) * hh),
                l2_err=l2, max_err=mx, max_outside=float(wo.max()) if wo.size else 0.0)


def resid_tol(prob):
    """kResid applies A with the division-free band coefficients, which differ
    from the assembly's by at most (1/ε)·ulp(1) per face (the bound
    test_fast_coefficients_vs_assembly holds them to; + 4 ulp for 1/D's
    share); the factor 100 covers the summation order."""
    return 100.0 * (1.0 / prob.eps + 4.0) * np.spacing(1.0)


def check_norms(tag, prob, got, w, three):
    """got: res_true, b_norm, l2_err, max_err, max_outside (+ res_rec, res_gap).
    Prints every deviation, then asserts; returns the deviations."""
    ref = fp64_norms(prob, w)
    tol = resid_tol(prob)
    dev = {k: abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] else abs(got[k]) for k in ref}
    print(f"norm-dev {tag} tol={tol:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in dev.items())
          + f" res_true={got['res_true']:.6e} b_norm={got['b_norm']:.6e}")
    assert got["res_true"] == pytest.approx(ref["res_true"], rel=tol)
    assert got["b_norm"] == pytest.approx(ref["b_norm"], rel=tol)
    assert got["l2_err"] == pytest.approx(ref["l2_err"], rel=1e-12)
    assert got["max_err"] == pytest.approx(ref["max_err"], rel=1e-12)
    assert got["max_outside"] == ref["max_outside"] or got["max_outside"] == pytest.approx(ref["max_outside"], rel=1e-12)
    if three:  # the triangle inequality among kResid's own sums: |‖ρ‖ − ‖r‖| ≤ ‖ρ − r‖
        assert abs(got["res_true"] - got["res_rec"]) <= got["res_gap"] * got["res_rec"] * (1 + 1e-9)
    return dev
