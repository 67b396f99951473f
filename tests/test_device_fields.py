"""CPU-side tests of the device-tensor interface of solve(): what must hold
without a GPU — the refusals of return_w="device" off the device backends,
the helper that turns a tensor into (address, strides, float32 flag), and that
the host-side results keep their types."""

import field_checks as fc
import numpy as np
import pytest
import torch

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, SolveReport, solve
from poisson_ellipse_openmp_mpi_cuda_amd.solver import is_device_tensor, tensor_spec

M, N = 10, 14


@pytest.mark.parametrize("backend", ["serial", "omp", "torch"])
def test_device_result_needs_a_device_backend(pe, backend):
    with pytest.raises(ValueError, match="device"):
        solve(EllipseProblem(M, N), backend=backend, return_w="device")


def test_return_w_rejects_other_strings(pe):
    with pytest.raises(ValueError, match="return_w"):
        solve(EllipseProblem(M, N), backend="serial", return_w="gpu")


def test_return_w_true_is_still_numpy(pe):
    rep = solve(EllipseProblem(M, N), backend="serial", return_w=True, rhs=fc.rhs(M, N))
    assert isinstance(rep.w, np.ndarray) and rep.w.shape == (M - 1, N - 1) and rep.w.dtype == np.float64
    assert rep.w_origin is None
    assert solve(EllipseProblem(M, N), backend="serial", return_w=False).w is None


def test_tensor_spec_strides():
    prob = EllipseProblem(M, N)
    c = torch.zeros(M - 1, N - 1, dtype=torch.float64)
    assert tensor_spec("rhs", c, prob) == (c.data_ptr(), N - 1, 1, False)
    t = torch.zeros(N - 1, M - 1, dtype=torch.float64).t()  # a transposed view
    assert tensor_spec("rhs", t, prob) == (t.data_ptr(), 1, M - 1, False)
    e = torch.tensor(1.0, dtype=torch.float64).expand(M - 1, N - 1)
    assert tensor_spec("rhs", e, prob) == (e.data_ptr(), 0, 0, False)
    big = torch.zeros(M + 6, 2 * N + 9, dtype=torch.float32)
    v = big[3:3 + M - 1, 5:5 + 2 * (N - 1):2]  # a strided window: the address is the window's first element
    assert tensor_spec("w0", v, prob) == (big.data_ptr() + 4 * (3 * (2 * N + 9) + 5), 2 * N + 9, 2, True)
    assert not is_device_tensor(c) and not is_device_tensor(np.zeros(3)) and not is_device_tensor(None)


@pytest.mark.parametrize("bad", [
    torch.zeros(M - 1, N, dtype=torch.float64),
    torch.zeros(M - 1, dtype=torch.float64),
    torch.zeros(N - 1, M - 1, dtype=torch.float64),
    torch.zeros(M - 1, N - 1, dtype=torch.int64),
    torch.zeros(M - 1, N - 1, dtype=torch.float16),
    torch.zeros(M - 1, N - 1, dtype=torch.complex128)])
def test_tensor_spec_refusals(bad):
    with pytest.raises(ValueError, match="w0"):
        tensor_spec("w0", bad, EllipseProblem(M, N))


def test_to_dict_drops_a_tensor_w():
    rep = SolveReport("hip", M, N, 1, 1, 1, 1, 5, True, False, 1e-7, {"solver": 1.0}, -1.0, -1.0, 0.0,
                      w=torch.ones(M - 1, N - 1, dtype=torch.float64), w_origin=(1, 1))
    d = rep.to_dict()
    assert "w" not in d and d["iters"] == 5 and d["w_origin"] == (1, 1)
    assert rep.w is not None  # the report itself keeps it


def test_session_is_exported():
    assert callable(DeviceSession) and hasattr(DeviceSession, "solve") and hasattr(DeviceSession, "close")
