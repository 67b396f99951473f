// Python binding of the native core (pybind11).  The package's Python layer
// (poisson_ellipse_openmp_mpi_cuda_amd) adds torch.distributed bootstrap,
// the PyTorch fp64 oracle, the CLI/bench and reporting on top of this.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "../hip/kernels.hpp"
#include "pe/device.hpp"
#include "pe/solver.hpp"

namespace py = pybind11;
using namespace pe;

namespace {

py::dict timers_dict(const Timers& t) {
  py::dict d;
  d["gpu"] = t.gpu;
  d["copy"] = t.copy;
  d["halo"] = t.halo;
  d["reduce"] = t.reduce;
  d["prec"] = t.prec;
  d["dot"] = t.dot;
  d["setup"] = t.setup;
  d["solver"] = t.solver;
  d["iterate"] = t.iterate;
  d["check"] = t.check;
  d["construct"] = t.construct;
  d["sampled"] = t.sampled;
  d["wait"] = t.wait;
  d["dot_fused"] = t.dot_fused;
  return d;
}

// (first row, rows, strip, flags: kBandBit | kUniBit) per list position; rows 0: an empty position
std::vector<std::tuple<int, int, int, int>> entry_tuples(const std::vector<Entry>& list) {
  std::vector<std::tuple<int, int, int, int>> v;
  for (const Entry& e : list) v.emplace_back(e.x & dev::kRowMask3, e.y >> 20, e.y & 0xFFFFF, e.x & ~dev::kRowMask3);
  return v;
}

py::array_t<double> to_array(std::vector<double>&& v, int64_t rows, int64_t cols) {
  auto* heap = new std::vector<double>(std::move(v));
  py::capsule owner(heap, [](void* p) { delete static_cast<std::vector<double>*>(p); });
  return py::array_t<double>({rows, cols}, {cols * int64_t(sizeof(double)), int64_t(sizeof(double))}, heap->data(),
                             owner);
}

// (integral, energy, grad_max) of pe/fields.hpp GradStats
py::tuple grad_tuple(const GradStats& g) { return py::make_tuple(g.integral, g.energy, g.grad_max); }

py::dict state_dict(const dev::DevState& s) {
  py::dict d;
  d["red_F"] = py::make_tuple(s.red_F[0], s.red_F[1]);
  d["red_G"] = s.red_G[0];
  d["stop_thr"] = s.red_G[1];  // residual rule: the threshold (0 otherwise)
  d["err"] = py::make_tuple(s.err[0], s.err[1], s.err[2]);
  d["rz_cur"] = s.rz_cur;
  d["alpha"] = s.alpha;
  d["beta"] = s.beta;
  d["last_diff"] = s.last_diff;
  d["iter"] = s.iter;
  d["done"] = s.done;
  d["status"] = s.status;
  d["started"] = s.started;
  d["gprev"] = s.gprev;
  d["fs"] = py::make_tuple(py::make_tuple(s.fs[0][0], s.fs[0][1], s.fs[0][2], s.fs[0][3], s.fs[0][4], s.fs[0][5],
                                          s.fs[0][6]),
                           py::make_tuple(s.fs[1][0], s.fs[1][1], s.fs[1][2], s.fs[1][3], s.fs[1][4], s.fs[1][5],
                                          s.fs[1][6]));
  py::list f2;
  for (int b = 0; b < 2; ++b) {
    py::list v;
    for (int n = 0; n < dev::kNS2; ++n) v.append(s.fs2[b][n]);
    f2.append(py::tuple(v));
  }
  d["fs2"] = py::tuple(f2);
  d["late3"] = s.late3;
  py::list c3;
  for (int n = 0; n < 12; ++n) c3.append(s.sc3[n]);
  d["sc3"] = py::tuple(c3);
  d["wait_s"] = double(s.xr_wait) * 1e-8;
  d["wpar"] = s.wpar;
  d["res"] = py::make_tuple(s.res[0], s.res[1], s.res[2], s.res[3]);
  d["k0"] = s.k0;
  d["fixj"] = s.fixj;
  return d;
}

// User fields from Python: None or a float64 array of the given shape (any
// layout / dtype numpy converts; the Python layer rejects lossy conversions
// and non-finite values first).  `hold` keeps the converted array alive.
using FieldArr = py::array_t<double, py::array::c_style | py::array::forcecast>;
const double* field_ptr(const py::object& o, int64_t rows, int64_t cols, const char* name, FieldArr& hold) {
  if (o.is_none()) return nullptr;
  hold = FieldArr::ensure(o);
  if (!hold) {
    PyErr_Clear();
    throw std::invalid_argument(std::string(name) + ": not convertible to a float64 array");
  }
  if (hold.ndim() != 2 || hold.shape(0) != rows || hold.shape(1) != cols)
    throw std::invalid_argument(std::string(name) + ": expected shape (" + std::to_string(rows) + ", " +
                                std::to_string(cols) + ")");
  return hold.data();
}

// A device field of Python, (address of element [0][0], stride_i, stride_j, float32 flag) or None, into DeviceFields.
void device_spec(const py::object& o, const void*& ptr, int64_t& si, int64_t& sj, bool& f32) {
  if (o.is_none()) return;
  const auto t = o.cast<std::tuple<uintptr_t, int64_t, int64_t, bool>>();
  ptr = reinterpret_cast<const void*>(std::get<0>(t));
  si = std::get<1>(t);
  sj = std::get<2>(t);
  f32 = std::get<3>(t);
}

// Handle to a DeviceComm owned by Python.
struct CommHandle {
  std::unique_ptr<DeviceComm> comm;
};

}  // namespace

PYBIND11_MODULE(_native, m) {
  m.doc() = "Native core of the MI355X Poisson/fictitious-domain PCG framework (C++ / HIP gfx950 / RCCL)";

  py::enum_<Norm>(m, "Norm").value("Weighted", Norm::Weighted).value("Unweighted", Norm::Unweighted);
  py::enum_<Init>(m, "Init").value("Zero", Init::Zero).value("Random", Init::Random);
  py::enum_<Stop>(m, "Stop").value("Step", Stop::Step).value("Residual", Stop::Residual);
  py::enum_<DecompMode>(m, "DecompMode")
      .value("Reference", DecompMode::Reference)
      .value("Aspect", DecompMode::Aspect)
      .value("Rows", DecompMode::Rows)
      .value("Cols", DecompMode::Cols);

  py::class_<Problem>(m, "Problem")
      .def(py::init<>())
      .def_readwrite("A1", &Problem::A1)
      .def_readwrite("B1", &Problem::B1)
      .def_readwrite("A2", &Problem::A2)
      .def_readwrite("B2", &Problem::B2)
      .def_readwrite("F", &Problem::F)
      .def_readwrite("cx", &Problem::cx)
      .def_readwrite("cy", &Problem::cy)
      .def_readwrite("sx", &Problem::sx)
      .def_readwrite("sy", &Problem::sy)
      .def_readwrite("M", &Problem::M)
      .def_readwrite("N", &Problem::N)
      .def_readwrite("tol", &Problem::tol)
      .def_readwrite("max_iter", &Problem::max_iter)
      .def_readwrite("norm", &Problem::norm)
      .def_readwrite("shift", &Problem::shift)
      .def_readwrite("stop", &Problem::stop)
      .def_readwrite("atol", &Problem::atol)
      .def_readwrite("reaction", &Problem::reaction)
      .def("h1", &Problem::h1)
      .def("h2", &Problem::h2)
      .def("eps", &Problem::eps)
      .def("iter_cap", &Problem::iter_cap)
      .def("u_scale", &Problem::u_scale);

  py::class_<ProcessGrid>(m, "ProcessGrid")
      .def(py::init<>())
      .def_readwrite("Px", &ProcessGrid::Px)
      .def_readwrite("Py", &ProcessGrid::Py);

  py::class_<Block>(m, "Block")
      .def_readonly("rank", &Block::rank)
      .def_readonly("size", &Block::size)
      .def_readonly("Px", &Block::Px)
      .def_readonly("Py", &Block::Py)
      .def_readonly("px", &Block::px)
      .def_readonly("py", &Block::py)
      .def_readonly("i0", &Block::i0)
      .def_readonly("i1", &Block::i1)
      .def_readonly("j0", &Block::j0)
      .def_readonly("j1", &Block::j1)
      .def_readonly("nx", &Block::nx)
      .def_readonly("ny", &Block::ny)
      .def_readonly("pitch", &Block::pitch)
      .def_readonly("rows", &Block::rows)
      .def_readonly("base", &Block::base)
      .def_readonly("alloc", &Block::alloc)
      .def_property_readonly("nbr", [](const Block& b) { return std::vector<int>(b.nbr, b.nbr + 4); })
      .def("__repr__", &describe);

  m.def("choose_process_grid", &choose_process_grid, py::arg("P"), py::arg("M"), py::arg("N"),
        py::arg("mode") = DecompMode::Aspect);
  m.def("choose_process_grid_reference", &choose_process_grid_reference);
  m.def("process_grid_from_spec", &process_grid_from_spec, py::arg("spec"), py::arg("P"), py::arg("M"), py::arg("N"));
  m.def("halo_cost", &halo_cost);
  m.def("decompose", &decompose, py::arg("M"), py::arg("N"), py::arg("pg"), py::arg("rank"), py::arg("align") = 8);

  py::class_<SolveOptions>(m, "SolveOptions")
      .def(py::init<>())
      .def_readwrite("init", &SolveOptions::init)
      .def_readwrite("seed", &SolveOptions::seed)
      .def_readwrite("init_amp", &SolveOptions::init_amp)
      .def_readwrite("threads", &SolveOptions::threads)
      .def_readwrite("log_every", &SolveOptions::log_every)
      .def_readwrite("keep_history", &SolveOptions::keep_history)
      .def_readwrite("compute_error", &SolveOptions::compute_error)
      .def_readwrite("verbose", &SolveOptions::verbose)
      .def_readwrite("chunk", &SolveOptions::chunk)
      .def_readwrite("use_graph", &SolveOptions::use_graph)
      .def_readwrite("timing", &SolveOptions::timing)
      .def_readwrite("check_tol", &SolveOptions::check_tol)
      .def_readwrite("variant", &SolveOptions::variant)
      .def_readwrite("algo", &SolveOptions::algo)
      .def_readwrite("checkpoint_every", &SolveOptions::checkpoint_every)
      .def_readwrite("checkpoint_path", &SolveOptions::checkpoint_path)
      .def_readwrite("resume_path", &SolveOptions::resume_path);

  py::class_<SolveResult>(m, "SolveResult")
      .def_readonly("iters", &SolveResult::iters)
      .def_readonly("converged", &SolveResult::converged)
      .def_readonly("breakdown", &SolveResult::breakdown)
      .def_readonly("nonfinite", &SolveResult::nonfinite)
      .def_readonly("last_diff", &SolveResult::last_diff)
      .def_readonly("zr", &SolveResult::zr)
      .def_readonly("l2_err", &SolveResult::l2_err)
      .def_readonly("max_err", &SolveResult::max_err)
      .def_readonly("max_outside", &SolveResult::max_outside)
      .def_readonly("history", &SolveResult::history)
      .def_readonly("Px", &SolveResult::Px)
      .def_readonly("Py", &SolveResult::Py)
      .def_readonly("backend", &SolveResult::backend)
      .def_readonly("algo", &SolveResult::algo)
      .def_readonly("resident_fallback", &SolveResult::resident_fallback)
      .def_readonly("res_true", &SolveResult::res_true)
      .def_readonly("res_rec", &SolveResult::res_rec)
      .def_readonly("res_gap", &SolveResult::res_gap)
      .def_readonly("b_norm", &SolveResult::b_norm)
      .def_readonly("restarts", &SolveResult::restarts)
      .def_readonly("res_nat0", &SolveResult::res_nat0)
      .def_readonly("res_nat", &SolveResult::res_nat)
      .def_readonly("stop_thr", &SolveResult::stop_thr)
      .def_property_readonly("grad", [](const SolveResult& r) { return grad_tuple(r.grad); },
                             "(integral, energy, grad_max) where the solve computed them (hip-group on request), else -1s")
      .def_property_readonly("timers", [](const SolveResult& r) { return timers_dict(r.t); });

  m.def("format_result_legacy", &format_result_legacy);
  m.def("p2p_setup_status", []() { return p2p_setup_status(); },
        "the last P2P transport set-up of this process: not attempted / ok / fallback: why");

  // ---- CPU backends ------------------------------------------------------
  m.def(
      "cpu_solve",
      [](const Problem& P, int ranks, DecompMode mode, const SolveOptions& opt, bool return_w) {
        std::vector<double> w;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = cpu_pcg_threads(P, ranks, mode, opt, return_w ? &w : nullptr);
        }
        py::object wa = py::none();
        if (return_w) wa = to_array(std::move(w), P.M - 1, P.N - 1);
        return py::make_tuple(r, wa);
      },
      py::arg("prob"), py::arg("ranks") = 1, py::arg("mode") = DecompMode::Reference, py::arg("opt") = SolveOptions(),
      py::arg("return_w") = false);
  m.def(
      "cpu_solve_grid",
      [](const Problem& P, const ProcessGrid& pg, const SolveOptions& opt, bool return_w, py::object rhs,
         py::object w0, py::object exact, py::object reaction) {
        FieldArr hr, hw, he, hc;
        UserFields uf;
        uf.rhs = field_ptr(rhs, P.M - 1, P.N - 1, "rhs", hr);
        uf.w0 = field_ptr(w0, P.M - 1, P.N - 1, "w0", hw);
        uf.exact = field_ptr(exact, P.M - 1, P.N - 1, "exact", he);
        uf.reaction = field_ptr(reaction, P.M - 1, P.N - 1, "reaction", hc);
        std::vector<double> w;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = cpu_pcg_threads(P, pg, opt, return_w ? &w : nullptr, uf);
        }
        py::object wa = py::none();
        if (return_w) wa = to_array(std::move(w), P.M - 1, P.N - 1);
        return py::make_tuple(r, wa);
      },
      py::arg("prob"), py::arg("grid"), py::arg("opt") = SolveOptions(), py::arg("return_w") = false,
      py::arg("rhs") = py::none(), py::arg("w0") = py::none(), py::arg("exact") = py::none(),
      py::arg("reaction") = py::none());

  // One rank of a multi-process CPU run; the transport is Python callbacks
  // (torch.distributed, typically gloo).  exchange_fn receives a list of
  // (dir, peer, send: ndarray, recv: writable ndarray) valid during the call.
  m.def(
      "cpu_solve_rank",
      [](const Problem& P, const Block& blk, py::function reduce_fn, py::function exchange_fn,
         py::function barrier_fn, const SolveOptions& opt, bool return_w, py::object rhs, py::object w0,
         py::object exact, py::object reaction) {
        FieldArr hr, hw, he, hc;
        UserFields uf;  // the GLOBAL arrays: every rank passes the same and takes its slice
        uf.rhs = field_ptr(rhs, P.M - 1, P.N - 1, "rhs", hr);
        uf.w0 = field_ptr(w0, P.M - 1, P.N - 1, "w0", hw);
        uf.exact = field_ptr(exact, P.M - 1, P.N - 1, "exact", he);
        uf.reaction = field_ptr(reaction, P.M - 1, P.N - 1, "reaction", hc);
        auto reduce = [reduce_fn](double* buf, int n, bool is_max) {
          py::gil_scoped_acquire g;
          py::array_t<double> a({n}, {int64_t(sizeof(double))}, buf, py::none());
          reduce_fn(a, is_max);
        };
        auto exch = [exchange_fn](const std::vector<Exchange>& ex) {
          py::gil_scoped_acquire g;
          py::list items;
          for (const auto& e : ex) {
            py::array_t<double> s({e.count}, {int64_t(sizeof(double))}, const_cast<double*>(e.send), py::none());
            py::array_t<double> r({e.count}, {int64_t(sizeof(double))}, e.recv, py::none());
            items.append(py::make_tuple(e.dir, e.peer, s, r));
          }
          exchange_fn(items);
        };
        auto bar = [barrier_fn]() {
          py::gil_scoped_acquire g;
          barrier_fn();
        };
        CallbackHostComm comm(blk.rank, blk.size, reduce, exch, bar);
        std::vector<double> w;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = cpu_pcg(P, blk, comm, opt, return_w ? &w : nullptr, uf);
        }
        py::object wa = py::none();
        if (return_w) wa = to_array(std::move(w), blk.nx, blk.ny);
        return py::make_tuple(r, wa);
      },
      py::arg("prob"), py::arg("block"), py::arg("reduce_fn"), py::arg("exchange_fn"), py::arg("barrier_fn"),
      py::arg("opt") = SolveOptions(), py::arg("return_w") = false, py::arg("rhs") = py::none(),
      py::arg("w0") = py::none(), py::arg("exact") = py::none(), py::arg("reaction") = py::none());

  // One block's slices of global interior arrays (pe/fields.hpp block_field):
  // (rhs owned nx × ny | None, w0 with its ring (nx+2) × (ny+2) | None) — the
  // operands of DeviceSolver.set_rhs / set_w0.
  m.def(
      "block_fields",
      [](int M, int N, const Block& blk, py::object rhs, py::object w0) {
        FieldArr hr, hw;
        const double* r = field_ptr(rhs, int64_t(M) - 1, int64_t(N) - 1, "rhs", hr);
        const double* w = field_ptr(w0, int64_t(M) - 1, int64_t(N) - 1, "w0", hw);
        py::object ro = py::none(), wo = py::none();
        if (r) ro = to_array(block_field(r, M, N, blk, 0), blk.nx, blk.ny);
        if (w) wo = to_array(block_field(w, M, N, blk, 1), blk.nx + 2, blk.ny + 2);
        return py::make_tuple(ro, wo);
      },
      py::arg("M"), py::arg("N"), py::arg("block"), py::arg("rhs") = py::none(), py::arg("w0") = py::none());

  // One field's slice (ring 0: owned nx × ny, ring 1: with its ring) — the
  // operand of DeviceSolver.set_exact (ring 0), and block_fields one field at a time.
  m.def(
      "block_field",
      [](int M, int N, const Block& blk, py::object g, int ring) {
        FieldArr h;
        const double* p = field_ptr(g, int64_t(M) - 1, int64_t(N) - 1, "field", h);
        if (!p) throw std::invalid_argument("block_field: the array is None");
        return to_array(block_field(p, M, N, blk, ring), blk.nx + 2 * ring, blk.ny + 2 * ring);
      },
      py::arg("M"), py::arg("N"), py::arg("block"), py::arg("g"), py::arg("ring") = 0);

  // The gradient of a global interior array and its functionals (pe/fields.hpp
  // gradient_field): ((integral, energy, grad_max), g) with g of shape
  // (2, M-1, N-1), [0] = ∂x, [1] = ∂y — or None with field=False.
  m.def(
      "gradient_field",
      [](const Problem& P, py::object w, bool field) {
        FieldArr h;
        const double* p = field_ptr(w, int64_t(P.M) - 1, int64_t(P.N) - 1, "w", h);
        if (!p) throw std::invalid_argument("gradient_field: the array is None");
        const size_t n = size_t((int64_t(P.M) - 1) * (int64_t(P.N) - 1));
        std::vector<double> g(field ? 2 * n : 0);
        const GradStats s = gradient_field(P, p, field ? g.data() : nullptr, field ? g.data() + n : nullptr);
        py::object ga = py::none();
        if (field) ga = to_array(std::move(g), 2 * (int64_t(P.M) - 1), P.N - 1).attr("reshape")(2, P.M - 1, P.N - 1);
        return py::make_tuple(grad_tuple(s), ga);
      },
      py::arg("prob"), py::arg("w"), py::arg("field") = true);

  // The operator applied to a global interior array, and the residual field
  // B − A w (pe/fields.hpp apply_operator / residual_field): (sum, field) with
  // the field of shape (M-1, N-1) — or None with field=False.  sum =
  // h1·h2·Σ v·(A v), or h1·h2·Σ (B − A w)².
  m.def(
      "apply_operator",
      [](const Problem& P, py::object v, bool field, int threads, py::object reaction) {
        FieldArr h, hc;
        const double* p = field_ptr(v, int64_t(P.M) - 1, int64_t(P.N) - 1, "v", h);
        if (!p) throw std::invalid_argument("apply_operator: the array is None");
        const double* c = field_ptr(reaction, int64_t(P.M) - 1, int64_t(P.N) - 1, "reaction", hc);
        std::vector<double> out(field ? size_t((int64_t(P.M) - 1) * (int64_t(P.N) - 1)) : 0);
        double sum;
        {
          py::gil_scoped_release nogil;
          sum = apply_operator(P, p, field ? out.data() : nullptr, threads, c);
        }
        py::object oa = py::none();
        if (field) oa = to_array(std::move(out), P.M - 1, P.N - 1);
        return py::make_tuple(sum, oa);
      },
      py::arg("prob"), py::arg("v"), py::arg("field") = true, py::arg("threads") = 1, py::arg("reaction") = py::none());
  m.def(
      "residual_field",
      [](const Problem& P, py::object w, py::object rhs, bool field, int threads, py::object reaction) {
        FieldArr h, hr, hc;
        const double* c = field_ptr(reaction, int64_t(P.M) - 1, int64_t(P.N) - 1, "reaction", hc);
        const double* p = field_ptr(w, int64_t(P.M) - 1, int64_t(P.N) - 1, "w", h);
        if (!p) throw std::invalid_argument("residual_field: the array is None");
        const double* r = field_ptr(rhs, int64_t(P.M) - 1, int64_t(P.N) - 1, "rhs", hr);
        std::vector<double> out(field ? size_t((int64_t(P.M) - 1) * (int64_t(P.N) - 1)) : 0);
        double sum;
        {
          py::gil_scoped_release nogil;
          sum = residual_field(P, p, r, field ? out.data() : nullptr, threads, c);
        }
        py::object oa = py::none();
        if (field) oa = to_array(std::move(out), P.M - 1, P.N - 1);
        return py::make_tuple(sum, oa);
      },
      py::arg("prob"), py::arg("w"), py::arg("rhs") = py::none(), py::arg("field") = true, py::arg("threads") = 1,
      py::arg("reaction") = py::none());

  m.def("host_coefficients", [](const Problem& P, const Block& blk) {
    std::vector<double> a, b;
    std::vector<int> c;
    host_coefficients(P, blk, a, b, c);
    const int64_t R = blk.nx + 2, C = blk.ny + 2;
    auto* heap = new std::vector<int>(std::move(c));
    py::capsule owner(heap, [](void* p) { delete static_cast<std::vector<int>*>(p); });
    py::array_t<int> ca({R, C}, {C * int64_t(sizeof(int)), int64_t(sizeof(int))}, heap->data(), owner);
    return py::make_tuple(to_array(std::move(a), R, C), to_array(std::move(b), R, C), ca);
  });

  // ---- item layouts (host only: no device needed) -----------------------
  m.def(
      "sweep_geometry",
      [](int64_t nx, int64_t ny, int steps) {
        const SweepGeometry g = sweep_geometry(nx, ny, steps, true);
        py::dict d;
        d["fsw"] = g.fsw;
        d["hdep"] = g.hdep;
        d["xorg"] = g.xorg;
        d["strips"] = g.strips;
        d["plane"] = g.plane;
        d["rows_hi"] = g.rows_hi;
        d["cols_hi"] = g.cols_hi;
        d["tab_lo"] = g.tab_lo;
        d["xsize"] = g.xsize;
        d["wsize"] = g.wsize;
        return d;
      },
      py::arg("nx"), py::arg("ny"), py::arg("steps"), "field planes, strips and table ranges of a block's sweep");
  m.def(
      "ti_candidates",
      [](int64_t nx, int64_t ny, int steps, int wave_cap) {
        return ti_candidates(sweep_geometry(nx, ny, steps, true), nx, ny, wave_cap);
      },
      py::arg("nx"), py::arg("ny"), py::arg("steps"), py::arg("wave_cap") = 2048,
      "rows-per-item candidates of the construction's tuning");
  m.def(
      "item_layout",
      [](const Problem& P, const Block& blk, int steps, int ti, int order, bool overlap, const std::string& layout,
         std::pair<int, int> wave_caps, int cus, int ov_reserve, double young, int wperm, int ov_debug,
         const std::string& force_layout) {
        LayoutRequest q;
        q.ti = ti;
        q.order = order;
        q.overlap = overlap;
        q.name = layout;
        q.wave_caps[0] = wave_caps.first;
        q.wave_caps[1] = wave_caps.second;
        q.wave_cap = std::min(wave_caps.first, wave_caps.second);
        q.cus = cus;
        q.ov_reserve = ov_reserve;
        q.knobs.young = young;
        q.knobs.wperm = wperm;
        q.knobs.ov_debug = ov_debug;
        q.knobs.force_layout = force_layout;
        const ItemLayout l = block_planner(P, blk, steps).build(q);
        py::dict d;
        d["entries"] = entry_tuples(l.list);
        d["boundary"] = l.lnb[0];
        d["shards"] = l.lnsh;
        d["lbase"] = std::vector<int>(l.lbase, l.lbase + 9);
        d["lnb"] = std::vector<int>(l.lnb, l.lnb + 8);
        d["waves"] = l.lwaves;
        d["name"] = l.name;
        d["cuts"] = l.cuts;
        d["load"] = std::vector<double>{l.max, l.mean, double(l.items)};
        d["nblocks"] = l.nblocks;
        d["nslots"] = l.nslots;
        return d;
      },
      py::arg("prob"), py::arg("block"), py::arg("steps"), py::arg("ti"), py::arg("order") = 0,
      py::arg("overlap") = false, py::arg("layout") = "lpt", py::arg("wave_caps") = std::make_pair(2048, 2048),
      py::arg("cus") = 256, py::arg("ov_reserve") = 8, py::arg("young") = 1.0, py::arg("wperm") = 0,
      py::arg("ov_debug") = 0, py::arg("force_layout") = "",
      "the item list a solver of this block would walk (the defaults: two 4-wave workgroups on each of 256 CUs)");

  m.def(
      "planner_row_classes",
      [](const Problem& P, const Block& blk, int steps) {
        const LayoutPlanner pl = block_planner(P, blk, steps);
        const std::vector<int>& rc = pl.row_classes();
        const int64_t R = int64_t(rc.size() / 4);
        py::array_t<int> a({R, int64_t(4)});
        std::copy(rc.begin(), rc.begin() + R * 4, a.mutable_data());
        return py::make_tuple(a, pl.tab_lo());
      },
      py::arg("prob"), py::arg("block"), py::arg("steps"),
      "the row classes item_layout plans from: ({in_lo, in_hi, out_lo, out_hi} per local row, first local row)");

  // ---- the solver's plan (host only: no device needed) -------------------
  m.def(
      "solver_plan",
      [](const Problem& P, const Block& blk, int comm_size, const SolveOptions& opt, std::optional<int> pe_resident,
         std::optional<int> pe_steps, std::optional<int> pe_ti, std::optional<int> pe_order, std::optional<int> pe_ti_tune,
         int cus, int per_cu, int per_cu0, std::optional<bool> resident) {
        const SolverKnobs knobs{pe_resident, pe_steps, pe_ti, pe_order, pe_ti_tune};
        SolverPlan pl = plan_solver(P, blk, comm_size, opt, knobs, cus);
        finish_plan(pl, blk, DeviceFacts{cus, per_cu, per_cu0});
        // (the resident kernel's own further conditions are the device's: without its answer, the estimate)
        const bool res = resident ? *resident
                                  : pl.resident_likely && pl.fused && !pl.sstep && comm_size == 1 && blk.Px * blk.Py == 1;
        const ChunkPlan ch = plan_chunk(pl, blk, comm_size, opt.chunk, res);
        py::dict d;
        d["fused"] = pl.fused;
        d["steps"] = pl.steps;
        d["resident_likely"] = pl.resident_likely;
        d["ti"] = pl.ti;
        d["ti_query"] = pl.ti_query;
        d["order"] = pl.order;
        d["layout"] = pl.lay_name;
        d["strips"] = pl.geo.strips;
        d["wave_caps"] = py::make_tuple(pl.wave_caps[0], pl.wave_caps[1]);
        d["tune_ti"] = pl.tune_ti;
        d["candidates"] = pl.ti_cands;
        d["ti_min"] = pl.ti_min;
        d["npart"] = pl.npart;
        d["nitems_max"] = pl.nitems_max;
        d["nslot_cap"] = pl.nslot_cap;
        d["resident"] = res;
        d["chunk"] = ch.chunk;
        d["stream_chunk"] = ch.stream_chunk;
        d["algo"] = algo_name(pl.fused, pl.steps, res);
        return d;
      },
      py::arg("prob"), py::arg("block"), py::arg("comm_size") = 1, py::arg("opt") = SolveOptions(),
      py::arg("pe_resident") = py::none(), py::arg("pe_steps") = py::none(), py::arg("pe_ti") = py::none(),
      py::arg("pe_order") = py::none(), py::arg("pe_ti_tune") = py::none(), py::arg("cus") = 256, py::arg("per_cu") = 0,
      py::arg("per_cu0") = 0, py::arg("resident") = py::none(),
      "what a DeviceSolver of this block decides: kernel family, iterations per sweep, rows per item, order, tuning, "
      "capacities, chunk (pe_*: the parsed PE_* knobs, None: unset; per_cu / per_cu0: resident blocks per CU of the "
      "applying / deferring sweep; resident: whether the resident kernel runs, None: the estimate)");
  m.def(
      "resident_tiling",
      [](int64_t nx, int64_t ny, int cus) -> py::object {
        const std::optional<ResidentTiling> t = resident_tiling(nx, ny, cus);
        if (!t) return py::none();
        py::dict d;
        d["strips"] = t->nstrips;
        d["bands"] = t->ntr;
        d["rowstart"] = t->rowstart;
        d["rcap"] = t->rcap;
        return std::move(d);
      },
      py::arg("nx"), py::arg("ny"), py::arg("cus"), "the LDS-resident kernel's tile geometry of a block, or None");
  m.def(
      "halo_candidates",
      [](int steps, bool put_ok, bool push_ok, bool shared_dev, int nheights, std::vector<int> heights,
         std::optional<std::string> pe_halo, std::optional<int> pe_overlap) {
        const HaloCandidates hc =
            halo_candidates(HaloInputs{steps, put_ok, push_ok, shared_dev, nheights, std::move(heights), pe_halo, pe_overlap});
        py::list l;
        for (const HaloCandidate& c : hc.list) l.append(py::make_tuple(c.path, c.overlap, c.ti));
        return py::make_tuple(l, hc.put_ov_late);
      },
      py::arg("steps"), py::arg("put_ok") = false, py::arg("push_ok") = false, py::arg("shared_dev") = false,
      py::arg("nheights") = 1, py::arg("heights") = std::vector<int>{0}, py::arg("pe_halo") = py::none(),
      py::arg("pe_overlap") = py::none(),
      "([(path, overlap, rows per item)], put_ov_late): the halo-path candidates in timing order");

  // ---- device (HIP / RCCL) ----------------------------------------------
  m.def("device_count", &device_count);
  m.def("set_device", &set_device);
  m.def("device_name", &device_name);
  m.def("current_device", &current_device);
  m.def("device_pci_bus_id", &device_pci_bus_id, py::arg("dev"));
  m.def("rccl_unique_id", []() { return py::bytes(rccl_unique_id()); });

  py::class_<CommHandle>(m, "DeviceComm")
      .def_property_readonly("rank", [](const CommHandle& h) { return h.comm->rank(); })
      .def_property_readonly("size", [](const CommHandle& h) { return h.comm->size(); })
      .def_property_readonly("name", [](const CommHandle& h) { return h.comm->name(); })
      .def(
          "bench_allreduce",
          [](CommHandle& h, int n, int iters) {
            // stream-ordered latency of the in-place sum of n doubles (collective)
            py::gil_scoped_release nogil;
            double* d = nullptr;
            hipStream_t s = nullptr;
            hipEvent_t e0, e1;
            PE_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            PE_HIP_CHECK(hipMalloc(&d, sizeof(double) * std::max(1, n)));
            PE_HIP_CHECK(hipMemsetAsync(d, 0, sizeof(double) * std::max(1, n), s));
            PE_HIP_CHECK(hipEventCreate(&e0));
            PE_HIP_CHECK(hipEventCreate(&e1));
            for (int i = 0; i < 5; ++i) h.comm->allreduce_sum(d, n, s);
            h.comm->barrier(s);
            PE_HIP_CHECK(hipEventRecord(e0, s));
            for (int i = 0; i < iters; ++i) h.comm->allreduce_sum(d, n, s);
            PE_HIP_CHECK(hipEventRecord(e1, s));
            PE_HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.f;
            PE_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            (void)hipFree(d);
            (void)hipStreamDestroy(s);
            return 1e3 * double(ms) / std::max(1, iters);
          },
          py::arg("n") = 7, py::arg("iters") = 1000,
          "Microseconds per in-place allreduce_sum of n doubles (call on every rank).");
  m.def(
      "make_rccl_comm",
      [](py::bytes uid, int rank, int size) {
        auto h = std::make_unique<CommHandle>();
        std::string s = uid;
        py::gil_scoped_release nogil;
        h->comm = make_rccl_comm(s, rank, size);
        return h;
      },
      py::arg("uid"), py::arg("rank"), py::arg("size"));
  m.def(
      "make_delay_comm",
      [](int size, double exchange_us, double allreduce_us, bool loopback) {
        auto h = std::make_unique<CommHandle>();
        h->comm = make_delay_comm(size, exchange_us, allreduce_us, loopback);
        return h;
      },
      py::arg("size"), py::arg("exchange_us"), py::arg("allreduce_us"), py::arg("loopback") = false);
  m.def(
      "make_host_staged_comm",
      [](int rank, int size, py::function reduce_fn, py::function exchange_fn, py::function barrier_fn) {
        auto reduce = [reduce_fn](double* buf, int n, bool is_max) {
          py::gil_scoped_acquire g;
          py::array_t<double> a({n}, {int64_t(sizeof(double))}, buf, py::none());
          reduce_fn(a, is_max);
        };
        auto exch = [exchange_fn](const std::vector<Exchange>& ex) {
          py::gil_scoped_acquire g;
          py::list items;
          for (const auto& e : ex) {
            py::array_t<double> s({e.count}, {int64_t(sizeof(double))}, const_cast<double*>(e.send), py::none());
            py::array_t<double> r({e.count}, {int64_t(sizeof(double))}, e.recv, py::none());
            items.append(py::make_tuple(e.dir, e.peer, s, r));
          }
          exchange_fn(items);
        };
        auto bar = [barrier_fn]() {
          py::gil_scoped_acquire g;
          barrier_fn();
        };
        auto h = std::make_unique<CommHandle>();
        h->comm = make_callback_device_comm(rank, size, reduce, exch, bar);
        return h;
      },
      py::arg("rank"), py::arg("size"), py::arg("reduce_fn"), py::arg("exchange_fn"), py::arg("barrier_fn"));
  m.def(
      "use_p2p_allreduce",
      [](CommHandle& h) {
        py::gil_scoped_release nogil;
        h.comm = make_p2p_allreduce_comm(std::move(h.comm));
      },
      py::arg("comm"),
      "Switch the per-iteration sums of this communicator to the one-shot P2P allreduce (collective: call on "
      "every rank).");
  m.def(
      "make_rccl_comm_from_handle",
      [](uintptr_t handle) {
        auto h = std::make_unique<CommHandle>();
        h->comm = make_rccl_comm_from_handle(reinterpret_cast<void*>(handle));
        return h;
      },
      py::arg("nccl_comm_ptr"));

  py::class_<DeviceSolver>(m, "DeviceSolver")
      .def(py::init([](const Problem& P, const Block& blk, CommHandle* comm, const SolveOptions& opt) {
             return std::make_unique<DeviceSolver>(P, blk, comm ? comm->comm.get() : nullptr, opt);
           }),
           py::arg("prob"), py::arg("block"), py::arg("comm") = nullptr, py::arg("opt") = SolveOptions(),
           py::keep_alive<1, 4>())
      .def("solve",
           [](DeviceSolver& s) {
             py::gil_scoped_release nogil;
             return s.solve();
           })
      .def("reset", [](DeviceSolver& s) {
        py::gil_scoped_release nogil;
        s.reset();
        s.synchronize();
      })
      .def("run_iterations",
           [](DeviceSolver& s, int64_t n, bool g) {
             py::gil_scoped_release nogil;
             s.run_iterations(n, g);
           },
           py::arg("iters"), py::arg("use_graph") = true)
      .def("set_check_tol", &DeviceSolver::set_check_tol, py::arg("on"))
      .def("set_atol", &DeviceSolver::set_atol, py::arg("atol"),
           "the residual rule's absolute floor of the next solves (ValueError under the step-size rule, or not finite / < 0)")
      .def("set_init", &DeviceSolver::set_init, py::arg("init"), py::arg("seed") = 1234, py::arg("amp") = 0.05)
      .def(
          "set_rhs",
          [](DeviceSolver& s, py::object owned) {
            FieldArr h;
            s.set_rhs(field_ptr(owned, s.block().nx, s.block().ny, "rhs", h));
          },
          py::arg("owned"), "this block's nx × ny slice of the right-hand side (block_fields), or None for F")
      .def(
          "set_w0",
          [](DeviceSolver& s, py::object ringed) {
            FieldArr h;
            s.set_w0(field_ptr(ringed, s.block().nx + 2, s.block().ny + 2, "w0", h));
          },
          py::arg("ringed"),
          "this block's (nx+2) × (ny+2) slice of the initial guess with its ring (block_fields), or None for init")
      .def(
          "set_rhs_device",
          [](DeviceSolver& s, uintptr_t ptr, int64_t si, int64_t sj, bool f32, uintptr_t stream) {
            s.set_rhs_device(reinterpret_cast<const void*>(ptr), si, sj, f32, reinterpret_cast<hipStream_t>(stream));
          },
          py::arg("ptr"), py::arg("stride_i"), py::arg("stride_j"), py::arg("f32") = false, py::arg("stream") = 0,
          "the right-hand side as the GLOBAL (M-1) × (N-1) array in device memory: address of element [0][0], "
          "element strides, float32 flag, the producing stream's handle (0 clears the field when ptr is 0)")
      .def(
          "set_w0_device",
          [](DeviceSolver& s, uintptr_t ptr, int64_t si, int64_t sj, bool f32, uintptr_t stream) {
            s.set_w0_device(reinterpret_cast<const void*>(ptr), si, sj, f32, reinterpret_cast<hipStream_t>(stream));
          },
          py::arg("ptr"), py::arg("stride_i"), py::arg("stride_j"), py::arg("f32") = false, py::arg("stream") = 0,
          "the initial guess as the GLOBAL (M-1) × (N-1) array in device memory (see set_rhs_device)")
      .def(
          "set_reaction",
          [](DeviceSolver& s, py::object ringed) {
            FieldArr h;
            s.set_reaction(field_ptr(ringed, s.block().nx + 2, s.block().ny + 2, "reaction", h));
          },
          py::arg("ringed"),
          "this block's (nx+2) × (ny+2) slice of the reaction field with its ring (block_field ring 1); a solver "
          "constructed with Problem.reaction only, None refused")
      .def(
          "set_reaction_device",
          [](DeviceSolver& s, uintptr_t ptr, int64_t si, int64_t sj, bool f32, uintptr_t stream) {
            s.set_reaction_device(reinterpret_cast<const void*>(ptr), si, sj, f32, reinterpret_cast<hipStream_t>(stream));
          },
          py::arg("ptr"), py::arg("stride_i"), py::arg("stride_j"), py::arg("float32") = false, py::arg("stream") = 0,
          "the reaction field as the GLOBAL (M-1) × (N-1) array in device memory (see set_rhs_device)")
      .def(
          "set_exact",
          [](DeviceSolver& s, py::object owned) {
            FieldArr h;
            s.set_exact(field_ptr(owned, s.block().nx, s.block().ny, "exact", h));
          },
          py::arg("owned"),
          "this block's nx × ny slice of the exact solution the error is taken against (block_field), or None for "
          "the analytic one")
      .def(
          "set_exact_device",
          [](DeviceSolver& s, uintptr_t ptr, int64_t si, int64_t sj, bool f32, uintptr_t stream) {
            s.set_exact_device(reinterpret_cast<const void*>(ptr), si, sj, f32, reinterpret_cast<hipStream_t>(stream));
          },
          py::arg("ptr"), py::arg("stride_i"), py::arg("stride_j"), py::arg("f32") = false, py::arg("stream") = 0,
          "the exact solution as the GLOBAL (M-1) × (N-1) array in device memory (see set_rhs_device)")
      .def(
          "copy_w_device",
          [](DeviceSolver& s, uintptr_t ptr, int64_t si, int64_t sj, int64_t off_i, int64_t off_j, uintptr_t stream) {
            s.copy_w_device(reinterpret_cast<double*>(ptr), si, sj, off_i, off_j, reinterpret_cast<hipStream_t>(stream));
          },
          py::arg("ptr"), py::arg("stride_i"), py::arg("stride_j"), py::arg("off_i") = 0, py::arg("off_j") = 0,
          py::arg("stream") = 0,
          "the owned w into float64 device memory at element offset (off_i, off_j) of `ptr`, ordered with `stream`")
      .def(
          "gradient",
          [](DeviceSolver& s, bool field) {
            const Block& b = s.block();
            std::vector<double> gx, gy;
            if (field) {
              gx.resize(size_t(b.nx * b.ny));
              gy.resize(size_t(b.nx * b.ny));
            }
            GradStats g;
            {
              py::gil_scoped_release nogil;
              g = s.gradient(field ? gx.data() : nullptr, field ? gy.data() : nullptr);
            }
            py::object ax = py::none(), ay = py::none();
            if (field) {
              ax = to_array(std::move(gx), b.nx, b.ny);
              ay = to_array(std::move(gy), b.nx, b.ny);
            }
            return py::make_tuple(grad_tuple(g), ax, ay);
          },
          py::arg("field") = true,
          "after solve(): ((integral, energy, grad_max), gx, gy) of w on this block's owned nodes (field=False: the "
          "functionals only, gx = gy = None); collective on a multi-rank job; only reset() / solve() may follow")
      .def(
          "gradient_device",
          [](DeviceSolver& s, uintptr_t gx, uintptr_t gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j,
             uintptr_t stream) {
            GradStats g;
            {
              py::gil_scoped_release nogil;
              g = s.gradient_device(reinterpret_cast<double*>(gx), reinterpret_cast<double*>(gy), si, sj, off_i, off_j,
                                    reinterpret_cast<hipStream_t>(stream));
            }
            return grad_tuple(g);
          },
          py::arg("gx"), py::arg("gy"), py::arg("stride_i"), py::arg("stride_j"), py::arg("off_i") = 0,
          py::arg("off_j") = 0, py::arg("stream") = 0,
          "the same with gx / gy written into float64 device memory at element offset (off_i, off_j), ordered with "
          "`stream` (both addresses 0: the functionals only); returns (integral, energy, grad_max)")
      .def(
          "apply",
          [](DeviceSolver& s, py::object v, bool resid, bool field) {
            FieldArr h;
            const double* p = field_ptr(v, int64_t(s.problem().M) - 1, int64_t(s.problem().N) - 1, "field", h);
            if (!p) throw std::invalid_argument("apply: the array is None");
            const Block& b = s.block();
            std::vector<double> out(field ? size_t(b.nx * b.ny) : 0);
            double sum;
            {
              py::gil_scoped_release nogil;
              sum = resid ? s.residual(p, field ? out.data() : nullptr) : s.apply(p, field ? out.data() : nullptr);
            }
            py::object oa = py::none();
            if (field) oa = to_array(std::move(out), b.nx, b.ny);
            return py::make_tuple(sum, oa);
          },
          py::arg("v"), py::arg("residual") = false, py::arg("field") = true,
          "(sum, field) of A v — or (residual) of B − A v, B the rhs that is set, else F — for the GLOBAL (M-1) × "
          "(N-1) host array v: the field on this block's owned nodes (field=False: None), sum = the job's h1 h2 Σ "
          "v·(A v) or h1 h2 Σ (B − A v)²; collective on a multi-rank job; disturbs no state of the solve")
      .def(
          "apply_device",
          [](DeviceSolver& s, uintptr_t ptr, int64_t si, int64_t sj, bool f32, bool resid, uintptr_t dst, int64_t dsi,
             int64_t dsj, int64_t off_i, int64_t off_j, uintptr_t stream) {
            py::gil_scoped_release nogil;
            const void* v = reinterpret_cast<const void*>(ptr);
            double* d = reinterpret_cast<double*>(dst);
            hipStream_t st = reinterpret_cast<hipStream_t>(stream);
            return resid ? s.residual_device(v, si, sj, f32, d, dsi, dsj, off_i, off_j, st)
                         : s.apply_device(v, si, sj, f32, d, dsi, dsj, off_i, off_j, st);
          },
          py::arg("ptr"), py::arg("stride_i"), py::arg("stride_j"), py::arg("f32") = false, py::arg("residual") = false,
          py::arg("dst") = 0, py::arg("dst_stride_i") = 0, py::arg("dst_stride_j") = 0, py::arg("off_i") = 0,
          py::arg("off_j") = 0, py::arg("stream") = 0,
          "the same with the GLOBAL array in device memory (address of element [0][0], element strides, float32 "
          "flag) and the owned part written into float64 device memory at element offset (off_i, off_j) of `dst` "
          "(0: the sum only), ordered with `stream`; returns the sum")
      .def(
          "user_plane",
          [](DeviceSolver& s, int which) -> py::object {
            std::vector<double> v = s.user_plane(which);
            if (v.empty()) return py::none();
            const int64_t ring = which == 1 ? 1 : 0;
            return to_array(std::move(v), s.block().nx + 2 * ring, s.block().ny + 2 * ring);
          },
          py::arg("which"), "host copy of the user plane the solve reads (0 rhs, 1 w0, 2 exact), None when unset")
      .def_property_readonly("user_rhs", &DeviceSolver::user_rhs)
      .def_property_readonly("user_w0", &DeviceSolver::user_w0)
      .def_property_readonly("user_exact", &DeviceSolver::user_exact)
      .def("relayout", &DeviceSolver::relayout, py::arg("ti"), py::arg("order") = -1)
      .def("prepare_graphs",
           [](DeviceSolver& s, int64_t n) {
             py::gil_scoped_release nogil;
             s.prepare_graphs(n);
           },
           py::arg("iters"))
      .def("time_iterations",
           [](DeviceSolver& s, int64_t n, bool g) {
             py::gil_scoped_release nogil;
             return s.time_iterations(n, g);
           },
           py::arg("iters"), py::arg("use_graph") = true)
      .def("synchronize", [](DeviceSolver& s) {
        py::gil_scoped_release nogil;
        s.synchronize();
      })
      .def("state",
           [](DeviceSolver& s) {
             dev::DevState st;
             s.read_state(&st);
             return state_dict(st);
           })
      .def("w",
           [](DeviceSolver& s) {
             const Block& b = s.block();
             std::vector<double> v(size_t(b.nx * b.ny));
             s.copy_w(v.data());
             return to_array(std::move(v), b.nx, b.ny);
           })
      .def("field",
           [](DeviceSolver& s, int which) {
             std::vector<double> v(size_t(s.field_rows() * s.field_cols()));
             s.copy_field(which, v.data());
             return to_array(std::move(v), s.field_rows(), s.field_cols());
           })
      .def_property_readonly("chunk", &DeviceSolver::chunk)
      .def_property_readonly("fused", &DeviceSolver::fused)
      .def_property_readonly("two_step", &DeviceSolver::two_step, "several iterations per sweep (fused2.hip / fused3.hip)")
      .def_property_readonly("sweep_steps", &DeviceSolver::sweep_steps, "iterations per sweep launch (1, 2, 3)")
      .def_property_readonly("resident", &DeviceSolver::resident)
      .def_property_readonly("resident_fallback", &DeviceSolver::resident_fallback)
      .def_property_readonly("layout_cuts", &DeviceSolver::layout_cuts)
      .def_property_readonly("layout_name", &DeviceSolver::layout_name, "static item layout: lpt / fill / equal")
      .def_property_readonly(
          "layout_entries",
          [](const DeviceSolver& s) {
            // (first row, rows, strip, flags) per list position; rows 0: an empty position
            return entry_tuples(s.layout_entries());
          },
          "the static item list: (first row, rows, strip, flags: kBandBit | kUniBit)")
      .def_property_readonly(
          "layout_request",
          [](const DeviceSolver& s) {
            const LayoutRequest& q = s.layout_request();
            py::dict d;
            d["prob"] = s.problem();
            d["block"] = s.block();
            d["steps"] = s.sweep_steps();
            d["ti"] = q.ti;
            d["order"] = q.order;
            d["overlap"] = q.overlap;
            d["layout"] = q.name;
            d["wave_caps"] = py::make_tuple(q.wave_caps[0], q.wave_caps[1]);
            d["cus"] = q.cus;
            d["ov_reserve"] = q.ov_reserve;
            d["young"] = q.knobs.young;
            d["wperm"] = q.knobs.wperm;
            d["ov_debug"] = q.knobs.ov_debug;
            d["force_layout"] = q.knobs.force_layout;
            return d;
          },
          "what the solver last asked the layout planner: the keyword arguments of item_layout()")
      .def_property_readonly(
          "plan_request",
          [](const DeviceSolver& s) {
            const SolverKnobs& kn = s.plan_knobs();
            py::dict d;
            d["prob"] = s.problem();
            d["block"] = s.block();
            d["comm_size"] = s.comm_size();
            d["opt"] = s.options();
            d["pe_resident"] = kn.resident;
            d["pe_steps"] = kn.steps;
            d["pe_ti"] = kn.ti;
            d["pe_order"] = kn.order;
            d["pe_ti_tune"] = kn.ti_tune;
            d["cus"] = s.plan_facts().cus;
            d["per_cu"] = s.plan_facts().per_cu;
            d["per_cu0"] = s.plan_facts().per_cu0;
            d["resident"] = s.resident();
            return d;
          },
          "what the solver's plan was made with: the keyword arguments of solver_plan()")
      .def_property_readonly(
          "halo_request",
          [](const DeviceSolver& s) {
            const HaloInputs& in = s.halo_inputs();
            py::dict d;
            d["steps"] = in.steps;
            d["put_ok"] = in.put_ok;
            d["push_ok"] = in.push_ok;
            d["shared_dev"] = in.shared_dev;
            d["nheights"] = in.nheights;
            d["heights"] = in.heights;
            d["pe_halo"] = in.halo;
            d["pe_overlap"] = in.overlap;
            return d;
          },
          "what the halo-path choice asked for its candidates: the keyword arguments of halo_candidates()")
      .def_property_readonly("layout_waves", [](DeviceSolver& s) { return s.params().lwaves; })
      .def_property_readonly("strips", [](DeviceSolver& s) { return s.params().nstrips; }, "wave strips across the block")
      .def_property_readonly("layout_boundary", &DeviceSolver::layout_boundary,
                             "overlap: list positions 0 .. n-1 hold the boundary items (0: no overlap)")
      .def_property_readonly("peer_access", &DeviceSolver::peer_access,
                             "hipDeviceCanAccessPeer toward each rank's device (1/0; -1 same device)")
      .def_property_readonly("push_status", &DeviceSolver::push_status, "halo push: on / off: why / fallback: why")
      .def_property_readonly("xr_status", &DeviceSolver::xr_status, "transport of the per-sweep sums")
      .def_property_readonly("overlap", &DeviceSolver::overlap)
      .def_property_readonly("halo_push", &DeviceSolver::halo_push,
                             "halo rows pushed by the sweep over xGMI (no exchange call; graph-capturable)")
      .def_property_readonly("halo_put", &DeviceSolver::halo_put,
                             "halo phases exchanged by the peer-put kernel (p2p.hip kPut) instead of the comm")
      .def_property_readonly("halo_path", &DeviceSolver::halo_path,
                             "the multi-rank halo path chosen at construction (exchange / put / push [+overlap])")
      .def_property_readonly("halo_candidates", &DeviceSolver::halo_candidates,
                             "[(path, µs per sweep)] as timed by the construction's halo-path choice (max over ranks)")
      .def_property_readonly("graphs_usable", &DeviceSolver::graphs_usable)
      .def("set_halo_path", &DeviceSolver::set_halo_path, py::arg("path"), py::arg("overlap"),
           "probe: switch to another halo path candidate (exchange / put / push, overlap)")
      .def("time_halo_path", &DeviceSolver::time_halo_path, py::arg("sweeps") = 4, py::arg("warm") = 2,
           py::arg("from_reset") = true, "probe: ms per sweep of the current halo path")
      .def_property_readonly("put_status", &DeviceSolver::put_status, "peer put: available / off: why / fallback: why")
      .def("save_checkpoint", &DeviceSolver::save_checkpoint, py::arg("path"))
      .def("load_checkpoint", &DeviceSolver::load_checkpoint, py::arg("path"))
      .def_property_readonly("fields_address", &DeviceSolver::fields_address)
      .def_property_readonly("placement_ms", &DeviceSolver::placement_ms)
      .def_property_readonly("placement_choice", &DeviceSolver::placement_choice)
      .def_property_readonly("placement_s", &DeviceSolver::placement_seconds)
      .def_property_readonly("placement_job_ms", &DeviceSolver::placement_job_ms)
      .def_property_readonly("construct_s", &DeviceSolver::construct_seconds)
      .def_property_readonly("exchange_us", &DeviceSolver::exchange_us)
      .def_property_readonly("ti_tuning_ms", &DeviceSolver::ti_tuning_ms)
      .def_property_readonly("ti_tuning_rows", &DeviceSolver::ti_tuning_rows)
      .def_property_readonly("layout_load", &DeviceSolver::layout_load)
      .def_property_readonly("ti", [](DeviceSolver& s) { return s.params().ti; })
      .def_property_readonly("order", [](DeviceSolver& s) { return s.params().order; })
      .def_property_readonly("xr", [](DeviceSolver& s) { return s.params().xr.peers != nullptr; },
                             "True when the sweep sums its scalars over ranks itself (P2P transport)")
      .def_property_readonly("nitems", [](DeviceSolver& s) { return s.params().nslots; })
      .def_property_readonly("stamp_waves",
                             [](DeviceSolver& s) { return dev::kWPB * std::max(s.params().nblocks, s.params().nblocks0); })
      .def("stamps",
           [](DeviceSolver& s) {
             std::vector<unsigned long long> v = s.stamps();
             py::array_t<unsigned long long> a(py::ssize_t(v.size()));
             if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), sizeof(unsigned long long) * v.size());
             return a;
           },
           "PE_STAMPS=1 diagnostic timeline of the last sweep (tools/stamp_probe.py).")
      .def("clear_stamps", &DeviceSolver::clear_stamps)
      .def_property_readonly("blocks", [](DeviceSolver& s) { return dev::grid_blocks(s.params()); })
      .def_property_readonly("block", &DeviceSolver::block);

  m.def(
      "device_solve_group",
      [](const Problem& P, int ranks, DecompMode mode, const SolveOptions& opt, bool return_w) {
        std::vector<double> w;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = device_solve_group(P, ranks, mode, opt, return_w ? &w : nullptr);
        }
        py::object wa = py::none();
        if (return_w) wa = to_array(std::move(w), P.M - 1, P.N - 1);
        return py::make_tuple(r, wa);
      },
      py::arg("prob"), py::arg("ranks"), py::arg("mode") = DecompMode::Aspect, py::arg("opt") = SolveOptions(),
      py::arg("return_w") = false);

  m.def(
      "device_solve_group_grid",
      [](const Problem& P, const ProcessGrid& pg, const SolveOptions& opt, bool return_w, py::object rhs,
         py::object w0, py::object exact, py::object reaction) {
        FieldArr hr, hw, he, hc;
        UserFields uf;
        uf.rhs = field_ptr(rhs, P.M - 1, P.N - 1, "rhs", hr);
        uf.w0 = field_ptr(w0, P.M - 1, P.N - 1, "w0", hw);
        uf.exact = field_ptr(exact, P.M - 1, P.N - 1, "exact", he);
        uf.reaction = field_ptr(reaction, P.M - 1, P.N - 1, "reaction", hc);
        std::vector<double> w;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = device_solve_group(P, pg, opt, return_w ? &w : nullptr, uf);
        }
        py::object wa = py::none();
        if (return_w) wa = to_array(std::move(w), P.M - 1, P.N - 1);
        return py::make_tuple(r, wa);
      },
      py::arg("prob"), py::arg("grid"), py::arg("opt") = SolveOptions(), py::arg("return_w") = false,
      py::arg("rhs") = py::none(), py::arg("w0") = py::none(), py::arg("exact") = py::none(),
      py::arg("reaction") = py::none());

  // The same with fields and / or the result in device memory: rhs_dev /
  // w0_dev / exact_dev = (address of element [0][0], stride_i, stride_j, float32 flag) of
  // the global interior array or None, w_dev = (address, stride_i, stride_j)
  // of a float64 (M-1) × (N-1) destination or None, `stream` the caller's
  // stream handle.  Host fields may be mixed in (a field given both ways is
  // taken from the device).
  m.def(
      "device_solve_group_grid_device",
      [](const Problem& P, const ProcessGrid& pg, const SolveOptions& opt, bool return_w, py::object rhs,
         py::object w0, py::object rhs_dev, py::object w0_dev, py::object w_dev, uintptr_t stream, py::object exact,
         py::object exact_dev, py::object reaction, py::object reaction_dev) {
        FieldArr hr, hw, he, hc;
        UserFields uf;
        uf.rhs = field_ptr(rhs, P.M - 1, P.N - 1, "rhs", hr);
        uf.w0 = field_ptr(w0, P.M - 1, P.N - 1, "w0", hw);
        uf.exact = field_ptr(exact, P.M - 1, P.N - 1, "exact", he);
        uf.reaction = field_ptr(reaction, P.M - 1, P.N - 1, "reaction", hc);
        DeviceFields df;
        device_spec(reaction_dev, df.reaction, df.reaction_si, df.reaction_sj, df.reaction_f32);
        df.stream = reinterpret_cast<hipStream_t>(stream);
        device_spec(rhs_dev, df.rhs, df.rhs_si, df.rhs_sj, df.rhs_f32);
        device_spec(w0_dev, df.w0, df.w0_si, df.w0_sj, df.w0_f32);
        device_spec(exact_dev, df.exact, df.exact_si, df.exact_sj, df.exact_f32);
        if (!w_dev.is_none()) {
          auto t = w_dev.cast<std::tuple<uintptr_t, int64_t, int64_t>>();
          df.w_dst = reinterpret_cast<double*>(std::get<0>(t));
          df.w_si = std::get<1>(t);
          df.w_sj = std::get<2>(t);
        }
        std::vector<double> w;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = device_solve_group(P, pg, opt, return_w ? &w : nullptr, uf, df);
        }
        py::object wa = py::none();
        if (return_w) wa = to_array(std::move(w), P.M - 1, P.N - 1);
        return py::make_tuple(r, wa);
      },
      py::arg("prob"), py::arg("grid"), py::arg("opt") = SolveOptions(), py::arg("return_w") = false,
      py::arg("rhs") = py::none(), py::arg("w0") = py::none(), py::arg("rhs_dev") = py::none(),
      py::arg("w0_dev") = py::none(), py::arg("w_dev") = py::none(), py::arg("stream") = 0,
      py::arg("exact") = py::none(), py::arg("exact_dev") = py::none(), py::arg("reaction") = py::none(),
      py::arg("reaction_dev") = py::none());

  // The same with the gradient of the solution (pe/fields.hpp): grad = 1 the
  // functionals only (the result's integral / energy / grad_max), 2 the field
  // as well — into grad_dev = (address of gx, address of gy, stride_i,
  // stride_j), two float64 (M-1) × (N-1) destinations in device memory, or
  // else returned as a (2, M-1, N-1) array.  Returns (result, w, gradient).
  m.def(
      "device_solve_group_grad",
      [](const Problem& P, const ProcessGrid& pg, const SolveOptions& opt, bool return_w, int grad, py::object rhs,
         py::object w0, py::object exact, py::object rhs_dev, py::object w0_dev, py::object exact_dev, py::object w_dev,
         py::object grad_dev, uintptr_t stream, py::object reaction, py::object reaction_dev) {
        if (grad != 1 && grad != 2) throw std::invalid_argument("grad: 1 (functionals) or 2 (field)");
        FieldArr hr, hw, he, hc;
        UserFields uf;
        uf.reaction = field_ptr(reaction, P.M - 1, P.N - 1, "reaction", hc);
        uf.rhs = field_ptr(rhs, P.M - 1, P.N - 1, "rhs", hr);
        uf.w0 = field_ptr(w0, P.M - 1, P.N - 1, "w0", hw);
        uf.exact = field_ptr(exact, P.M - 1, P.N - 1, "exact", he);
        DeviceFields df;
        df.stream = reinterpret_cast<hipStream_t>(stream);
        device_spec(reaction_dev, df.reaction, df.reaction_si, df.reaction_sj, df.reaction_f32);
        device_spec(rhs_dev, df.rhs, df.rhs_si, df.rhs_sj, df.rhs_f32);
        device_spec(w0_dev, df.w0, df.w0_si, df.w0_sj, df.w0_f32);
        device_spec(exact_dev, df.exact, df.exact_si, df.exact_sj, df.exact_f32);
        if (!w_dev.is_none()) {
          const auto t = w_dev.cast<std::tuple<uintptr_t, int64_t, int64_t>>();
          df.w_dst = reinterpret_cast<double*>(std::get<0>(t));
          df.w_si = std::get<1>(t);
          df.w_sj = std::get<2>(t);
        }
        if (!grad_dev.is_none()) {
          const auto t = grad_dev.cast<std::tuple<uintptr_t, uintptr_t, int64_t, int64_t>>();
          df.grad_x = reinterpret_cast<double*>(std::get<0>(t));
          df.grad_y = reinterpret_cast<double*>(std::get<1>(t));
          df.grad_si = std::get<2>(t);
          df.grad_sj = std::get<3>(t);
        }
        std::vector<double> w, g;
        GroupGradient gg;
        gg.stats = true;
        gg.host = grad == 2 && grad_dev.is_none() ? &g : nullptr;
        SolveResult r;
        {
          py::gil_scoped_release nogil;
          r = device_solve_group(P, pg, opt, return_w ? &w : nullptr, uf, df, gg);
        }
        py::object wa = py::none(), ga = py::none();
        if (return_w) wa = to_array(std::move(w), P.M - 1, P.N - 1);
        if (gg.host) ga = to_array(std::move(g), 2 * (int64_t(P.M) - 1), P.N - 1).attr("reshape")(2, P.M - 1, P.N - 1);
        return py::make_tuple(r, wa, ga);
      },
      py::arg("prob"), py::arg("grid"), py::arg("opt"), py::arg("return_w"), py::arg("grad"), py::arg("rhs") = py::none(),
      py::arg("w0") = py::none(), py::arg("exact") = py::none(), py::arg("rhs_dev") = py::none(),
      py::arg("w0_dev") = py::none(), py::arg("exact_dev") = py::none(), py::arg("w_dev") = py::none(),
      py::arg("grad_dev") = py::none(), py::arg("stream") = 0, py::arg("reaction") = py::none(),
      py::arg("reaction_dev") = py::none());

  // The operator (residual: B − A w) on P virtual ranks of one device: v / rhs
  // as host arrays or device specs (address, stride_i, stride_j, float32
  // flag); out_dev = (address, stride_i, stride_j) of a float64 (M-1) × (N-1)
  // destination, else field=True returns the array.  Returns (sum, field).
  m.def(
      "device_apply_group",
      [](const Problem& P, const ProcessGrid& pg, const SolveOptions& opt, bool residual, py::object v, py::object v_dev,
         py::object rhs, py::object rhs_dev, py::object out_dev, bool field, uintptr_t stream, py::object reaction,
         py::object reaction_dev) {
        FieldArr hv, hr, hc;
        OperatorFields f;
        f.reaction_host = field_ptr(reaction, P.M - 1, P.N - 1, "reaction", hc);
        device_spec(reaction_dev, f.reaction, f.reaction_si, f.reaction_sj, f.reaction_f32);
        f.v_host = field_ptr(v, P.M - 1, P.N - 1, "field", hv);
        f.rhs_host = field_ptr(rhs, P.M - 1, P.N - 1, "rhs", hr);
        device_spec(v_dev, f.v, f.v_si, f.v_sj, f.v_f32);
        device_spec(rhs_dev, f.rhs, f.rhs_si, f.rhs_sj, f.rhs_f32);
        f.stream = reinterpret_cast<hipStream_t>(stream);
        if (!out_dev.is_none()) {
          const auto t = out_dev.cast<std::tuple<uintptr_t, int64_t, int64_t>>();
          f.dst = reinterpret_cast<double*>(std::get<0>(t));
          f.dst_si = std::get<1>(t);
          f.dst_sj = std::get<2>(t);
        }
        std::vector<double> out;
        if (field && out_dev.is_none()) f.host = &out;
        double sum;
        {
          py::gil_scoped_release nogil;
          sum = device_apply_group(P, pg, opt, f, residual);
        }
        py::object oa = py::none();
        if (f.host) oa = to_array(std::move(out), P.M - 1, P.N - 1);
        return py::make_tuple(sum, oa);
      },
      py::arg("prob"), py::arg("grid"), py::arg("opt"), py::arg("residual") = false, py::arg("v") = py::none(),
      py::arg("v_dev") = py::none(), py::arg("rhs") = py::none(), py::arg("rhs_dev") = py::none(),
      py::arg("out_dev") = py::none(), py::arg("field") = true, py::arg("stream") = 0, py::arg("reaction") = py::none(),
      py::arg("reaction_dev") = py::none());

  // Single-shot device ops for numerics tests: `p` is a full local field
  // (rows × pitch, halo included); returns arrays of the same shape.
  m.def("device_apply_A", [](const Problem& P, const Block& blk, py::array_t<double, py::array::c_style> p) {
    if (p.size() != blk.rows * blk.pitch) throw std::invalid_argument("p must be rows x pitch");
    SolveOptions opt;
    opt.algo = 1;  // classic layout: p is rows × pitch of the block
    DeviceSolver s(P, blk, nullptr, opt);
    const size_t bytes = sizeof(double) * blk.rows * blk.pitch;
    double *dp = nullptr, *dA = nullptr;
    PE_HIP_CHECK(hipMalloc(&dp, bytes));
    PE_HIP_CHECK(hipMalloc(&dA, bytes));
    // everything on the solver's (non-blocking) stream: a null-stream memset
    // is not ordered with it
    PE_HIP_CHECK(hipMemcpyAsync(dp, p.data(), bytes, hipMemcpyHostToDevice, s.stream()));
    PE_HIP_CHECK(hipMemsetAsync(dA, 0, bytes, s.stream()));
    dev::launch_apply_A(s.params(), dp, dA, s.stream());
    std::vector<double> out(blk.rows * blk.pitch);
    PE_HIP_CHECK(hipStreamSynchronize(s.stream()));
    PE_HIP_CHECK(hipMemcpy(out.data(), dA, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipFree(dp));
    PE_HIP_CHECK(hipFree(dA));
    return to_array(std::move(out), blk.rows, blk.pitch);
  });
  m.def("device_coefficients", [](const Problem& P, const Block& blk) {
    SolveOptions opt;
    opt.algo = 1;
    DeviceSolver s(P, blk, nullptr, opt);
    const size_t n = size_t(blk.rows * blk.pitch), bytes = sizeof(double) * n;
    double* d = nullptr;
    PE_HIP_CHECK(hipMalloc(&d, 3 * bytes));
    PE_HIP_CHECK(hipMemsetAsync(d, 0, 3 * bytes, s.stream()));  // ordered with the kernel (non-blocking stream)
    dev::launch_coef(s.params(), d, d + n, d + 2 * n, s.stream());
    PE_HIP_CHECK(hipStreamSynchronize(s.stream()));
    std::vector<double> a(n), b(n), D(n);
    PE_HIP_CHECK(hipMemcpy(a.data(), d, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipMemcpy(b.data(), d + n, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipMemcpy(D.data(), d + 2 * n, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipFree(d));
    return py::make_tuple(to_array(std::move(a), blk.rows, blk.pitch), to_array(std::move(b), blk.rows, blk.pitch),
                          to_array(std::move(D), blk.rows, blk.pitch));
  });
  m.def("device_coefficients_fast", [](const Problem& P, const Block& blk) {
    SolveOptions opt;
    opt.algo = 2;  // single-sweep tables (row classes / chord tables past the halo)
    DeviceSolver s(P, blk, nullptr, opt);
    const int64_t rows = blk.nx + 2, cols = blk.ny + 2;
    const size_t n = size_t(rows * cols), bytes = sizeof(double) * n;
    double* d = nullptr;
    PE_HIP_CHECK(hipMalloc(&d, 3 * bytes));
    dev::launch_coef_fast(s.params(), d, d + n, d + 2 * n, s.stream());
    PE_HIP_CHECK(hipStreamSynchronize(s.stream()));
    std::vector<double> a(n), b(n), di(n);
    PE_HIP_CHECK(hipMemcpy(a.data(), d, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipMemcpy(b.data(), d + n, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipMemcpy(di.data(), d + 2 * n, bytes, hipMemcpyDeviceToHost));
    PE_HIP_CHECK(hipFree(d));
    return py::make_tuple(to_array(std::move(a), rows, cols), to_array(std::move(b), rows, cols),
                          to_array(std::move(di), rows, cols));
  });
}
