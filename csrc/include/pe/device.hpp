// Device (MI355X) runtime: stream-ordered communication + the device-resident
// PCG solver.  Replaces the stage-4 driver gradient_solver_mpi
// (poisson_mpi_cuda2.cu:687-982) and its host-staged halo exchange
// exchange_halos_2d_gpu (:331-500).
#pragma once

#include <hip/hip_runtime_api.h>

#include <memory>
#include <stdexcept>
#include <array>
#include <chrono>
#include <functional>
#include <map>
#include <tuple>
#include <string>
#include <vector>

#include "pe/comm.hpp"
#include "pe/row_classes.hpp"  // host tables, row classes, the item-layout planner
#include "pe/solver.hpp"
#include "pe/solver_plan.hpp"  // the host-only plan of the constructor's decisions

#define PE_HIP_CHECK(expr)                                                                     \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) ::pe::hip_fail(_e, #expr, __FILE__, __LINE__);                       \
  } while (0)

namespace pe {

namespace dev {
struct PeerSum;
}  // namespace dev

[[noreturn]] void hip_fail(hipError_t e, const char* expr, const char* file, int line);
int device_count();
void set_device(int dev);  // hipSetDevice + one pooled solver stream and halo stream for that device
// Solver streams (non-blocking) from / back to the per-device idle pool.
hipStream_t acquire_stream();
void release_stream(hipStream_t s);
// High-priority halo streams (the overlap's), pooled the same way.
hipStream_t acquire_halo_stream();
void release_halo_stream(hipStream_t s);
std::string device_name(int dev);
int current_device();
std::string device_pci_bus_id(int dev);

// Stream-ordered transport over device buffers.
class DeviceComm {
 public:
  virtual ~DeviceComm() = default;
  virtual int rank() const = 0;
  virtual int size() const = 0;
  virtual void allreduce_sum(double* dbuf, int n, hipStream_t s) = 0;
  virtual void allreduce_max(double* dbuf, int n, hipStream_t s) = 0;
  virtual void exchange(const std::vector<Exchange>& ex, hipStream_t s) = 0;
  // Host-side max of a few doubles (timer reduction); may synchronize.
  virtual void host_max(double* hbuf, int n, hipStream_t s) = 0;
  virtual void barrier(hipStream_t s) = 0;
  virtual bool capturable() const { return false; }
  virtual std::string name() const = 0;
  // Failure detection: poll asynchronous transport errors (throws), and
  // abort the communicator so peers blocked in it fail instead of hanging.
  virtual void check_async() {}
  virtual void abort() {}
  // One-shot P2P sum tables (P2P transport only): the single-sweep solver
  // then sums its per-iteration scalars over ranks inside the sweep.
  virtual const dev::PeerSum* peer_sum() const { return nullptr; }
  // Collective (every rank calls it, in the same order): map every rank's
  // `mine` — a fine-grained device buffer of that process — into this one.
  // result[r] = rank r's buffer (result[rank()] = mine); empty on EVERY rank
  // when any rank cannot map (no peer-mapping transport, or a failure).
  virtual std::vector<void*> map_peer_buffers(void* mine) {
    (void)mine;
    return {};
  }
  // Release a mapping made by map_peer_buffers (this process's side only).
  virtual void unmap_peer_buffers(const std::vector<void*>& peers) { (void)peers; }
};

class SelfDeviceComm final : public DeviceComm {
 public:
  int rank() const override { return 0; }
  int size() const override { return 1; }
  void allreduce_sum(double*, int, hipStream_t) override {}
  void allreduce_max(double*, int, hipStream_t) override {}
  void exchange(const std::vector<Exchange>&, hipStream_t) override {}
  void host_max(double*, int, hipStream_t) override {}
  void barrier(hipStream_t) override {}
  bool capturable() const override { return true; }
  std::string name() const override { return "self"; }
};

// RCCL (NCCL API) over xGMI.  The 128-byte unique id is produced by rank 0
// (rccl_unique_id) and distributed by the caller (torch.distributed store,
// or the pe_launch bootstrap file).
std::string rccl_unique_id();
std::unique_ptr<DeviceComm> make_rccl_comm(const std::string& uid, int rank, int size);
// Wrap an existing ncclComm_t (e.g. one owned by another runtime); not owned.
std::unique_ptr<DeviceComm> make_rccl_comm_from_handle(void* nccl_comm);

// Host-staged transport over caller callbacks (e.g. torch.distributed gloo):
// device → host copy, host collective, host → device copy — the reference's
// stage-4 pattern (poisson_mpi_cuda2.cu:331-500).  A test/fallback transport
// for several ranks sharing one GPU (RCCL refuses duplicate devices); the
// production transport is RCCL.
// Timing-only test transport (stream-ordered busy waits; no data moves).
// loopback: the exchange also copies each send buffer into its own receive
// buffer, stream-ordered (an asynchronous transport that moves data).
std::unique_ptr<DeviceComm> make_delay_comm(int size, double exchange_us, double allreduce_us, bool loopback = false);
// One-shot P2P allreduce (IPC-mapped receive buffers, p2p.hip) for the
// per-iteration sums; everything else through `base` (PE_ALLREDUCE=p2p).
std::unique_ptr<DeviceComm> make_p2p_allreduce_comm(std::unique_ptr<DeviceComm> base);
// The last make_p2p_allreduce_comm of this process: "not attempted", "ok" or
// "fallback: <reason>" (its self-tests; bench / CLI diagnostics).
const std::string& p2p_setup_status();
std::unique_ptr<DeviceComm> make_callback_device_comm(int rank, int size, CallbackHostComm::ReduceFn reduce,
                                                      CallbackHostComm::ExchangeFn exch,
                                                      CallbackHostComm::BarrierFn barrier);

namespace dev {
struct DevState;
struct KParams;
struct ResParams;
}  // namespace dev
struct EnvKnobs;  // the parsed PE_* knobs (csrc/hip/env_knobs.hpp)

class DeviceSolver {
 public:
  DeviceSolver(const Problem& prob, const Block& blk, DeviceComm* comm, const SolveOptions& opt);
  ~DeviceSolver();
  DeviceSolver(const DeviceSolver&) = delete;
  DeviceSolver& operator=(const DeviceSolver&) = delete;

  // Full solve: init + iterations until convergence / cap + error.
  SolveResult solve();
  // Benchmark helpers: reset to the initial state, then run exactly `iters`
  // iterations (convergence test off when check_tol == false).
  void reset();
  void run_iterations(int64_t iters, bool use_graph);
  // Capture + instantiate every chunk graph run_iterations(iters, true)
  // will launch, so a timed run_iterations contains no capture.
  void prepare_graphs(int64_t iters);
  // Switch the convergence test on / off (drops cached graphs): the bench
  // times fixed-work steps, then solves to convergence on the same solver.
  void set_check_tol(bool on);
  // Residual rule (Problem::stop): the absolute floor of the next solves'
  // threshold.  The threshold lives in the device state, not in the kernels'
  // parameters: cached graphs stay.  std::invalid_argument under the step-size
  // rule, or for a value that is not finite and >= 0.
  void set_atol(double atol);
  // Initial guess of the next reset() / solve() (bench: the BASELINE
  // random-init solve on the same solver as the zero-init one).
  void set_init(Init init, uint64_t seed, double amp);
  // User fields of the next reset() / solve() (pe/fields.hpp), as this
  // block's slices in host memory: `owned` nx × ny (block_field ring 0) for
  // the right-hand side, `ringed` (nx+2) × (ny+2) (ring 1) for the initial
  // guess, which overrides set_init.  nullptr clears a field (back to F /
  // Init).  Uploaded on the solver stream into planes the solver owns
  // (allocated when first set, kept until cleared); drops cached graphs.  The
  // constructor's tuning always runs on the built-in problem.  A resumed
  // solve needs the same rhs again (B is an input, not checkpointed state)
  // and ignores w0.
  void set_rhs(const double* owned);
  void set_w0(const double* ringed);
  // The same fields from device memory: `g` points at element [0][0] of the
  // GLOBAL interior array (M-1) × (N-1) on this solver's device, float64 or
  // (f32) float32, element strides (si, sj) ≥ 0 (0: an expanded tensor).  This
  // block's share is cut out by kSliceField into the same planes set_rhs /
  // set_w0 fill; nullptr clears the field.  Ordered by events, no host
  // synchronise: the solver stream waits for what `producer` has enqueued so
  // far, and `producer` waits for the slice — the caller may overwrite or free
  // the array in `producer`'s order as soon as the call returns.  Anything but
  // device memory of the solver's device (first and last element) throws
  // std::invalid_argument before any launch and leaves the field as it was.
  void set_rhs_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer);
  void set_w0_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer);
  // User exact solution of the next solve()'s error (pe/fields.hpp): `owned`
  // nx × ny (block_field ring 0) in host memory, or the global array in device
  // memory, exactly like set_rhs / set_rhs_device.  While set, the end-of-solve
  // error is taken against it (kErrorField) instead of the analytic solution,
  // with or without a user rhs; it never enters the iteration.  The plane costs
  // 8 B per owned node while set (allocated when set, freed when cleared) and
  // survives reset() / solve() until replaced or cleared.  Not checkpointed: a
  // resumed solve takes it again, as it takes rhs again.
  void set_exact(const double* owned);
  void set_exact_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer);
  // The reaction field c of A + diag(c) (pe/fields.hpp; a solver constructed
  // with Problem::reaction, else std::invalid_argument): `ringed` (nx+2) ×
  // (ny+2) (block_field ring 1 — kF forms p on the halo ring, so D + c is
  // needed one node beyond the owned block; every rank holds the global array:
  // no halo exchange) in host memory, or the global array in device memory,
  // with set_rhs / set_rhs_device's stream and event ordering and pointer
  // checks.  It is copied into a plane of the p planes' layout
  // (KParams::creact) on the solver stream, takes effect at the next reset() /
  // solve() / operator pass, and may be called again between solves (a Newton
  // loop).  The values are the caller's to check (finite, ≥ 0:
  // check_reaction).  Such a solver refuses reset() until a field is set; a
  // null pointer is refused.  Not checkpointed: a resumed solve needs the same
  // field again, as it needs rhs.
  void set_reaction(const double* ringed);
  void set_reaction_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer);
  bool user_reaction() const { return react_set_; }
  // Host copy of the user plane (0: rhs, nx × ny; 1: w0, (nx+2) × (ny+2);
  // 2: exact, nx × ny); empty when the field is unset.  Synchronizes the
  // stream (tests).
  std::vector<double> user_plane(int which);
  bool user_rhs() const { return rhs_dev_ != nullptr; }
  bool user_w0() const { return w0_dev_ != nullptr; }
  bool user_exact() const { return exact_dev_ != nullptr; }
  // Tuning probe: re-lay out the work items for `ti` rows per item, re-reading
  // the PE_* layout knobs (same allocation, so configurations compare at one
  // memory placement).  Drops cached graphs.
  void relayout(int ti, int order = -1);  // probe: re-lay out the items (ti rows; order 0 / 3, -1 keeps)
  double time_iterations(int64_t iters, bool use_graph);  // device seconds (events)
  // Wait for the stream; with PE_WATCHDOG_S set (or a stall injected) the
  // wait is bounded: no progress for that long aborts the communicator and
  // throws (the bench's timed region and solve are both covered).
  void synchronize();

  // Phases (used by the virtual-rank group driver and tests).
  void enqueue_init();
  void enqueue_F(int par);
  void enqueue_G(int par);
  void enqueue_S(int par);      // single-sweep iteration kernel
  void enqueue_pack(int buf);   // single-sweep: y strips of buffer `buf` → send buffers
  void enqueue_unpack(int buf); // single-sweep: recv buffers → y halo columns of `buf`
  void enqueue_error();
  // Residual rule: g_0 = h1·h2·(z⁰, r⁰) of a state read after the initial
  // reduction, and the write of the threshold (and sqrt(g_0), for the report
  // of a resumed solve) into the device state on the solver stream — two pad
  // slots, DevState::red_G[1] and err[3], so a checkpoint carries them.
  double stop_g0(const dev::DevState& s) const;
  void enqueue_stop_threshold(double thr, double nat0);
  void enqueue_wflush();        // single-sweep: add a deferred α·p term to w (no-op if none)
  double* red_F_dev();
  double* red_G_dev();
  double* fs_dev(int par);
  double* fs2_dev(int par);  // multi-step sweeps' sums (kNS2 / kNS3 of them)
  double* err_dev();
  // Halo exchange as ordered phases; after a phase with `unpack` set the
  // received y strips are scattered into buffer `buf` (single-sweep layout:
  // y phase, unpack, then x phase whose rows carry the corners).  The
  // classic path has one phase (r: x rows + y strips).
  struct HaloPhase {
    std::vector<Exchange> ex;
    bool unpack = false;
  };
  std::vector<HaloPhase> halo_phases(int buf) const;
  std::vector<Exchange> halo_plan() const;  // classic: the single phase
  bool fused() const { return fused_; }
  // two iterations per sweep (fused2.hip)
  bool two_step() const { return sstep_; }     // a multi-iteration sweep (two- or three-step)
  int sweep_steps() const { return steps_; }   // iterations per sweep launch: 1, 2 or 3
  // LDS-resident single sweep (resident.hip): small single-rank blocks run
  // each chunk of iterations as one launch.  PE_RESIDENT=0 disables.
  bool resident() const { return resident_; }
  bool resident_fallback() const { return resident_fallback_; }
  bool overlap() const { return overlap_; }
  // Halo rows pushed by the sweep itself over xGMI (row slabs + in-sweep P2P
  // sums): no exchange call in the iteration, which is then graph-capturable.
  bool halo_push() const { return push_; }
  // Halo exchange by the solver's own peer-put kernel (p2p.hip kPut) instead
  // of the comm's exchange (RCCL grouped send / receive).
  bool halo_put() const { return put_; }
  // The iteration replays from captured hipGraphs (run_iterations(.., true)):
  // no comm call inside it and no two-stream overlap
  bool graphs_usable() const;
  // Multi-rank halo path chosen at construction by timing the candidates on
  // the job's own transport (max over ranks): "exchange", "put" or "push",
  // "+overlap" when the exchange runs on the halo stream under the interior
  // items; halo_candidates() = {path, µs per sweep} as timed ("forced: …" /
  // "none: …" when there was nothing to choose).
  const std::string& halo_path() const { return halo_path_; }
  const std::vector<std::pair<std::string, double>>& halo_candidates() const { return halo_cands_; }
  const std::string& put_status() const { return put_status_; }
  // Probes: switch to another halo path after construction (one of the
  // candidates the construction could pick; the item list is re-laid out for
  // the overlap), and time `sweeps` sweeps of the current path after `warm`
  // ones, from a reset or from the current state (ms per sweep, max over
  // ranks; collective).
  void set_halo_path(const std::string& path, bool overlap);
  double time_halo_path(int sweeps, int warm = 2, bool from_reset = true);
  uintptr_t fields_address() const { return reinterpret_cast<uintptr_t>(fields_); }
  const std::vector<float>& placement_ms() const { return placement_ms_; }
  int placement_choice() const { return placement_best_; }       // index into placement_ms()
  // multi-rank: the slowest rank's chosen ms/sweep (the job runs at its pace;
  // this rank's own choice when alone, 0 without a search)
  double placement_job_ms() const { return placement_job_ms_; }
  double placement_seconds() const { return placement_s_; }      // wall time of the search
  double construct_seconds() const { return ctor_s_; }           // wall time of the constructor
  double exchange_us() const { return exchange_us_; }            // measured halo exchange (multi-rank)
  const std::vector<float>& ti_tuning_ms() const { return ti_ms_; }  // per candidate (8, 10, 14, 18 rows)
  const std::vector<int>& ti_tuning_rows() const { return ti_rows_; }  // the candidates
  // static layout: {most loaded wave, mean wave load, max items on a wave}
  // in row-step cost units (0s for a dynamic layout)
  std::vector<double> layout_load() const { return {lay_.max, lay_.mean, double(lay_.items)}; }
  int layout_cuts() const { return lay_.cuts; }
  // the static layout in use: "lpt", "fill" or "equal" (three-step sweep)
  const std::string& layout_name() const { return lay_.name; }
  // the item list as laid out (host copy of KParams::ilist; empty for walks
  // without a list): {first row | flags, strip | rows << 20} per position
  const std::vector<Entry>& layout_entries() const { return lay_.list; }
  // overlap: list positions 0 .. n-1 hold the boundary items (0: no overlap)
  int layout_boundary() const { return overlap_ ? lay_.lnb[0] : 0; }
  const LayoutRequest& layout_request() const { return lay_req_; }  // what that list was asked with (occupancy, knobs)
  // The plan the constructor followed and what it was made with: plan_solver /
  // finish_plan / plan_chunk of these inputs rebuild it (pe/solver_plan.hpp).
  const SolverPlan& plan() const { return plan_; }
  const SolverKnobs& plan_knobs() const { return plan_knobs_; }
  const DeviceFacts& plan_facts() const { return facts_; }
  const SolveOptions& options() const { return opt_; }
  const HaloInputs& halo_inputs() const { return halo_in_; }  // what choose_halo_path asked halo_candidates() with
  int comm_size() const { return comm_->size(); }
  // First cross-device run diagnostics: hipDeviceCanAccessPeer of this
  // rank's device toward each rank's (1 / 0; -1 the same device; empty on
  // one rank), why the halo push is on / off / fell back, and the transport
  // of the per-sweep sums.
  const std::vector<int>& peer_access() const { return peer_access_; }
  const std::string& push_status() const { return push_status_; }
  const std::string& xr_status() const { return xr_status_; }
  hipStream_t stream() const { return stream_; }

  // Checkpoint / resume of the full device state of this rank (raw fields,
  // halo buffers, scalar block, iteration parity).  Synchronizes the stream.
  // The format holds no problem data: a resumed solve needs the same
  // Problem::shift again (as it needs the same rhs), or it iterates on
  // another operator from this one's state.
  void save_checkpoint(const std::string& path);
  void load_checkpoint(const std::string& path);

  // State / data access.
  void read_state(dev::DevState* out);
  void copy_w(double* host, bool owned_only = true);  // nx × ny row-major
  // The owned w into device memory of this solver's device (kGatherW):
  // dst[(off_i + li) si + (off_j + lj) sj], li < nx, lj < ny — offsets (0, 0)
  // for a dense nx × ny array, (i0-1, j0-1) for the block's position inside a
  // global interior array.  Events only: the solver stream waits for
  // `consumer` (the destination may have work pending from its allocator's
  // stream), `consumer` waits for the gather.  Same pointer check as set_*_device.
  void copy_w_device(double* dst, int64_t si, int64_t sj, int64_t off_i, int64_t off_j, hipStream_t consumer);
  // The gradient of w on the owned nodes and its functionals (pe/fields.hpp
  // gradient_field; kGradField).  Valid after solve().  gradient(): gx / gy
  // receive the owned nx × ny parts in host memory (both null: the
  // functionals only, no field is written).  gradient_device(): gx / gy are
  // float64 device memory of this solver's device, written like copy_w_device
  // writes w — dst[(off_i + li) si + (off_j + lj) sj] — ordered with `consumer`
  // by events only, after the same pointer check, before any launch (both
  // null: the functionals only).  Collective on a multi-rank job (the halo of
  // w is exchanged, the sums are reduced over ranks: every rank gets the
  // job's figures).  Both use the iteration's own planes as scratch, as the
  // end-of-solve residual pass does: afterwards only reset() or solve() may
  // follow, and run_iterations() throws std::logic_error until then.
  GradStats gradient(double* gx_host, double* gy_host);
  GradStats gradient_device(double* gx, double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j,
                            hipStream_t consumer);
  // Its phases, for the virtual-rank group driver: w (flushed) → the plane the
  // layout exchanges (+ its y strips); [the driver exchanges halo_phases(0)];
  // the kernel (classic: its y strips unpacked first) → res_dev()[0..2].
  void enqueue_grad_stage();
  void enqueue_grad(double* gx, double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j);
  double* res_dev();
  // The operator applied to a user field, and the residual field of an iterate
  // (pe/fields.hpp apply_operator / residual_field; kApplyField).  `v` / `w`
  // points at element [0][0] of the GLOBAL interior array (M-1) × (N-1) on
  // this solver's device, float64 or (f32) float32, element strides (si, sj)
  // ≥ 0; on a multi-rank job every rank holds the global array, as for rhs.
  // This block's owned part of A v — or of B − A w, B the rhs set by set_rhs /
  // set_rhs_device (else F) inside the ellipse and 0 outside — is written into
  // float64 device memory as copy_w_device writes w, dst[(off_i + li) dsi +
  // (off_j + lj) dsj] (dst null: the sum only).  Returns the job's
  // h1·h2·Σ v·(A v), or h1·h2·Σ (B − A w)²: collective on a multi-rank job.
  // Events only: the solver stream waits for `caller`, `caller` waits for the
  // kernel.  Source and destination get copy_w_device's pointer check before
  // any launch (std::invalid_argument; nothing is changed).  The pass reads
  // the solver's tables only — no iteration plane, not w: it may run before a
  // solve, after one and after a gradient pass, and the next solve is the
  // same solve.
  double apply_device(const void* v, int64_t si, int64_t sj, bool f32, double* dst, int64_t dsi, int64_t dsj,
                      int64_t off_i, int64_t off_j, hipStream_t caller);
  double residual_device(const void* w, int64_t si, int64_t sj, bool f32, double* dst, int64_t dsi, int64_t dsj,
                         int64_t off_i, int64_t off_j, hipStream_t caller);
  // The same from / to host memory: `v` / `w` the global (M-1)(N-1) array,
  // `out` the owned nx × ny part (null: the sum only); staged through device
  // buffers freed at return.
  double apply(const double* v, double* out);
  double residual(const double* w, double* out);
  // Their phases, for the virtual-rank group driver: the refusal (throws
  // std::invalid_argument unless source and destination are device memory of
  // this solver's device over their whole extent), and the kernel → res_dev()[0].
  void check_apply_span(const void* v, int64_t si, int64_t sj, bool f32, const double* dst, int64_t dsi, int64_t dsj,
                        int64_t off_i, int64_t off_j) const;
  void enqueue_apply(const void* v, int64_t si, int64_t sj, bool f32, bool resid, double* dst, int64_t dsi, int64_t dsj,
                     int64_t off_i, int64_t off_j);
  // gradient_device()'s refusal: throws std::invalid_argument unless both destinations are device memory of this
  // solver's device from element [0][0] to this block's last element
  void check_grad_span(const double* gx, const double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j) const;
  // 0 r, 1 w, 2 p0, 3 p1 (single-sweep: 0 r of x[0], 2 p of x[0], 3 p of
  // x[1], 4 r of x[1]) as field_rows() × field_cols(), local (-h, -h) first.
  void copy_field(int which, double* host);
  int64_t field_rows() const;
  int64_t field_cols() const;
  const Block& block() const { return blk_; }
  const Problem& problem() const { return prob_; }
  int chunk() const { return chunk_; }
  dev::KParams& params();
  // PE_STAMPS=1 diagnostic timeline of the last sweep (see KParams::stamps);
  // empty when off.
  std::vector<unsigned long long> stamps();
  void clear_stamps();  // stream-ordered: the next sweep's stamps only

 private:
  // the constructor's steps (device_solver.cpp)
  void ctor_mark(const char* phase);     // PE_CTOR_TRACE=1: the phase's wall time → stderr
  void peer_diagnostics();               // collective: peer_access_, shared_dev_
  void allocate_fields();
  void allocate_state();
  void fill_kparams(const EnvKnobs& env);
  void allocate_stamps();
  void setup_in_sweep_sums(const EnvKnobs& env);
  void build_tables(int64_t rows_hi, int64_t cols_hi);
  void upload(void* dst, const void* src, size_t bytes);  // set-up data via pinned staging + copy kernel
  void set_plane(double** plane, const double* host, int64_t n);  // set_rhs / set_w0
  // set_rhs_device / set_w0_device (ring 0 / 1)
  void set_plane_device(double** plane, int ring, const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer,
                        const char* what);
  // throws std::invalid_argument unless elements [0] and [last] of `p` are device memory of device_
  void check_device_span(const void* p, int64_t last, size_t elem, const char* what) const;
  void io_events();  // creates ev_io_ on first use
  void set_fused_fields(double* x0, double* x1, double* w);
  // item lists at `ti` rows per item: static layout or dynamic per-XCD shards (+ halo/interior overlap)
  void apply_layout(int ti);
  // the planner's (or the cache's) layout on that halo path; the PE_* layout knobs are read here
  ItemLayout plan_layout(int ti, bool want_overlap, bool push, LayoutRequest* asked);
  void tune_rows_per_item(const std::vector<int>& cands, int ti);  // times the candidates, keeps the fastest
  void create_halo_stream();
  void choose_placement();   // local search, then (multi-rank) the coordinated retry round
  bool placement_search(bool retry);  // local; true when the kept candidate is in the best class
  void measure_exchange();  // sets exchange_us_ (collective)
  void setup_resident();    // tile geometry, band-table size, buffers (single rank, small blocks)
  void enqueue_iteration(int par, int mlimit = 0);  // mlimit > 0: a partial three-step sweep
  void enqueue_fs_reduce(int par);  // cross-rank sum of sweep sums (no-op when the sweep does it)
  // after_sweep: the halo of `buf` was produced by a sweep (with the halo
  // push: import it); false for the initial state (the comm's exchange).
  void enqueue_exchange(int buf, bool after_sweep = true);
  void setup_halo_push();  // collective: maps the push's receive buffers (push_ok_) identically on every rank
  void setup_halo_put();   // collective: maps the put's inboxes + self-test (put_ok_) identically on every rank
  // collective: time the available halo paths (exchange / put / push, with and
  // without the overlap) for a few sweeps each and keep the fastest (max over ranks)
  void choose_halo_path();
  // switch path + re-lay the items; live: the iteration state carries on (halo moved between x and the push buffer)
  // ti > 0: rows per item of the overlap's layout (another height than the tuning's)
  void apply_halo_path(const std::string& path, bool overlap, bool live = false, int ti = 0);
  void prepare_layout(int ti, bool overlap);  // into the cache, host only (item_layout.cpp)
  // one halo phase through the put kernel (put_) or the comm
  void xfer(const std::vector<Exchange>& ex, hipStream_t s);
  void import_halos();     // halo push: x's halo rows <- the receive buffers (enqueued)
  // End-of-solve true residual (single-sweep layouts): w → the p-plane of
  // x[0], the sweep's halo exchange, then kResid into DevState::res
  // (with_r: against the recurrence's r; store: ρ → x[0]'s r-plane) and the
  // cross-rank sum of the four sums.
  void residual_pass(bool with_r, bool store);
  // gradient() / gradient_device(): stage, halo exchange, kernel, cross-rank reductions, state read
  GradStats gradient_pass(double* gx, double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j);
  // apply_device() / residual_device(): check, events, kernel, cross-rank sum, state read
  double operator_pass(const void* v, int64_t si, int64_t sj, bool f32, bool resid, double* dst, int64_t dsi,
                       int64_t dsj, int64_t off_i, int64_t off_j, hipStream_t caller);
  double operator_host(const double* v, double* out, bool resid);  // apply() / residual()
  void wait_event(hipEvent_t ev);  // event wait with transport-error polling + watchdog
  void enqueue_chunk(int iters, int sample_iters = 0);
  // Sampled phase timing (Timers): hipEvent pairs around the phases of the
  // sampled iterations, read once their chunk has completed.
  enum Phase { kPhSweep, kPhDot, kPhHalo, kPhReduce, kPhCopy, kNPhase };
  struct PhaseRec {
    int ph;
    int64_t iter;  // first iteration covered (kPhCopy: the chunk's last), for dropping post-convergence samples
    int64_t n;     // iterations covered (a resident launch covers its whole chunk)
    hipEvent_t a, b;
  };
  struct PhaseSample {
    int ph;
    int64_t iter, n;
    float ms;
  };
  hipEvent_t pooled_event();
  void mark_begin(int ph, hipStream_t s);
  void mark_end(hipStream_t s);
  void harvest(size_t n);  // read the first n records (their events have completed)
  hipGraphExec_t graph_for(int iters);

  Problem prob_;
  Block blk_;
  DeviceComm* comm_;
  std::unique_ptr<DeviceComm> self_;
  SolveOptions opt_;
  SolverPlan plan_;         // what the constructor set up (pe/solver_plan.hpp)
  SolverKnobs plan_knobs_;  // the PE_* values it was planned with
  DeviceFacts facts_;       // the CU count and occupancy it was finished with
  HaloInputs halo_in_;      // the halo-path choice's inputs (multi-rank single-sweep solvers)
  bool ctor_trace_ = false;
  std::chrono::steady_clock::time_point t_mark_;
  hipStream_t stream_ = nullptr;
  bool fused_ = false;
  bool sstep_ = false;    // multi-iteration sweep (fused2.hip / fused3.hip): steps_ iterations per launch
  int steps_ = 1;         // iterations per sweep launch (1, 2, 3)
  SweepGeometry geo_;     // strips, planes, halo depth, table ranges (pe/item_layout.hpp)
  double* fields_ = nullptr;  // classic: r, w, p0, p1 (alloc each); single-sweep: x0, x1, w
  double* xalt_ = nullptr;    // single-sweep: x1 (separate allocation)
  double* walt_ = nullptr;    // single-sweep: w
  std::vector<float> placement_ms_;  // per-candidate sweep time of the placement search
  double* tables_ = nullptr;
  int* rowcls_ = nullptr;
  std::vector<int> rowcls_host_;  // host copy of the row classes (item cost estimates)
  double* halo_ = nullptr;    // send_dn, send_up, recv_dn, recv_up (nx each; ×4 single-sweep)
  int64_t hsize_ = 0;
  double* rhs_dev_ = nullptr;  // user right-hand side, dense nx × ny (null: F)
  // reaction field: the dense ring plane set_plane / set_plane_device fill, and the plane of the p planes' layout
  // the kernels read (KParams::creact = react_dev_ + blk_.base); allocated at construction under Problem::reaction
  double* react_ring_ = nullptr;
  double* react_dev_ = nullptr;
  bool react_set_ = false;
  void place_reaction();
  double* w0_dev_ = nullptr;   // user initial guess, dense (nx+2) × (ny+2) with its ring (null: opt_.init)
  double* exact_dev_ = nullptr;  // user exact solution, dense nx × ny (null: the analytic u)
  int device_ = 0;             // the device the solver was constructed on (device fields must live there)
  hipEvent_t ev_io_[2] = {nullptr, nullptr};  // device fields: caller's stream → solver stream, and back
  double* partial_ = nullptr;
  double* hist_ = nullptr;
  unsigned long long* stamps_ = nullptr;
  size_t nstamps_ = 0;
  // halo/interior overlap (multi-rank single-sweep)
  bool overlap_ = false;
  int2* ilist_ = nullptr;  // per shard: boundary items, heavy items, the rest (dev::KParams::ilist)
  size_t ilist_cap_ = 0;   // entries allocated at ilist_
  int nslot_cap_ = 0;      // item-sum slots allocated
  unsigned long long ov_epoch_ = 0;  // overlapped sweeps since the state was last cleared (sig targets)
  hipStream_t hs_ = nullptr;
  hipEvent_t ev_halo_ = nullptr;
  dev::DevState* st_ = nullptr;
  dev::DevState* hst_ = nullptr;  // pinned, 2 slots
  std::unique_ptr<dev::KParams> kp_;
  std::vector<std::pair<int, hipGraphExec_t>> graphs_;  // instantiated chunk graphs, by length
  int chunk_ = 16;
  int par_ = 0;  // parity of the next iteration (x / p ping-pong)
  bool scratch_used_ = false;  // a gradient pass overwrote an iteration plane: reset() / solve() first
  double watchdog_s_ = 0;   // PE_WATCHDOG_S: abort if a chunk makes no progress this long (0 = off)
  bool fault_stall_ = false;  // PE_FAULT_INJECT=stall: pretend the device never finishes (watchdog test)
  // PE_FAULT_INJECT=drift@iter:K,amp:X — w(M/2, N/2) += X once the host has
  // enqueued iteration K (the residual check's test hook)
  long long fault_drift_ = 0;
  double fault_drift_amp_ = 1e-6;
  // three-step restart threshold on ‖B − A w − r‖_E / ‖r‖_E (PE_RESID_GAP)
  double gap_bound_ = 1e-4;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  hipEvent_t ev_sync_ = nullptr;  // synchronize() under the watchdog
  hipEvent_t t0_ = nullptr, t1_ = nullptr;
  std::vector<hipEvent_t> evpool_;
  std::vector<PhaseRec> recs_;
  std::vector<PhaseSample> samples_;
  bool sampling_ = false;
  int64_t sample_iter_ = 0;  // iteration index of the next enqueued iteration (sampled chunks)
  double ctor_s_ = 0, copy_setup_s_ = 0, placement_s_ = 0;
  bool ctor_counted_ = false;
  int placement_best_ = 0;
  double placement_job_ms_ = 0;
  std::vector<float> ti_ms_;      // their per-sweep times
  std::vector<int> ti_rows_;      // the candidates timed
  std::vector<int> ti_alt_;       // the tuning's best two heights (the overlap is timed at both)
  std::string lay_name_ = "lpt";  // three-step static layout: the construction's choice (PE_LAYOUT overrides)
  std::unique_ptr<LayoutPlanner> planner_;  // host-only (pe/item_layout.hpp); built after the row classes
  ItemLayout lay_;                          // the list the sweeps walk (uploaded at ilist_)
  LayoutRequest lay_req_;                   // what lay_ was asked with
  std::vector<int> peer_access_;
  std::map<std::tuple<int, bool, std::string>, ItemLayout> lay_cache_;  // (rows per item, overlap, layout name)
  bool lay_cache_on_ = false;
  std::function<void()> halo_idle_;        // host work while time_halo_path's sweeps run (the choice's next layouts)
  std::string push_status_ = "off", xr_status_ = "none";
  int cus_ = 256;                  // compute units of the device (a static layout's first cus_ workgroups run first on their CU)
  bool resident_ = false;
  bool resident_fallback_ = false;  // a resident launch aborted (status 5): switched to the streaming sweep
  int stream_chunk_ = 16;           // chunk length of the streaming sweep (after a resident fallback)
  std::unique_ptr<dev::ResParams> rp_;
  int* res_rowstart_ = nullptr;
  double* res_buf_ = nullptr;  // edges then partials
  unsigned* res_ctr_ = nullptr;
  void* stage_ = nullptr;           // pinned staging buffer of upload()
  size_t stage_bytes_ = 0;
  bool push_ = false;               // in-sweep halo push (KParams::push)
  bool push_ok_ = false;            // push set up on every rank: a halo-path candidate
  bool push_loop_ = false;          // PE_PUSH_LOOPBACK diagnostic (own receive buffer)
  bool put_ = false;                // halo phases through kPut (peer put) instead of comm_->exchange
  bool put_ok_ = false;             // put set up and self-tested on every rank: a halo-path candidate
  bool put_loop_ = false;           // PE_PUT_LOOPBACK: this rank is its own peer (one-GPU probes / tests)
  bool want_overlap_ = false;       // the chosen path's overlap (apply_layout)
  bool shared_dev_ = false;         // another rank of the job runs on this rank's GPU (test jobs)
  void* put_buf_ = nullptr;         // fine-grained: [4 dirs][kPutParts] flags, then [4 dirs][2][put_stride_] inbox
  std::vector<void*> put_peers_;    // every rank's put_buf_ mapped here
  unsigned* put_cnt_ = nullptr;     // PutArgs::cnt (device)
  int64_t put_stride_ = 0;          // doubles per inbox parity
  double put_timeout_s_ = 120.0;    // a peer that never arrives poisons the halo after this long (PE_P2P_TIMEOUT_S)
  std::string put_status_ = "off";
  std::string halo_path_ = "none: one rank";
  std::vector<std::pair<std::string, double>> halo_cands_;
  double* hrecv_ = nullptr;         // its fine-grained receive buffer [2][2][2 × pitch]
  std::vector<void*> hpeers_;       // every rank's receive buffer mapped here (comm_->map_peer_buffers)
  double exchange_us_ = 0;  // measured halo exchange (max over ranks), multi-rank only  // the first solve() carries the construction time
};

// P virtual ranks on ONE device (LocalComm).  Every rank runs the
// same kernels and the same halo plan as under RCCL; the transport is
// device-to-device copies + a cross-stream reduction kernel.
// `fields`: user right-hand side / initial guess / exact solution as global interior arrays;
// every block takes its slices through block_field (pe/fields.hpp).
// `dfields`: the same fields, and a destination for w, as global interior
// arrays in device memory (the sibling of UserFields; a field given both ways
// is taken from the device).  Every block's solver slices its part with
// set_*_device and gathers its w into its position of `w_dst` with
// copy_w_device, ordered with `stream` by events.
struct DeviceFields {
  const void* rhs = nullptr;  // element [0][0], strides in elements, float64 or float32
  int64_t rhs_si = 0, rhs_sj = 0;
  bool rhs_f32 = false;
  const void* w0 = nullptr;
  int64_t w0_si = 0, w0_sj = 0;
  bool w0_f32 = false;
  const void* exact = nullptr;
  int64_t exact_si = 0, exact_sj = 0;
  bool exact_f32 = false;
  const void* reaction = nullptr;  // (with Problem::reaction; else UserFields::reaction)
  int64_t reaction_si = 0, reaction_sj = 0;
  bool reaction_f32 = false;
  double* w_dst = nullptr;    // (M-1) × (N-1), strides in elements
  int64_t w_si = 0, w_sj = 0;
  // destinations of the gradient (both or neither), (M-1) × (N-1) each with the same strides
  double* grad_x = nullptr;
  double* grad_y = nullptr;
  int64_t grad_si = 0, grad_sj = 0;
  hipStream_t stream = nullptr;  // the caller's stream (producer of the fields, consumer of w and the gradient)
};
// What the group driver computes of the gradient (DeviceSolver::gradient): nothing, the
// functionals only (SolveResult::grad), or the field as well — into `host`
// (gx then gy, 2 × (M-1)(N-1)) and / or DeviceFields::grad_x / grad_y, every
// block writing its position; the sums go through the group reduction.
struct GroupGradient {
  bool stats = false;
  std::vector<double>* host = nullptr;
};
// device_apply_group: the operand v (or the iterate w) and, for the residual,
// a user right-hand side (neither form: F) as global interior arrays in host or
// device memory (a field given both ways is taken from the device); A v (or
// B − A w) into one global (M-1) × (N-1) destination in device memory, every
// block's solver writing its position, and / or into `host` (row-major).
struct OperatorFields {
  const double* v_host = nullptr;
  const void* v = nullptr;  // element [0][0], strides in elements, float64 or float32
  int64_t v_si = 0, v_sj = 0;
  bool v_f32 = false;
  const double* rhs_host = nullptr;
  const void* rhs = nullptr;
  int64_t rhs_si = 0, rhs_sj = 0;
  bool rhs_f32 = false;
  // the reaction field of A + diag(c) (with Problem::reaction), host or device
  const double* reaction_host = nullptr;
  const void* reaction = nullptr;
  int64_t reaction_si = 0, reaction_sj = 0;
  bool reaction_f32 = false;
  double* dst = nullptr;
  int64_t dst_si = 0, dst_sj = 0;
  std::vector<double>* host = nullptr;
  hipStream_t stream = nullptr;  // the caller's stream (producer of v and rhs, consumer of dst)
};
// P virtual ranks on one device apply the operator (residual: form B − A w):
// every block's kApplyField reads the one global array — the seams between
// blocks get their neighbours' values from it — and the blocks' sums go
// through the group reduction.  Returns h1·h2·Σ.
double device_apply_group(const Problem& prob, const ProcessGrid& pg, const SolveOptions& opt,
                          const OperatorFields& fields, bool residual);
SolveResult device_solve_group(const Problem& prob, int ranks, DecompMode mode, const SolveOptions& opt,
                               std::vector<double>* w_out = nullptr, const UserFields& fields = UserFields());
SolveResult device_solve_group(const Problem& prob, const ProcessGrid& pg, const SolveOptions& opt,
                               std::vector<double>* w_out = nullptr, const UserFields& fields = UserFields(),
                               const DeviceFields& dfields = DeviceFields(),
                               const GroupGradient& grad = GroupGradient());

}  // namespace pe
