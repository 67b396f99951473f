// Device-resident Jacobi-PCG driver (host side).
//
// Reference: gradient_solver_mpi (poisson_mpi_cuda2.cu:687-982).  Where the
// reference assembles a/b/B on the CPU, copies them over, and then drives
// every iteration from the host (6 cudaDeviceSynchronize, 3 × 256 KiB D2H
// partial copies, 3 host MPI_Allreduce, host-staged halos), this driver:
//   * builds two 1-D chord tables (O(M+N) bytes) instead of 3 full arrays,
//   * keeps α, β, the stop test and the iteration count on the device,
//   * enqueues chunks of iterations (captured once into a hipGraph when the
//     transport allows it) and only looks at a pinned copy of the device
//     state once per chunk, with two chunks in flight so the GPU never idles
//     on the host,
//   * talks to peers through a stream-ordered DeviceComm (RCCL over xGMI).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <deque>
#include <limits>
#include <thread>

#include <unistd.h>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "../hip/kernels.hpp"
#include "env_knobs.hpp"
#include "pe/device.hpp"
#include "solver_internal.hpp"

namespace pe {

using dev::DevState;
using dev::KParams;

using detail::clk;
using detail::field_alloc;
using detail::field_free;
using detail::field_try_alloc;
using detail::Range;
using detail::secs;


// Compute units of the current device; unchecked: 256 when the runtime does
// not answer (the plan's resident estimate, before anything is set up).
static int device_cus(bool checked) {
  int cus = 256, dev = 0;
  if (checked) {
    PE_HIP_CHECK(hipGetDevice(&dev));
    PE_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  } else if (hipGetDevice(&dev) == hipSuccess) {
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  }
  return cus;
}

// PE_CTOR_TRACE=1: wall time of each construction phase → stderr
void DeviceSolver::ctor_mark(const char* phase) {
  if (!ctor_trace_) return;
  PE_HIP_CHECK(hipDeviceSynchronize());
  const auto now = clk::now();
  std::fprintf(stderr, "[pe] ctor %-14s %8.3f ms\n", phase, 1e3 * secs(t_mark_, now));
  t_mark_ = now;
}

// The constructor: what to run is the host-only plan's (pe/solver_plan.hpp);
// the steps below set it up on the device, in the order the job's other ranks
// run the same collectives.
DeviceSolver::DeviceSolver(const Problem& prob, const Block& blk, DeviceComm* comm, const SolveOptions& opt)
    : prob_(prob), blk_(blk), comm_(comm), opt_(opt), kp_(std::make_unique<KParams>()) {
  const auto t_ctor = clk::now();
  const EnvKnobs env = read_env_knobs();
  ctor_trace_ = env.ctor_trace >= 1;
  t_mark_ = t_ctor;
  if (!comm_) {
    self_ = std::make_unique<SelfDeviceComm>();
    comm_ = self_.get();
  }
  // 1. plan, stage one: the kernel family, iterations per sweep, rows per
  //    item and item order (refusals throw here, before anything is allocated)
  plan_knobs_ = env.plan;
  plan_ = plan_solver(prob_, blk_, comm_->size(), opt_, env.plan, device_cus(false));
  fused_ = plan_.fused;
  steps_ = plan_.steps;
  sstep_ = plan_.sstep;
  geo_ = plan_.geo;
  lay_name_ = plan_.lay_name;
  ctor_mark("start");
  // 2. stream and peer diagnostics
  stream_ = acquire_stream();  // (pooled: set_device created one — runtime.cpp)
  device_ = current_device();
  ctor_mark("stream");
  if (comm_->size() > 1) peer_diagnostics();
  // 3. allocation
  KParams& k = *kp_;
  std::memset(&k, 0, sizeof(KParams));
  allocate_fields();
  ctor_mark("fields");
  allocate_state();
  // 4. KParams from problem and plan
  fill_kparams(env);
  // 5. occupancy of the sweep the plan selected (k.steps / k.ti / k.order), then plan stage two
  cus_ = device_cus(true);
  k.ncu = cus_;
  facts_.cus = cus_;
  facts_.per_cu = fused_ ? dev::resident_blocks_S(k, 2) : dev::resident_blocks_classic(opt_.variant, prob_.shift != 0.0, prob_.reaction);
  facts_.per_cu0 = fused_ ? dev::resident_blocks_S(k, 0) : 0;
  finish_plan(plan_, blk_, facts_);
  nslot_cap_ = plan_.nslot_cap;
  PE_HIP_CHECK(hipMalloc(&partial_, sizeof(double) * (plan_.npart + 8 * int64_t(nslot_cap_))));
  k.partial = partial_;
  k.itemsum = fused_ ? partial_ + plan_.npart : nullptr;
  ctor_mark("buffers");
  // 6. tables
  build_tables(geo_.rows_hi, geo_.cols_hi);
  const bool has[4] = {blk_.has(LEFT), blk_.has(RIGHT), blk_.has(DOWN), blk_.has(UP)};
  planner_ = std::make_unique<LayoutPlanner>(geo_, blk_.nx, blk_.ny, has, rowcls_host_);
  ctor_mark("tables");
  // 7. halo set-up
  if (env.p2p_timeout_s) put_timeout_s_ = std::max(0.1, *env.p2p_timeout_s);
  setup_halo_push();
  setup_halo_put();
  // 8. layout.  The placement search times the item layout the solve will run
  // (after apply_layout): its best class then reaches the early-stop rate (8192²
  // static layout 0.536-0.545 ms vs 0.564-0.567 for the plain walk), so it
  // stops after 2-3 tries instead of 8 — construction 0.10-0.14 vs 0.15-0.25 s,
  // the same iteration speed (profiles/r2_bench_psearch.txt).
  if (comm_->size() > 1) measure_exchange();  // (diagnostic: the comm's exchange, bench JSON)
  apply_layout(plan_.ti);
  ctor_mark("items");
  // 9. placement
  if (fused_) choose_placement();
  ctor_mark("placement");
  // 10. resident
  setup_resident();
  ctor_mark("resident");
  // 11. tuning
  if (plan_.tune_ti && !resident_) tune_rows_per_item(plan_.ti_cands, plan_.ti);
  if (fused_ && env.stamps) allocate_stamps();
  // 12. in-sweep sums
  setup_in_sweep_sums(env);
  ctor_mark("ti tuning");
  // 13. halo path
  choose_halo_path();
  ctor_mark("halo path");
  // 14. chunk
  const ChunkPlan ch = plan_chunk(plan_, blk_, comm_->size(), opt_.chunk, resident_);
  chunk_ = ch.chunk;
  stream_chunk_ = ch.stream_chunk;
  ctor_mark("tuning+rest");
  // Graph-replayed solves (--graph): one small pageable copy at construction.
  // The runtime sets up its pageable-copy path lazily at the first such copy
  // of the process (≈19 ms, profiles/r2_init_probe.txt) — which a graph
  // instantiation triggers; this keeps that cost out of the iteration loop (4
  // µs per iteration at 1600×2400 otherwise).  The eager solve never takes
  // that path.
  if (opt_.use_graph) {
    double h = 0.0;
    PE_HIP_CHECK(hipMemcpy(partial_, &h, sizeof(double), hipMemcpyHostToDevice));
  }
  PE_HIP_CHECK(hipDeviceSynchronize());
  ctor_s_ = secs(t_ctor, clk::now());
}

// Peer access of this rank's device toward every rank's (first cross-device
// run diagnostics: the halo push and the in-sweep sums map peers' memory):
// 1 / 0 hipDeviceCanAccessPeer, -1 the same physical device, -2 a device this
// process cannot see (another node, or masked by HIP_VISIBLE_DEVICES).
// Devices are compared by PCI location, not by process-local ordinals, and
// gathered 64 ranks per collective (the comms' host scratch size); a failure
// leaves the diagnostics empty and never aborts construction.
void DeviceSolver::peer_diagnostics() {
  // key = (host hash << 32) | PCI domain / bus / device: exact in a double
  // (52 bits), so GPUs of different nodes never compare equal.  Every rank
  // runs every collective round whatever failed locally (a failure only
  // turns its own contribution into -1).
  const int P = comm_->size();
  auto host_hash = []() -> int64_t {
    char name[256] = {0};
    if (gethostname(name, sizeof(name) - 1) != 0) return 0;
    uint64_t h = 1469598103934665603ull;  // FNV-1a
    for (const char* c = name; *c; ++c) h = (h ^ uint64_t(uint8_t(*c))) * 1099511628211ull;
    return int64_t((h ^ (h >> 20) ^ (h >> 40)) & 0xFFFFF);
  };
  const int64_t hh = host_hash();
  auto pci_key = [hh](int dv) -> double {
    int dom = 0, bus = -1, dev = 0;
    if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, dv) != hipSuccess ||
        hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, dv) != hipSuccess ||
        hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, dv) != hipSuccess) {
      (void)hipGetLastError();
      return -1.0;
    }
    return double((hh << 32) | (int64_t(dom & 0xFFFF) << 16) | (int64_t(bus & 0xFF) << 8) | int64_t(dev & 0xFF));
  };
  int mydev = -1, ndev = 0;
  if (hipGetDevice(&mydev) != hipSuccess || hipGetDeviceCount(&ndev) != hipSuccess) {
    (void)hipGetLastError();
    mydev = -1;
    ndev = 0;
  }
  const double mykey = mydev >= 0 ? pci_key(mydev) : -1.0;
  std::vector<double> keys(size_t(P), -1.0);
  for (int c0 = 0; c0 < P; c0 += 64) {
    const int n = std::min(64, P - c0);
    double chunk[64];
    for (int i = 0; i < n; ++i) chunk[i] = c0 + i == comm_->rank() ? mykey : -1.0;
    comm_->host_max(chunk, n, stream_);
    for (int i = 0; i < n; ++i) keys[size_t(c0 + i)] = chunk[i];
  }
  for (int r = 0; r < P; ++r)
    if (r != comm_->rank() && mykey >= 0 && keys[size_t(r)] == mykey) shared_dev_ = true;
  std::vector<int> pa(size_t(P), -1);
  for (int r = 0; r < P && mykey >= 0; ++r) {
    const double key = keys[size_t(r)];
    if (key < 0 || key == mykey) continue;
    int d = -1;
    for (int i = 0; i < ndev && d < 0; ++i)
      if (pci_key(i) == key) d = i;
    if (d < 0) {
      pa[size_t(r)] = -2;
      continue;
    }
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, mydev, d) != hipSuccess) {
      (void)hipGetLastError();
      can = 0;
    }
    pa[size_t(r)] = can;
  }
  peer_access_ = std::move(pa);
}

// The iteration's planes: single-sweep x0, x1 (r and p interleaved by row)
// and w; classic r, w, p0, p1 in one allocation.
void DeviceSolver::allocate_fields() {
  KParams& k = *kp_;
  const int64_t nx = blk_.nx;
  if (fused_) {
    k.pitch = 2 * geo_.plane;
    k.wpitch = geo_.plane;
    k.poff = geo_.plane;
    fields_ = static_cast<double*>(field_alloc(sizeof(double) * geo_.xsize));
    xalt_ = static_cast<double*>(field_alloc(sizeof(double) * geo_.xsize));
    walt_ = static_cast<double*>(field_alloc(sizeof(double) * geo_.wsize));
    ctor_mark("field allocs");
    set_fused_fields(fields_, xalt_, walt_);
    hsize_ = std::max<int64_t>(1, nx) * 2 * geo_.hdep;  // y strips: hdep columns of r and p per owned row
  } else {
    const int64_t A = blk_.alloc;
    PE_HIP_CHECK(hipMalloc(&fields_, sizeof(double) * A * 4));
    k.pitch = blk_.pitch;
    k.wpitch = blk_.pitch;
    k.r = fields_ + blk_.base;
    k.w = fields_ + A + blk_.base;
    k.p[0] = fields_ + 2 * A + blk_.base;
    k.p[1] = fields_ + 3 * A + blk_.base;
    hsize_ = std::max<int64_t>(1, nx);
    if (prob_.reaction) {  // the reaction plane: a p plane's allocation, zero until set_reaction* fills block and ring
      PE_HIP_CHECK(hipMalloc(&react_dev_, sizeof(double) * A));
      PE_HIP_CHECK(hipMemsetAsync(react_dev_, 0, sizeof(double) * A, stream_));
    }
  }
}

// Tables, halo buffers, the device state and its pinned copy, events, the history.
void DeviceSolver::allocate_state() {
  const int64_t nrow_tab = geo_.rows_hi - geo_.tab_lo + 1, ncol_tab = geo_.cols_hi - geo_.tab_lo + 1;
  const int64_t ntab = nrow_tab * 4 + ncol_tab * 4;
  PE_HIP_CHECK(hipMalloc(&tables_, sizeof(double) * ntab));
  PE_HIP_CHECK(hipMalloc(&rowcls_, sizeof(int) * nrow_tab * 4));
  PE_HIP_CHECK(hipMalloc(&halo_, sizeof(double) * hsize_ * 4));
  PE_HIP_CHECK(hipMalloc(&st_, sizeof(DevState)));
  // (every reset zeroes the state again; an operator pass may run before the first one and needs ticket[3] == 0)
  PE_HIP_CHECK(hipMemsetAsync(st_, 0, sizeof(DevState), stream_));
  PE_HIP_CHECK(hipHostMalloc(&hst_, sizeof(DevState) * 2, hipHostMallocDefault));
  std::memset(hst_, 0, sizeof(DevState) * 2);
  PE_HIP_CHECK(hipEventCreateWithFlags(&ev_[0], hipEventDisableTiming));
  PE_HIP_CHECK(hipEventCreateWithFlags(&ev_[1], hipEventDisableTiming));
  PE_HIP_CHECK(hipEventCreateWithFlags(&ev_sync_, hipEventDisableTiming));
  PE_HIP_CHECK(hipEventCreate(&t0_));
  PE_HIP_CHECK(hipEventCreate(&t1_));
  if (opt_.keep_history) {  // per-iteration ‖Δw‖ on the device (capped at 2²⁴ iterations)
    kp_->hist_n = std::min<long long>(prob_.iter_cap(), 1LL << 24);
    PE_HIP_CHECK(hipMalloc(&hist_, sizeof(double) * size_t(std::max<long long>(1, kp_->hist_n))));
    kp_->hist = hist_;
  }
}

// The kernels' parameter block from the problem, the block, the plan and the
// buffers allocated so far (the item list and the sums' buffers follow).
void DeviceSolver::fill_kparams(const EnvKnobs& env) {
  KParams& k = *kp_;
  const int64_t nrow_tab = geo_.rows_hi - geo_.tab_lo + 1;
  k.fused = fused_ ? 1 : 0;
  k.steps = steps_;
  k.hdep = geo_.hdep;
  k.pre_load = 1;  // first item's list entry + row classes loaded at kernel entry (fused3.hip Pre3)
  k.dring = 1;     // band rows read 1/D from the LDS ring (+0.7 % at 8192², profiles/r5_ab_kernel.txt)
  // SIMD priority turns (fused3.hip prio_turn), opt-in: 1-GPU 2048² and
  // 1600×2400 T_iterate −0.8-1.5 % at PE_PRIO=10, but the 2-rank blocks of
  // 2048² / 1600×2400 +2-7 % (20.2 vs 18.9 µs per iteration), 8192² −4-6 %
  // it/s, the 8-rank slab and 4×2 blocks neutral — profiles/r5_prio.txt
  k.prio = env.prio;
  k.stage = env.stage;
  k.xorg = geo_.xorg;
  k.nx = blk_.nx;
  k.ny = blk_.ny;
  k.M = prob_.M;
  k.N = prob_.N;
  k.gi0 = blk_.i0 - 1;
  k.gj0 = blk_.j0 - 1;
  k.A1 = prob_.A1;
  k.A2 = prob_.A2;
  k.h1 = prob_.h1();
  k.h2 = prob_.h2();
  k.eps = prob_.eps();
  k.inv_eps = 1.0 / k.eps;
  k.h1sq = k.h1 * k.h1;
  k.h2sq = k.h2 * k.h2;
  k.nih1 = -1.0 / k.h1;
  k.nih2 = -1.0 / k.h2;
  k.cx = prob_.cx;
  k.cy = prob_.cy;
  k.F = prob_.F;
  k.u_scale = prob_.u_scale();
  k.tol = prob_.tol;
  k.weighted = prob_.norm == Norm::Weighted ? 1 : 0;
  k.max_iter = prob_.iter_cap();
  for (int d = 0; d < 4; ++d) k.has[d] = blk_.has(d) ? 1 : 0;
  // tables start at local index geo_.tab_lo; the kernels index them by (local + 1)
  k.colT = tables_ - (geo_.tab_lo + 1) * 4;
  k.rowcls = rowcls_ - (geo_.tab_lo + 1) * 4;
  k.rowT = tables_ + nrow_tab * 4 - (geo_.tab_lo + 1) * 4;
  k.send_dn = halo_;
  k.send_up = halo_ + hsize_;
  k.recv_dn = halo_ + 2 * hsize_;
  k.recv_up = halo_ + 3 * hsize_;
  k.st = st_;
  k.check_tol = opt_.check_tol ? 1 : 0;
  // Failure-detection hooks: PE_FAULT_INJECT=nan@iter:K poisons
  // the reduced sums after iteration K (the solver must stop with a
  // non-finite status), PE_FAULT_INJECT=stall (or stall@rank:R, one rank
  // only) makes the host believe the device never finishes (the watchdog
  // must fire); PE_WATCHDOG_S sets the
  // no-progress limit of the host loop.
  const FaultInject& fi = env.fault;
  k.fault_iter = fi.nan_iter;
  k.fault_zero = fi.zero_iter;
  fault_stall_ = fi.stall || fi.stall_rank == blk_.rank;
  if (fi.slow_rank == blk_.rank) k.slow_ticks = fi.slow_ticks;
  if (fi.drift) {
    fault_drift_ = fi.drift_iter;
    if (fi.drift_amp) fault_drift_amp_ = *fi.drift_amp;
  }
  if (env.resid_gap) gap_bound_ = *env.resid_gap;
  if (env.watchdog_s) watchdog_s_ = *env.watchdog_s;
  // Work decomposition: wave strips (128 columns classic, 124 output
  // columns single-sweep) × `ti`-row chunks, dealt round-robin (chunk-major)
  // to a persistent grid of ~16 waves per CU, so the waves running at any
  // moment cover a compact window of rows (measured: long per-wave row
  // ranges spread over the whole array run 25 % slower than 8-16-row items
  // despite their halo-row re-reads, which then hit L2/MALL).
  // Persistent grid: exactly the resident waves (a second partial round of
  // blocks would run after the first finishes — a tail of up to one item
  // per wave).
  k.order = plan_.order;
  k.ti = plan_.ti_query;
  k.nstrips = int(geo_.strips);
  k.ih1sq = 1.0 / k.h1sq;
  k.ih2sq = 1.0 / k.h2sq;
  k.D_in = (1.0 + 1.0) / k.h1sq + (1.0 + 1.0) / k.h2sq;
  k.D_out = (k.inv_eps + k.inv_eps) / k.h1sq + (k.inv_eps + k.inv_eps) / k.h2sq;
  k.dinv_in = 1.0 / ((1.0 + 1.0) * k.ih1sq + (1.0 + 1.0) * k.ih2sq);
  k.dinv_out = 1.0 / ((k.inv_eps + k.inv_eps) * k.ih1sq + (k.inv_eps + k.inv_eps) * k.ih2sq);
  k.stop_res = prob_.stop == Stop::Residual ? 1 : 0;
  // (a reaction field: the FIELD instantiations; the four diagonal constants stay unshifted, the kernels add c per node)
  k.creact = react_dev_ ? react_dev_ + blk_.base : nullptr;
  k.shift = prob_.shift;
  if (k.shift != 0.0) {  // the diagonal of A + σI in the two uniform classes (pe/fields.hpp; the band adds σ in cset)
    k.D_in = shifted_diag(k.D_in, k.shift);
    k.D_out = shifted_diag(k.D_out, k.shift);
    k.dinv_in = 1.0 / shifted_diag((1.0 + 1.0) * k.ih1sq + (1.0 + 1.0) * k.ih2sq, k.shift);
    k.dinv_out = 1.0 / shifted_diag((k.inv_eps + k.inv_eps) * k.ih1sq + (k.inv_eps + k.inv_eps) * k.ih2sq, k.shift);
  }
}

// PE_STAMPS=1: the sweeps' diagnostic timeline (KParams::stamps)
void DeviceSolver::allocate_stamps() {
  KParams& k = *kp_;
  const size_t nw = size_t(dev::kWPB) * size_t(std::max(k.nblocks, k.nblocks0));
  nstamps_ = 4 * size_t(nslot_cap_) + 2 * nw + 32 * nw + 8;  // (+8 whole-grid stamps: three-step sweep)
  PE_HIP_CHECK(hipMalloc(&stamps_, sizeof(unsigned long long) * nstamps_));
  PE_HIP_CHECK(hipMemsetAsync(stamps_, 0, sizeof(unsigned long long) * nstamps_, stream_));
  k.stamps = stamps_;
  k.stamps2 = stamps_ + nstamps_ - 32 * nw;  // the last 32 × waves entries (the 8 grid stamps before them)
}

// In-sweep cross-rank reduction (after the placement search, whose sweeps
// are local and differ in number between ranks).  PE_XR=0 keeps the
// separate allreduce launch.
void DeviceSolver::setup_in_sweep_sums(const EnvKnobs& env) {
  KParams& k = *kp_;
  xr_status_ = comm_->size() < 2 ? "none: one rank" : "allreduce launch (" + comm_->name() + ")";
  if (fused_ && comm_->size() > 1 && comm_->peer_sum() && env.xr) {
    k.xr = *comm_->peer_sum();
    k.xr.wait_acc = &st_->xr_wait;  // T_MPI of the in-sweep sum (DevState::xr_wait, xr_n)
    xr_status_ = "in-sweep P2P over xGMI";
  }
  if (fused_ && comm_->size() > 1 && !comm_->peer_sum()) xr_status_ += "; P2P set-up " + p2p_setup_status();
  // The push's pointers (its kernel variant runs when choose_halo_path picks
  // it: the push is delivered by the in-sweep sum's flags, so the local
  // sweeps above ran without either).
  if (push_ok_) {
    const int64_t side = int64_t(geo_.hdep) * k.pitch;
    double* lo = static_cast<double*>(hpeers_[size_t(blk_.nbr[LEFT] >= 0 ? blk_.nbr[LEFT] : blk_.rank)]);
    double* hi = static_cast<double*>(hpeers_[size_t(blk_.nbr[RIGHT] >= 0 ? blk_.nbr[RIGHT] : blk_.rank)]);
    for (int b = 0; b < 2; ++b) {
      // my rows 1, 2 → the LEFT neighbour's side 1 (its rows nx'+1, nx'+2);
      // my rows nx-1, nx → the RIGHT neighbour's side 0 (its rows -1, 0)
      k.hpush_lo[b] = blk_.has(LEFT) ? lo + (2 * b + 1) * side : nullptr;
      k.hpush_hi[b] = blk_.has(RIGHT) ? hi + (2 * b + 0) * side : nullptr;
    }
    k.hrecv = hrecv_;
  }
  k.push = 0;
}

void DeviceSolver::relayout(int ti, int order) {
  if (!fused_ || resident_) return;
  ti = std::max(2, std::min(ti, steps_ >= 3 ? dev::kTImax3 : 64));
  const int ord = (order == 0 || order == 3) ? order : kp_->order;  // static LPT list / dynamic per-XCD queue
  // the item-sum slots of the dynamic order were sized at
  // construction: a layout that needs more is refused before anything
  // changes (the static layout sums per block, not per item: any height)
  const int64_t nitems = int64_t(kp_->nstrips) * ((blk_.nx + ti - 1) / ti);
  const int64_t need = ord == 0 ? 0 : 2 * nitems + 64;
  if (need > nslot_cap_)
    throw std::invalid_argument("relayout: " + std::to_string(ti) + " rows per item (order " + std::to_string(ord) +
                                ") needs " + std::to_string(need) + " item-sum slots, " + std::to_string(nslot_cap_) +
                                " allocated");
  kp_->order = ord;
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
  for (auto& g : graphs_) PE_HIP_CHECK(hipGraphExecDestroy(g.second));
  graphs_.clear();
  apply_layout(ti);
}

void DeviceSolver::set_check_tol(bool on) {
  opt_.check_tol = on;
  kp_->check_tol = on ? 1 : 0;
  for (auto& g : graphs_) PE_HIP_CHECK(hipGraphExecDestroy(g.second));  // captured with the old parameters
  graphs_.clear();
}

void DeviceSolver::set_atol(double atol) {
  Problem p = prob_;
  p.atol = atol;
  check_stop(p, "DeviceSolver");
  prob_.atol = atol;  // (host only: the next solve's threshold; no kernel parameter, cached graphs stay)
}

double DeviceSolver::stop_g0(const DevState& s) const {
  // the expressions the kernels test with: kF's (red_G · h1) · h2, sweep_scalars' fs · (h1 · h2)
  return fused_ ? s.fs[1][0] * (prob_.h1() * prob_.h2()) : (s.red_G[0] * prob_.h1()) * prob_.h2();
}

void DeviceSolver::enqueue_stop_threshold(double thr, double nat0) {
  dev::launch_set_stop(*kp_, thr, nat0, stream_);
  PE_HIP_CHECK(hipGetLastError());
}

void DeviceSolver::set_init(Init init, uint64_t seed, double amp) {
  opt_.init = init;
  opt_.seed = seed;
  opt_.init_amp = amp;
}

void DeviceSolver::set_plane(double** plane, const double* host, int64_t n) {
  for (auto& g : graphs_) PE_HIP_CHECK(hipGraphExecDestroy(g.second));
  graphs_.clear();
  if (!host) {
    if (*plane) {
      PE_HIP_CHECK(hipStreamSynchronize(stream_));  // (a kernel of the last solve may still read it)
      PE_HIP_CHECK(hipFree(*plane));
      *plane = nullptr;
    }
    return;
  }
  if (!*plane) PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(plane), sizeof(double) * size_t(n)));
  upload(*plane, host, sizeof(double) * size_t(n));
}

void DeviceSolver::set_rhs(const double* owned) { set_plane(&rhs_dev_, owned, blk_.nx * blk_.ny); }

void DeviceSolver::set_w0(const double* ringed) { set_plane(&w0_dev_, ringed, (blk_.nx + 2) * (blk_.ny + 2)); }

void DeviceSolver::set_exact(const double* owned) { set_plane(&exact_dev_, owned, blk_.nx * blk_.ny); }

// The dense ring plane → the plane the kernels read, in stream order behind the
// upload / slice and behind every kernel of an earlier solve.
void DeviceSolver::place_reaction() {
  dev::launch_ring_to_pitched(react_ring_, blk_.nx, blk_.ny, react_dev_ + blk_.base, blk_.pitch, stream_);
  PE_HIP_CHECK(hipGetLastError());
  react_set_ = true;
}

void DeviceSolver::set_reaction(const double* ringed) {
  if (!prob_.reaction)
    throw std::invalid_argument("reaction: this solver was constructed without Problem::reaction (the layout is fixed at construction)");
  if (!ringed) throw std::invalid_argument("reaction: null field on a solver constructed with Problem::reaction");
  set_plane(&react_ring_, ringed, (blk_.nx + 2) * (blk_.ny + 2));
  place_reaction();
}

void DeviceSolver::set_reaction_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer) {
  if (!prob_.reaction)
    throw std::invalid_argument("reaction: this solver was constructed without Problem::reaction (the layout is fixed at construction)");
  if (!g) throw std::invalid_argument("reaction: null field on a solver constructed with Problem::reaction");
  set_plane_device(&react_ring_, 1, g, si, sj, f32, producer, "reaction");
  place_reaction();
}

// Device memory of this solver's device at elements [0] and [last] of `p`
// (hipPointerGetAttributes), and — where the runtime knows the allocation's
// range — both inside one allocation.  Throws before anything is launched.
void DeviceSolver::check_device_span(const void* p, int64_t last, size_t elem, const char* what) const {
  const std::string name(what);
  if (last < 0) throw std::invalid_argument(name + ": negative extent");
  const char* first = static_cast<const char*>(p);
  const char* end = first + size_t(last) * elem;  // the last element
  for (const char* q : {first, end}) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, q);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // (an unregistered host pointer: not a sticky error)
      throw std::invalid_argument(name + ": not a device pointer (" + hipGetErrorString(e) + ")");
    }
    if (at.type != hipMemoryTypeDevice)
      throw std::invalid_argument(name + ": not device memory (host, managed or unregistered pointer)");
    if (at.device != device_)
      throw std::invalid_argument(name + ": memory of device " + std::to_string(at.device) + ", the solver runs on device " +
                                  std::to_string(device_));
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<char*>(first)) == hipSuccess) {
    if (end + elem > static_cast<const char*>(base) + size)
      throw std::invalid_argument(name + ": shape and strides reach past the end of the allocation");
  } else {
    (void)hipGetLastError();
  }
}

void DeviceSolver::io_events() {
  for (hipEvent_t& e : ev_io_)
    if (!e) PE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

void DeviceSolver::set_plane_device(double** plane, int ring, const void* g, int64_t si, int64_t sj, bool f32,
                                    hipStream_t producer, const char* what) {
  if (!g) {
    set_plane(plane, nullptr, 0);
    return;
  }
  const int64_t gnx = int64_t(prob_.M) - 1, gny = int64_t(prob_.N) - 1;
  if (si < 0 || sj < 0) throw std::invalid_argument(std::string(what) + ": negative stride");
  check_device_span(g, (gnx - 1) * si + (gny - 1) * sj, f32 ? sizeof(float) : sizeof(double), what);
  for (auto& gr : graphs_) PE_HIP_CHECK(hipGraphExecDestroy(gr.second));
  graphs_.clear();
  io_events();
  const int64_t rows = blk_.nx + 2 * ring, cols = blk_.ny + 2 * ring;
  if (!*plane) PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(plane), sizeof(double) * size_t(rows * cols)));
  PE_HIP_CHECK(hipEventRecord(ev_io_[0], producer));
  PE_HIP_CHECK(hipStreamWaitEvent(stream_, ev_io_[0], 0));
  dev::launch_slice_field(g, f32, si, sj, gnx, gny, blk_.i0, blk_.j0, blk_.nx, blk_.ny, ring, *plane, stream_);
  PE_HIP_CHECK(hipGetLastError());
  PE_HIP_CHECK(hipEventRecord(ev_io_[1], stream_));
  PE_HIP_CHECK(hipStreamWaitEvent(producer, ev_io_[1], 0));
}

void DeviceSolver::set_rhs_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer) {
  set_plane_device(&rhs_dev_, 0, g, si, sj, f32, producer, "rhs");
}

void DeviceSolver::set_w0_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer) {
  set_plane_device(&w0_dev_, 1, g, si, sj, f32, producer, "w0");
}

void DeviceSolver::set_exact_device(const void* g, int64_t si, int64_t sj, bool f32, hipStream_t producer) {
  set_plane_device(&exact_dev_, 0, g, si, sj, f32, producer, "exact");
}

std::vector<double> DeviceSolver::user_plane(int which) {
  if (which < 0 || which > 2) throw std::invalid_argument("user_plane: 0 (rhs), 1 (w0) or 2 (exact)");
  const double* plane = which == 1 ? w0_dev_ : which == 2 ? exact_dev_ : rhs_dev_;
  if (!plane) return {};
  const int64_t ring = which == 1;
  std::vector<double> v(size_t((blk_.nx + 2 * ring) * (blk_.ny + 2 * ring)));
  PE_HIP_CHECK(hipMemcpyAsync(v.data(), plane, sizeof(double) * v.size(), hipMemcpyDeviceToHost, stream_));
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
  return v;
}

void DeviceSolver::set_fused_fields(double* x0, double* x1, double* w) {
  KParams& k = *kp_;
  fields_ = x0;
  xalt_ = x1;
  walt_ = w;
  // local (0, 0): row -(hdep-1), column -xorg at element 0
  const int64_t h = geo_.hdep - 1, hc = geo_.xorg;
  k.x[0] = x0 + h * k.pitch + hc;
  k.x[1] = x1 + h * k.pitch + hc;
  k.w = w + h * geo_.plane + hc;
  k.r = k.x[0];
  k.p[0] = k.x[0] + geo_.plane;
  k.p[1] = k.x[1] + geo_.plane;
}

// Median time of this rank's halo exchange (every rank runs the same
// number of collective exchanges here), then the max over ranks.
void DeviceSolver::measure_exchange() {
  Range range("pe.measure_exchange");
  std::vector<float> t;
  for (int i = 0; i < 9; ++i) {
    PE_HIP_CHECK(hipEventRecord(t0_, stream_));
    if (fused_) enqueue_exchange(0);
    else comm_->exchange(halo_plan(), stream_);
    PE_HIP_CHECK(hipEventRecord(t1_, stream_));
    PE_HIP_CHECK(hipEventSynchronize(t1_));
    float ms = 0.f;
    PE_HIP_CHECK(hipEventElapsedTime(&ms, t0_, t1_));
    if (i >= 2) t.push_back(ms);  // two warm-up exchanges (connection set-up)
  }
  std::sort(t.begin(), t.end());
  double us[1] = {1e3 * double(t[t.size() / 2])};
  comm_->host_max(us, 1, stream_);
  exchange_us_ = us[0];
}


void DeviceSolver::create_halo_stream() {
  if (hs_) return;
  hs_ = acquire_halo_stream();  // (pooled: set_device created one next to the solver stream — runtime.cpp)
  PE_HIP_CHECK(hipEventCreateWithFlags(&ev_halo_, hipEventDisableTiming));
}


DeviceSolver::~DeviceSolver() {
  for (auto& g : graphs_) (void)hipGraphExecDestroy(g.second);
  (void)hipEventDestroy(ev_[0]);
  (void)hipEventDestroy(ev_[1]);
  (void)hipEventDestroy(ev_sync_);
  for (hipEvent_t e : ev_io_)
    if (e) (void)hipEventDestroy(e);
  (void)hipEventDestroy(t0_);
  (void)hipEventDestroy(t1_);
  for (const PhaseRec& r : recs_) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (hipEvent_t e : evpool_) (void)hipEventDestroy(e);
  if (fused_) field_free(fields_);
  else (void)hipFree(fields_);
  field_free(xalt_);
  field_free(walt_);
  (void)hipFree(tables_);
  (void)hipFree(rowcls_);
  (void)hipFree(halo_);
  if (!hpeers_.empty() && !push_loop_) comm_->unmap_peer_buffers(hpeers_);
  if (hrecv_) (void)hipFree(hrecv_);
  if (!put_peers_.empty() && !put_loop_) comm_->unmap_peer_buffers(put_peers_);
  if (put_buf_) (void)hipFree(put_buf_);
  if (put_cnt_) (void)hipFree(put_cnt_);
  if (stage_) (void)hipHostFree(stage_);
  if (rhs_dev_) (void)hipFree(rhs_dev_);
  if (react_ring_) (void)hipFree(react_ring_);
  if (react_dev_) (void)hipFree(react_dev_);
  if (w0_dev_) (void)hipFree(w0_dev_);
  if (exact_dev_) (void)hipFree(exact_dev_);
  (void)hipFree(partial_);
  if (hist_) (void)hipFree(hist_);
  if (stamps_) (void)hipFree(stamps_);
  if (ilist_) (void)hipFree(ilist_);
  if (res_rowstart_) (void)hipFree(res_rowstart_);
  if (res_buf_) (void)hipFree(res_buf_);
  if (res_ctr_) (void)hipFree(res_ctr_);
  if (hs_) {
    (void)hipStreamSynchronize(hs_);
    release_halo_stream(hs_);
  }
  if (ev_halo_) (void)hipEventDestroy(ev_halo_);
  (void)hipFree(st_);
  (void)hipHostFree(hst_);
  (void)hipStreamSynchronize(stream_);
  release_stream(stream_);
}

KParams& DeviceSolver::params() { return *kp_; }

void DeviceSolver::clear_stamps() {
  if (nstamps_) PE_HIP_CHECK(hipMemsetAsync(stamps_, 0, sizeof(unsigned long long) * nstamps_, stream_));
}

std::vector<unsigned long long> DeviceSolver::stamps() {
  std::vector<unsigned long long> v(nstamps_);
  if (nstamps_) {
    PE_HIP_CHECK(hipStreamSynchronize(stream_));
    PE_HIP_CHECK(hipMemcpy(v.data(), stamps_, sizeof(unsigned long long) * nstamps_, hipMemcpyDeviceToHost));
  }
  return v;
}

// Host → device set-up data through a pinned staging buffer and a copy
// kernel (launch_copy_words: no hipMemcpy in T_solver); synchronous.
void DeviceSolver::upload(void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return;
  if (bytes % 4) throw std::logic_error("upload: size must be a multiple of 4 bytes");
  if (bytes > stage_bytes_) {
    if (stage_) PE_HIP_CHECK(hipHostFree(stage_));
    stage_bytes_ = std::max(bytes, size_t(1) << 20);
    PE_HIP_CHECK(hipHostMalloc(&stage_, stage_bytes_, hipHostMallocDefault));
  }
  std::memcpy(stage_, src, bytes);
  dev::launch_copy_words(dst, stage_, bytes, false, stream_);
  PE_HIP_CHECK(hipGetLastError());
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSolver::build_tables(int64_t rows_hi, int64_t cols_hi) {
  const std::vector<double> t = chord_tables(prob_, blk_, rows_hi, cols_hi, geo_.tab_lo);
  const auto t0 = clk::now();
  upload(tables_, t.data(), sizeof(double) * t.size());
  copy_setup_s_ += secs(t0, clk::now());
  const double* col = t.data();
  const double* row = t.data() + (rows_hi - geo_.tab_lo + 1) * 4;
  rowcls_host_ = row_classes(col, row, rows_hi, cols_hi, geo_.tab_lo);
  const std::vector<int>& rc = rowcls_host_;
  const auto t1 = clk::now();
  upload(rowcls_, rc.data(), sizeof(int) * rc.size());
  copy_setup_s_ += secs(t1, clk::now());
}

std::vector<Exchange> DeviceSolver::halo_plan() const {
  const KParams& k = *kp_;
  std::vector<Exchange> ex;
  if (blk_.has(LEFT))
    ex.push_back(Exchange{LEFT, blk_.nbr[LEFT], k.r + 1 * k.pitch + 1, k.r + 0 * k.pitch + 1, blk_.ny});
  if (blk_.has(RIGHT))
    ex.push_back(Exchange{RIGHT, blk_.nbr[RIGHT], k.r + blk_.nx * k.pitch + 1, k.r + (blk_.nx + 1) * k.pitch + 1,
                          blk_.ny});
  if (blk_.has(DOWN)) ex.push_back(Exchange{DOWN, blk_.nbr[DOWN], k.send_dn, const_cast<double*>(k.recv_dn), blk_.nx});
  if (blk_.has(UP)) ex.push_back(Exchange{UP, blk_.nbr[UP], k.send_up, const_cast<double*>(k.recv_up), blk_.nx});
  return ex;
}

std::vector<DeviceSolver::HaloPhase> DeviceSolver::halo_phases(int buf) const {
  if (!fused_) return {HaloPhase{halo_plan(), false}};
  const KParams& k = *kp_;
  std::vector<HaloPhase> ph(2);
  // Phase 0: y strips (2·hdep values per owned row: r and p of hdep columns;
  // the single sweep stores them from inside the sweep, the multi-step
  // sweeps' are packed after it — enqueue_exchange).
  const int64_t c = 2 * int64_t(geo_.hdep) * blk_.nx;
  if (blk_.has(DOWN)) ph[0].ex.push_back(Exchange{DOWN, blk_.nbr[DOWN], k.send_dn, const_cast<double*>(k.recv_dn), c});
  if (blk_.has(UP)) ph[0].ex.push_back(Exchange{UP, blk_.nbr[UP], k.send_up, const_cast<double*>(k.recv_up), c});
  ph[0].unpack = blk_.has(DOWN) || blk_.has(UP);
  // Phase 1: hdep full interleaved (r, p) rows per side, halo columns
  // included (so the corners arrive from the diagonal rank through the x
  // neighbour): rows 1..h → the LEFT neighbour's rows nx'+1..nx'+h, rows
  // nx-h+1..nx → the RIGHT neighbour's rows 1-h..0.
  double* x = k.x[buf];
  const int64_t h = geo_.hdep, n = h * k.pitch, hc = geo_.xorg;  // (whole rows: from column -xorg)
  if (blk_.has(LEFT))
    ph[1].ex.push_back(Exchange{LEFT, blk_.nbr[LEFT], x + 1 * k.pitch - hc, x + (1 - h) * k.pitch - hc, n});
  if (blk_.has(RIGHT))
    ph[1].ex.push_back(Exchange{RIGHT, blk_.nbr[RIGHT], x + (blk_.nx - h + 1) * k.pitch - hc,
                                x + (blk_.nx + 1) * k.pitch - hc, n});
  return ph;
}

void DeviceSolver::enqueue_exchange(int buf, bool after_sweep) {
  // halo push: the sweep that wrote `buf` has pushed its edge rows into the
  // neighbours' receive buffers, from which the next sweep reads them
  if (push_ && after_sweep) return;
  if (sstep_ && after_sweep) dev::launch_pack(*kp_, buf, stream_);  // (no-op without a y neighbour)
  for (const HaloPhase& ph : halo_phases(buf)) {
    xfer(ph.ex, stream_);
    if (ph.unpack) dev::launch_unpack(*kp_, buf, stream_);
  }
  // initial state through the comm: its halo rows into the receive buffer
  if (push_) dev::launch_halo_seed(*kp_, buf, stream_);
}

// halo push: x's halo rows ← the receive buffers (checkpoint, read-back)
void DeviceSolver::import_halos() {
  if (!push_) return;
  for (int b = 0; b < 2; ++b) dev::launch_halo_import(*kp_, b, stream_);
  PE_HIP_CHECK(hipGetLastError());
}

double* DeviceSolver::red_F_dev() { return st_->red_F; }
double* DeviceSolver::red_G_dev() { return st_->red_G; }
double* DeviceSolver::fs_dev(int par) { return st_->fs[par]; }
double* DeviceSolver::fs2_dev(int par) { return st_->fs2[par]; }
double* DeviceSolver::err_dev() { return st_->err; }

void DeviceSolver::enqueue_init() {
  const int64_t n = fused_ ? 2 * geo_.xsize + geo_.wsize : 4 * blk_.alloc;
  if (fused_) {
    PE_HIP_CHECK(hipMemsetAsync(fields_, 0, sizeof(double) * geo_.xsize, stream_));
    PE_HIP_CHECK(hipMemsetAsync(xalt_, 0, sizeof(double) * geo_.xsize, stream_));
    PE_HIP_CHECK(hipMemsetAsync(walt_, 0, sizeof(double) * geo_.wsize, stream_));
  } else {
    PE_HIP_CHECK(hipMemsetAsync(fields_, 0, sizeof(double) * n, stream_));
  }
  PE_HIP_CHECK(hipMemsetAsync(halo_, 0, sizeof(double) * hsize_ * 4, stream_));
  PE_HIP_CHECK(hipMemsetAsync(st_, 0, sizeof(DevState), stream_));
  ov_epoch_ = 0;
  if (rhs_dev_ || w0_dev_)  // user fields: kInit's sibling reads B / w⁰ from the planes
    dev::launch_init_field(*kp_, rhs_dev_, w0_dev_, opt_.init == Init::Random ? 1 : 0, opt_.seed, opt_.init_amp,
                           opt_.variant, stream_);
  else
    dev::launch_init(*kp_, opt_.init == Init::Random ? 1 : 0, opt_.seed, opt_.init_amp, opt_.variant, stream_);
  PE_HIP_CHECK(hipGetLastError());
}

void DeviceSolver::enqueue_F(int par) { dev::launch_F(*kp_, par, opt_.variant, stream_); }
void DeviceSolver::enqueue_G(int par) { dev::launch_G(*kp_, par, opt_.variant, stream_); }
void DeviceSolver::enqueue_S(int par) { dev::launch_S(*kp_, par, stream_); }
void DeviceSolver::enqueue_pack(int buf) { dev::launch_pack(*kp_, buf, stream_); }
void DeviceSolver::enqueue_unpack(int buf) { dev::launch_unpack(*kp_, buf, stream_); }
void DeviceSolver::enqueue_error() { dev::launch_error(*kp_, stream_, exact_dev_); }

// Cross-rank sum of sweep `par`'s 7 sums: nothing to enqueue when the sweep
// sums them over ranks itself (k.xr, P2P transport).
void DeviceSolver::enqueue_fs_reduce(int par) {
  if (kp_->xr.peers) return;
  if (sstep_) comm_->allreduce_sum(st_->fs2[par], dev::sweep_sums(steps_), stream_);
  else comm_->allreduce_sum(st_->fs[par], 7, stream_);
}

// Sampled phase timing: event pairs from a pool; a record's events are read
// (harvest) once the chunk that holds them has been waited for.
hipEvent_t DeviceSolver::pooled_event() {
  if (evpool_.empty()) {
    hipEvent_t e = nullptr;
    PE_HIP_CHECK(hipEventCreate(&e));
    return e;
  }
  hipEvent_t e = evpool_.back();
  evpool_.pop_back();
  return e;
}

void DeviceSolver::mark_begin(int ph, hipStream_t s) {
  if (!sampling_) return;
  PhaseRec r{ph, sample_iter_, steps_, pooled_event(), nullptr};  // (a multi-step sweep covers steps_ iterations)
  PE_HIP_CHECK(hipEventRecord(r.a, s));
  recs_.push_back(r);
}

void DeviceSolver::mark_end(hipStream_t s) {
  if (!sampling_) return;
  recs_.back().b = pooled_event();
  PE_HIP_CHECK(hipEventRecord(recs_.back().b, s));
}

void DeviceSolver::harvest(size_t n) {
  n = std::min(n, recs_.size());
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    PE_HIP_CHECK(hipEventElapsedTime(&ms, recs_[i].a, recs_[i].b));
    samples_.push_back(PhaseSample{recs_[i].ph, recs_[i].iter, recs_[i].n, ms});
    evpool_.push_back(recs_[i].a);
    evpool_.push_back(recs_[i].b);
  }
  recs_.erase(recs_.begin(), recs_.begin() + std::ptrdiff_t(n));
}

void DeviceSolver::enqueue_iteration(int par, int mlimit) {
  const int ncomm = comm_->size();
  if (fused_ && overlap_) {
    KParams ko = *kp_;
    ko.ilist = ilist_;
    for (int x = 0; x < 8; ++x) ko.lnb[x] = lay_.lnb[x];  // (lnsh, lbase: the plain launch's)
    ko.nblocks = std::max(lay_.lnsh, kp_->nblocks - lay_req_.ov_reserve);
    ko.nblocks0 = std::max(lay_.lnsh, kp_->nblocks0 - lay_req_.ov_reserve);
    ko.mlimit = mlimit;
    ov_epoch_ += 1;
    const unsigned long long target = ov_epoch_ * (unsigned long long)(lay_.nbnd);
    mark_begin(kPhSweep, stream_);
    dev::launch_S(ko, par, stream_, false);  // boundary items first in every shard
    mark_end(stream_);
    if (ko.order == 3) {
      mark_begin(kPhDot, stream_);
      dev::launch_red(ko, par, stream_);
      mark_end(stream_);
    }
    if (lay_req_.knobs.ov_debug & 2) {
      dev::launch_wait_sig(ko, target, stream_);
      mark_begin(kPhHalo, stream_);
      enqueue_exchange(par);
      mark_end(stream_);
    } else {
      dev::launch_wait_sig(ko, target, hs_);  // the exchange starts once they are stored
      mark_begin(kPhHalo, hs_);
      if (sstep_) dev::launch_pack(*kp_, par, hs_);  // (multi-step: y strips packed after the boundary items)
      for (const HaloPhase& ph : halo_phases(par)) {
        xfer(ph.ex, hs_);
        if (ph.unpack) dev::launch_unpack(*kp_, par, hs_);
      }
      mark_end(hs_);
      PE_HIP_CHECK(hipEventRecord(ev_halo_, hs_));
      PE_HIP_CHECK(hipStreamWaitEvent(stream_, ev_halo_, 0));
    }
    if (!kp_->xr.peers) {
      mark_begin(kPhReduce, stream_);
      enqueue_fs_reduce(par);
      mark_end(stream_);
    }
  } else if (fused_) {
    mark_begin(kPhSweep, stream_);
    if (mlimit > 0) {  // a partial three-step sweep: the run's last mlimit < 3 iterations
      KParams kk = *kp_;
      kk.mlimit = mlimit;
      dev::launch_S(kk, par, stream_, false);
    } else {
      dev::launch_S(*kp_, par, stream_, false);
    }
    mark_end(stream_);
    if (kp_->order == 3) {
      mark_begin(kPhDot, stream_);
      dev::launch_red(*kp_, par, stream_);
      mark_end(stream_);
    }
    if (ncomm > 1) {
      mark_begin(kPhHalo, stream_);
      enqueue_exchange(par);
      mark_end(stream_);
      if (!kp_->xr.peers) {
        mark_begin(kPhReduce, stream_);
        enqueue_fs_reduce(par);
        mark_end(stream_);
      }
    }
  } else {
    mark_begin(kPhSweep, stream_);
    dev::launch_F(*kp_, par, opt_.variant, stream_);
    mark_end(stream_);
    if (ncomm > 1) {
      mark_begin(kPhReduce, stream_);
      comm_->allreduce_sum(st_->red_F, 2, stream_);
      mark_end(stream_);
    }
    mark_begin(kPhSweep, stream_);
    dev::launch_G(*kp_, par, opt_.variant, stream_);
    mark_end(stream_);
    if (ncomm > 1) {
      mark_begin(kPhHalo, stream_);
      comm_->exchange(halo_plan(), stream_);
      mark_end(stream_);
      mark_begin(kPhReduce, stream_);
      comm_->allreduce_sum(st_->red_G, 1, stream_);
      mark_end(stream_);
    }
  }
  if (sampling_) sample_iter_ += mlimit > 0 ? mlimit : steps_;
}

// Chunk graphs are cached per length (a run of n iterations uses the chunk
// length and its remainder), so alternating lengths never re-capture.
hipGraphExec_t DeviceSolver::graph_for(int iters) {
  for (const auto& g : graphs_)
    if (g.first == iters) return g.second;
  const int per = steps_;
  if (iters % (2 * per)) throw std::logic_error("graph chunks must hold an even number of sweeps");
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  PE_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
  for (int it = 0; it < iters / per; ++it) enqueue_iteration(it & 1);
  PE_HIP_CHECK(hipStreamEndCapture(stream_, &g));
  PE_HIP_CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  PE_HIP_CHECK(hipGraphDestroy(g));
  // stage the executable's launch resources now, so its first replay (in a
  // bench's timed window) costs what the later ones do; stream-ordered, and
  // an optimisation only: a runtime without it replays the same graph
  if (hipGraphUpload(ge, stream_) != hipSuccess) (void)hipGetLastError();
  graphs_.emplace_back(iters, ge);
  return ge;
}

// (overlap: a graph may serialise the two streams' branches in any order,
// and the halo branch waits on the sweep — always eager)
// (no comm call in the iteration: the sweep's push or the put kernel for the
// halo, the in-sweep P2P sums for the scalars)
bool DeviceSolver::graphs_usable() const {
  return (comm_->capturable() || push_ || (put_ && kp_->xr.peers)) && !overlap_ && !resident_;
}

void DeviceSolver::enqueue_chunk(int iters, int sample_iters) {
  // The captured graph starts at parity 0 and has an even length; iterations
  // that would break the p / x ping-pong parity run eagerly.  A sampled
  // chunk runs eagerly with event pairs around the phases of its first
  // `sample_iters` iterations.
  int it = 0;
  if (resident_ && iters > 0) {
    // one launch for the whole chunk (always timed: two events per chunk)
    dev::ResParams r = *rp_;
    r.niter = iters;
    r.par0 = par_;
    PE_HIP_CHECK(hipMemsetAsync(res_ctr_, 0, sizeof(unsigned) * 8 * 32, stream_));
    const bool was = sampling_;
    sampling_ = true;
    mark_begin(kPhSweep, stream_);
    recs_.back().n = iters;
    dev::launch_resident(*kp_, r, stream_);
    mark_end(stream_);
    sampling_ = was;
    sample_iter_ += iters;
    par_ ^= iters & 1;
    PE_HIP_CHECK(hipGetLastError());
    return;
  }
  // (multi-step sweep: one launch = steps_ iterations; chunks are multiples
  // of 2·steps_; a three-step run of n iterations ends with a partial sweep
  // when 3 ∤ n)
  const int per = steps_;
  if (sample_iters == 0 && opt_.use_graph && graphs_usable() && par_ == 0 && iters >= 2 * per) {
    const int n = iters - iters % (2 * per);
    PE_HIP_CHECK(hipGraphLaunch(graph_for(n), stream_));
    it = n;
  }
  for (; it < iters; it += per) {
    sampling_ = it < sample_iters;
    enqueue_iteration(par_, steps_ >= 3 && iters - it < per ? iters - it : 0);
    par_ ^= 1;
  }
  sampling_ = false;
  PE_HIP_CHECK(hipGetLastError());
}

void DeviceSolver::prepare_graphs(int64_t iters) {
  if (!graphs_usable()) return;
  // the chunk lengths run_iterations(iters) launches from parity 0
  const int64_t full = iters / chunk_, rest = iters % chunk_;
  const int64_t q = 2 * steps_;
  if (full > 0) graph_for(chunk_);
  if (rest >= q) graph_for(int(rest - rest % q));
  // the capture enqueued nothing: the stream state is unchanged
}


void DeviceSolver::wait_event(hipEvent_t ev) {
  const auto t0 = clk::now();
  for (;;) {
    const hipError_t q = fault_stall_ ? hipErrorNotReady : hipEventQuery(ev);
    if (q == hipSuccess) return;
    if (q != hipErrorNotReady) PE_HIP_CHECK(q);
    comm_->check_async();
    if (watchdog_s_ > 0 && secs(t0, clk::now()) > watchdog_s_) {
      comm_->abort();
      throw std::runtime_error("watchdog: device made no progress for " + std::to_string(watchdog_s_) +
                               " s (communicator aborted)");
    }
    // spin (yielding) for the first 250 ms, then poll every 20 µs: a sleeping
    // poll detects the end late by up to a scheduler tick, and a bench's
    // closing wait of a 5 ms window used to span the 2 ms the spin lasted
    if (secs(t0, clk::now()) > 0.25) std::this_thread::sleep_for(std::chrono::microseconds(20));
    else std::this_thread::yield();
  }
}

void DeviceSolver::enqueue_wflush() {
  if (!fused_) return;
  if (steps_ >= 3) {  // the last sweep's pending stop tests (and its w fix-up when it converged early)
    KParams kk = *kp_;
    kk.mlimit = -1;
    dev::launch_S(kk, par_, stream_);
    return;
  }
  dev::launch_wflush(*kp_, stream_);
}

void DeviceSolver::residual_pass(bool with_r, bool store) {
  const KParams& k = *kp_;
  dev::launch_w_to_p(k, 0, stream_);
  if (comm_->size() > 1) {  // w's halo: x[0]'s exchange (y strips packed first, as reset() does)
    dev::launch_pack(k, 0, stream_);
    enqueue_exchange(0, false);
  }
  dev::launch_resid(k, 0, with_r, store, stream_, rhs_dev_);  // (user rhs: the check and the restart's ρ are the user's problem's)
  if (comm_->size() > 1) comm_->allreduce_sum(st_->res, 4, stream_);
  PE_HIP_CHECK(hipGetLastError());
}

// The gradient pass, residual_pass's sequence: w (flushed) into a plane the
// layout exchanges — the p-plane of x[0], or the classic r plane with its y
// strips — that plane's halo exchange, then kGradField reading it through
// (base, pitch).  The iteration state in that plane is gone afterwards.
void DeviceSolver::enqueue_grad_stage() {
  const KParams& k = *kp_;
  scratch_used_ = true;
  enqueue_wflush();
  if (fused_) {
    dev::launch_w_to_p(k, 0, stream_);
    dev::launch_pack(k, 0, stream_);  // (no-op without a y neighbour)
  } else {
    dev::launch_w_to_r(k, stream_);
  }
}

void DeviceSolver::enqueue_grad(double* gx, double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j) {
  const KParams& k = *kp_;
  if (fused_) {
    dev::launch_grad_field(k, k.x[0] + k.poff, k.pitch, gx, gy, si, sj, off_i, off_j, stream_);
  } else {
    dev::launch_unpack_r(k, stream_);
    dev::launch_grad_field(k, k.r, k.pitch, gx, gy, si, sj, off_i, off_j, stream_);
  }
  PE_HIP_CHECK(hipGetLastError());
}

double* DeviceSolver::res_dev() { return st_->res; }

GradStats DeviceSolver::gradient_pass(double* gx, double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j) {
  enqueue_grad_stage();
  if (comm_->size() > 1) {
    if (fused_) enqueue_exchange(0, false);
    else comm_->exchange(halo_plan(), stream_);
  }
  enqueue_grad(gx, gy, si, sj, off_i, off_j);
  if (comm_->size() > 1) {
    comm_->allreduce_sum(st_->res, 2, stream_);
    comm_->allreduce_max(st_->res + 2, 1, stream_);
  }
  DevState hs;
  read_state(&hs);
  const double hh = prob_.h1() * prob_.h2();
  GradStats g;
  g.integral = hh * hs.res[0];
  g.energy = hh * hs.res[1];
  g.grad_max = std::sqrt(hs.res[2]);
  return g;
}

GradStats DeviceSolver::gradient(double* gx_host, double* gy_host) {
  if ((gx_host == nullptr) != (gy_host == nullptr)) throw std::invalid_argument("gradient: gx and gy go together");
  if (!gx_host) return gradient_pass(nullptr, nullptr, 0, 0, 0, 0);
  const size_t n = size_t(blk_.nx * blk_.ny);
  double* d = nullptr;
  PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), sizeof(double) * 2 * n));
  GradStats g;
  try {
    g = gradient_pass(d, d + n, blk_.ny, 1, 0, 0);
    PE_HIP_CHECK(hipMemcpyAsync(gx_host, d, sizeof(double) * n, hipMemcpyDeviceToHost, stream_));
    PE_HIP_CHECK(hipMemcpyAsync(gy_host, d + n, sizeof(double) * n, hipMemcpyDeviceToHost, stream_));
    PE_HIP_CHECK(hipStreamSynchronize(stream_));
  } catch (...) {
    (void)hipFree(d);
    throw;
  }
  PE_HIP_CHECK(hipFree(d));
  return g;
}

void DeviceSolver::check_grad_span(const double* gx, const double* gy, int64_t si, int64_t sj, int64_t off_i,
                                   int64_t off_j) const {
  if (!gx || !gy) throw std::invalid_argument("grad: null destination");
  if (si < 0 || sj < 0 || off_i < 0 || off_j < 0) throw std::invalid_argument("grad: negative stride or offset");
  // (each destination from its element [0][0] to this block's last element)
  const int64_t last = (off_i + blk_.nx - 1) * si + (off_j + blk_.ny - 1) * sj;
  check_device_span(gx, last, sizeof(double), "grad x");
  check_device_span(gy, last, sizeof(double), "grad y");
}

GradStats DeviceSolver::gradient_device(double* gx, double* gy, int64_t si, int64_t sj, int64_t off_i, int64_t off_j,
                                        hipStream_t consumer) {
  if ((gx == nullptr) != (gy == nullptr)) throw std::invalid_argument("grad: gx and gy go together");
  if (!gx) return gradient_pass(nullptr, nullptr, 0, 0, 0, 0);
  check_grad_span(gx, gy, si, sj, off_i, off_j);
  io_events();
  PE_HIP_CHECK(hipEventRecord(ev_io_[0], consumer));
  PE_HIP_CHECK(hipStreamWaitEvent(stream_, ev_io_[0], 0));
  const GradStats g = gradient_pass(gx, gy, si, sj, off_i, off_j);
  PE_HIP_CHECK(hipEventRecord(ev_io_[1], stream_));
  PE_HIP_CHECK(hipStreamWaitEvent(consumer, ev_io_[1], 0));
  return g;
}

// The operator pass (kApplyField): the caller's global array is read in place —
// no plane of the iteration is touched, scratch_used_ stays as it is.
void DeviceSolver::check_apply_span(const void* v, int64_t si, int64_t sj, bool f32, const double* dst, int64_t dsi,
                                    int64_t dsj, int64_t off_i, int64_t off_j) const {
  if (!v) throw std::invalid_argument("field: null array");
  if (si < 0 || sj < 0) throw std::invalid_argument("field: negative stride");
  const int64_t gnx = int64_t(prob_.M) - 1, gny = int64_t(prob_.N) - 1;
  check_device_span(v, (gnx - 1) * si + (gny - 1) * sj, f32 ? sizeof(float) : sizeof(double), "field");
  if (!dst) return;
  if (dsi < 0 || dsj < 0 || off_i < 0 || off_j < 0) throw std::invalid_argument("out: negative stride or offset");
  // (the destination from its element [0][0] to this block's last element)
  check_device_span(dst, (off_i + blk_.nx - 1) * dsi + (off_j + blk_.ny - 1) * dsj, sizeof(double), "out");
}

void DeviceSolver::enqueue_apply(const void* v, int64_t si, int64_t sj, bool f32, bool resid, double* dst, int64_t dsi,
                                 int64_t dsj, int64_t off_i, int64_t off_j) {
  dev::launch_apply_field(*kp_, v, f32, si, sj, resid, resid ? rhs_dev_ : nullptr, dst, dsi, dsj, off_i, off_j, stream_);
  PE_HIP_CHECK(hipGetLastError());
}

double DeviceSolver::operator_pass(const void* v, int64_t si, int64_t sj, bool f32, bool resid, double* dst, int64_t dsi,
                                   int64_t dsj, int64_t off_i, int64_t off_j, hipStream_t caller) {
  check_apply_span(v, si, sj, f32, dst, dsi, dsj, off_i, off_j);
  if (prob_.reaction && !react_set_)
    throw std::invalid_argument("reaction: the problem has a reaction field and none is set (set_reaction / set_reaction_device)");
  io_events();
  PE_HIP_CHECK(hipEventRecord(ev_io_[0], caller));
  PE_HIP_CHECK(hipStreamWaitEvent(stream_, ev_io_[0], 0));
  enqueue_apply(v, si, sj, f32, resid, dst, dsi, dsj, off_i, off_j);
  PE_HIP_CHECK(hipEventRecord(ev_io_[1], stream_));
  PE_HIP_CHECK(hipStreamWaitEvent(caller, ev_io_[1], 0));
  if (comm_->size() > 1) comm_->allreduce_sum(st_->res, 1, stream_);
  DevState hs;
  read_state(&hs);
  return prob_.h1() * prob_.h2() * hs.res[0];
}

double DeviceSolver::apply_device(const void* v, int64_t si, int64_t sj, bool f32, double* dst, int64_t dsi, int64_t dsj,
                                  int64_t off_i, int64_t off_j, hipStream_t caller) {
  return operator_pass(v, si, sj, f32, false, dst, dsi, dsj, off_i, off_j, caller);
}

double DeviceSolver::residual_device(const void* w, int64_t si, int64_t sj, bool f32, double* dst, int64_t dsi,
                                     int64_t dsj, int64_t off_i, int64_t off_j, hipStream_t caller) {
  return operator_pass(w, si, sj, f32, true, dst, dsi, dsj, off_i, off_j, caller);
}

double DeviceSolver::operator_host(const double* v, double* out, bool resid) {
  if (!v) throw std::invalid_argument("field: null array");
  const int64_t gny = int64_t(prob_.N) - 1;
  const size_t gn = size_t((int64_t(prob_.M) - 1) * gny), n = size_t(blk_.nx * blk_.ny);
  double* d = nullptr;  // the global operand, then the owned result
  PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), sizeof(double) * (gn + (out ? n : 0))));
  double sum = 0.0;
  try {
    PE_HIP_CHECK(hipMemcpyAsync(d, v, sizeof(double) * gn, hipMemcpyHostToDevice, stream_));
    sum = operator_pass(d, gny, 1, false, resid, out ? d + gn : nullptr, blk_.ny, 1, 0, 0, stream_);
    if (out) {
      PE_HIP_CHECK(hipMemcpyAsync(out, d + gn, sizeof(double) * n, hipMemcpyDeviceToHost, stream_));
      PE_HIP_CHECK(hipStreamSynchronize(stream_));
    }
  } catch (...) {
    (void)hipFree(d);
    throw;
  }
  PE_HIP_CHECK(hipFree(d));
  return sum;
}

double DeviceSolver::apply(const double* v, double* out) { return operator_host(v, out, false); }
double DeviceSolver::residual(const double* w, double* out) { return operator_host(w, out, true); }

void DeviceSolver::read_state(DevState* out) {
  PE_HIP_CHECK(hipMemcpyAsync(out, st_, sizeof(DevState), hipMemcpyDeviceToHost, stream_));
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSolver::synchronize() {
  if (watchdog_s_ <= 0 && !fault_stall_) {
    PE_HIP_CHECK(hipStreamSynchronize(stream_));
    return;
  }
  PE_HIP_CHECK(hipEventRecord(ev_sync_, stream_));
  wait_event(ev_sync_);
}

void DeviceSolver::reset() {
  if (prob_.reaction && !react_set_)
    throw std::invalid_argument("reaction: the problem has a reaction field and none is set (set_reaction / set_reaction_device)");
  par_ = 0;
  scratch_used_ = false;
  enqueue_init();
  if (fused_) {
    // r⁰ (and p = 0) in x[0] → halos → sweep S_0 (z₀, A z₀ and their sums,
    // no iteration counted) into x[1]; iteration 1 then reads x[1] (par 0).
    dev::launch_pack(*kp_, 0, stream_);
    enqueue_exchange(0, false);
    dev::launch_S(*kp_, 1, stream_);
    enqueue_exchange(1);
    enqueue_fs_reduce(1);
    return;
  }
  comm_->exchange(halo_plan(), stream_);
  comm_->allreduce_sum(st_->red_G, 1, stream_);
}

void DeviceSolver::run_iterations(int64_t iters, bool use_graph) {
  if (scratch_used_)
    throw std::logic_error("run_iterations after gradient(): the pass used an iteration plane as scratch; reset() or solve() first");
  // (the three-step sweep ends an n-iteration run with a partial sweep when
  // 3 ∤ n; the two-step sweep has none — its one-iteration sweep ends the
  // solve — so an odd count would run one iteration too many)
  if (steps_ == 2 && iters % 2 != 0)
    throw std::invalid_argument("two-step sweep: run an even number of iterations (got " + std::to_string(iters) + ")");
  const bool saved = opt_.use_graph;
  opt_.use_graph = use_graph;
  int64_t done = 0;
  while (done < iters) {
    const int64_t n = std::min<int64_t>(chunk_, iters - done);
    enqueue_chunk(int(n));
    done += n;
  }
  opt_.use_graph = saved;
}

double DeviceSolver::time_iterations(int64_t iters, bool use_graph) {
  PE_HIP_CHECK(hipEventRecord(t0_, stream_));
  run_iterations(iters, use_graph);
  PE_HIP_CHECK(hipEventRecord(t1_, stream_));
  PE_HIP_CHECK(hipEventSynchronize(t1_));
  float ms = 0;
  PE_HIP_CHECK(hipEventElapsedTime(&ms, t0_, t1_));
  return ms * 1e-3;
}

SolveResult DeviceSolver::solve() {
  Range range("pe.solve");
  const auto t_start = clk::now();
  SolveResult res;
  res.backend = "hip";
  res.algo = algo_name(fused_, steps_, resident_);
  res.Px = blk_.Px;
  res.Py = blk_.Py;
  // T_solver spans construction (allocation, tables, placement search) like
  // the reference's time_solver (poisson_mpi_cuda2.cu:1010-1016); a second
  // solve on the same solver reuses it and does not count it again.
  const double construct = ctor_counted_ ? 0.0 : ctor_s_;
  ctor_counted_ = true;
  double copy_s = construct > 0 ? copy_setup_s_ : 0.0;
  int64_t start_iter = 0;
  if (!opt_.resume_path.empty()) {
    const auto tc = clk::now();
    load_checkpoint(opt_.resume_path + ".r" + std::to_string(blk_.rank));
    scratch_used_ = false;  // (every plane comes from the file)
    copy_s += secs(tc, clk::now());
    DevState s0;
    read_state(&s0);
    start_iter = s0.iter;
  } else {
    reset();
  }
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
  // Residual rule: the threshold from the reduced g_0 (the same bits on every
  // rank) into the device state, on the solver stream, before the first
  // iteration is enqueued; a resumed solve keeps the one its file carries.
  const bool res_rule = prob_.stop == Stop::Residual;
  auto set_threshold = [&]() {
    if (!res_rule || !opt_.resume_path.empty()) return;
    DevState s0;
    read_state(&s0);
    const double g0 = stop_g0(s0);
    enqueue_stop_threshold(stop_threshold(prob_, g0), std::sqrt(g0));
  };
  set_threshold();
  res.t.construct = construct;
  res.t.setup = construct + secs(t_start, clk::now());
  const int64_t ck_every = opt_.checkpoint_path.empty() ? 0 : opt_.checkpoint_every;

  // Phase sampling: every `sample_every`-th chunk, its first two iterations
  // (all of them with opt_.timing); no host sync beyond the per-chunk state
  // read the loop does anyway.
  int sample_every = 8, sample_iters = 2;
  if (const std::optional<int> e = read_env_knobs().timer_sample) sample_every = std::max(0, *e);
  if (opt_.timing) {
    sample_every = 1;
    sample_iters = chunk_;
  }
  samples_.clear();
  sample_iter_ = start_iter;

  const int64_t cap = prob_.iter_cap();
  const auto t_loop = clk::now();
  roctxRangePushA("pe.iterate");
  PE_HIP_CHECK(hipEventRecord(t0_, stream_));
  int64_t enq = start_iter;
  int64_t next_ck = ck_every > 0 ? (start_iter / ck_every + 1) * ck_every : std::numeric_limits<int64_t>::max();
  int64_t next_log = opt_.log_every > 0 ? opt_.log_every : 0;
  int slot = 0;
  struct Flight {
    int slot;
    size_t nrec;  // phase records enqueued up to and including this chunk
  };
  std::deque<Flight> inflight;
  int64_t nchunk = 0;
  bool stop = false;
  bool res_abort = false;  // a resident launch's grid barrier timed out (status 5)
  bool drift_done = fault_drift_ <= 0;
  int restarts = 0;
  DevState hs;
  double check_s = 0.0;
  for (;;) {  // (a three-step restart runs the loop again from the restart's iteration)
    for (;;) {
      while (!stop && enq < cap && inflight.size() < 2 && enq < next_ck) {
        const bool sample = sample_every > 0 && nchunk % sample_every == 0;
        sample_iter_ = enq;
        enqueue_chunk(chunk_, sample ? sample_iters : 0);
        enq += chunk_;
        if (!drift_done && enq >= fault_drift_) {  // PE_FAULT_INJECT=drift@iter:K
          drift_done = true;
          const int64_t li = prob_.M / 2 - kp_->gi0, lj = prob_.N / 2 - kp_->gj0;
          if (fused_ && li >= 1 && li <= blk_.nx && lj >= 1 && lj <= blk_.ny)
            dev::launch_poke_w(*kp_, li, lj, fault_drift_amp_, stream_);
        }
        sampling_ = sample;
        sample_iter_ = enq - 1;
        mark_begin(kPhCopy, stream_);
        // per-chunk state read: a copy kernel into mapped pinned memory (a
        // hipMemcpyAsync's first use initialises the runtime's copy path
        // inside T_solver)
        dev::launch_copy_words(&hst_[slot], st_, sizeof(DevState), true, stream_);
        mark_end(stream_);
        sampling_ = false;
        PE_HIP_CHECK(hipEventRecord(ev_[slot], stream_));
        inflight.push_back(Flight{slot, recs_.size()});
        slot ^= 1;
        ++nchunk;
      }
      if (inflight.empty()) {
        if (!stop && enq < cap && enq >= next_ck) {  // drained at a checkpoint boundary
          const auto tc = clk::now();
          save_checkpoint(opt_.checkpoint_path + ".r" + std::to_string(blk_.rank));
          copy_s += secs(tc, clk::now());
          while (next_ck <= enq) next_ck += ck_every;
          continue;
        }
        if (res_abort) {
          // Resident fallback: a workgroup of a resident launch timed out at a
          // grid barrier.  The aborted launch may still have written back part
          // of the grid (a late workgroup passes the barrier the others gave up
          // on), so its state is not resumed: the solve starts over from its
          // initial state (or its checkpoint) on the streaming sweep.
          res_abort = false;
          DevState s0;
          read_state(&s0);
          std::fprintf(stderr, "[pe] rank %d: resident kernel barrier timed out by iteration %lld; "
                               "restarting the solve with the streaming sweep\n", blk_.rank, (long long)s0.iter);
          resident_ = false;
          resident_fallback_ = true;
          chunk_ = stream_chunk_;
          harvest(recs_.size());
          samples_.clear();
          if (!opt_.resume_path.empty()) load_checkpoint(opt_.resume_path + ".r" + std::to_string(blk_.rank));
          else reset();
          set_threshold();  // (the reset zeroed the state)
          enq = start_iter;
          sample_iter_ = start_iter;
          stop = false;
          continue;
        }
        break;
      }
      const Flight f = inflight.front();
      inflight.pop_front();
      wait_event(ev_[f.slot]);
      // this chunk's (and every earlier) phase events have completed
      const size_t done_recs = std::min(f.nrec, recs_.size());
      harvest(done_recs);
      for (Flight& g : inflight) g.nrec -= std::min(g.nrec, done_recs);
      if (hst_[f.slot].done) {
        stop = true;
        if ((hst_[f.slot].status == 5 || hst_[f.slot].res_abort) && resident_) res_abort = true;
      }
      if (opt_.log_every > 0 && blk_.rank == 0 && hst_[f.slot].iter >= next_log) {  // chunk-granular progress log
        std::fprintf(stderr, "[pe] iter %lld  |dw| = %.6e  (z,r) = %.6e\n", (long long)hst_[f.slot].iter,
                     hst_[f.slot].last_diff, hst_[f.slot].rz_cur);
        while (next_log <= hst_[f.slot].iter) next_log += opt_.log_every;
      }
    }
    // True-residual check of the returned w: ρ = B − A w.  Three-step: the
    // s-step moment recurrence (fused3.hip) is checked against it — after a
    // fix-up (the solve stopped inside the last sweep), the replay launch
    // first recomputes that iterate's r into x[wpar], so w and r belong to the
    // same iterate.
    const bool three = fused_ && steps_ >= 3;  // (three-step: the moment recurrence)
    enqueue_wflush();
    // (the check below is timed on its own: res.t.check, outside T_iterate, inside T_solver)
    PE_HIP_CHECK(hipStreamSynchronize(stream_));
    const auto t_chk = clk::now();
    if (three) {  // (after a fix-up: x[wpar] ← the r of the returned w)
      KParams kk = *kp_;
      kk.mlimit = dev::kReplay3;
      dev::launch_S(kk, par_, stream_);
    }
    if (fused_) residual_pass(three, three);
    read_state(&hs);
    check_s += secs(t_chk, clk::now());
    const double hh = prob_.h1() * prob_.h2();
    if (three) {
      res.res_rec = std::sqrt(hs.res[1] * hh);
      // relative to the recurrence's own ‖r‖: the fp64 gap of any CG recurrence
    // scales with the residuals it has summed, not with ‖B‖ (8192² random
    // init: 8e-3 absolute = 5e-7 of ‖r‖ = 1.5e4; zero init 2e-10 of ‖r‖ —
    // profiles/r4_resid.txt)
    res.res_gap = std::sqrt(hs.res[2] / std::max(hs.res[1], 1e-300));
    }
    if (fused_) {
      res.res_true = std::sqrt(hs.res[0] * hh);
      res.b_norm = std::sqrt(hs.res[3] * hh);
    }
    // Residual replacement: a converged three-step solve whose recurrence has
    // drifted from B − A w (gap above PE_RESID_GAP, default 1e-4 of ‖r‖) goes on
    // from the returned w with r = B − A w (stored by the pass above), p = 0 and
    // a fresh recurrence (β = 0 after the restart), at most twice.  Every rank
    // reads the same reduced sums: every rank decides the same.
    if (three && hs.status == 1 && res.res_gap > gap_bound_ && restarts < 2 && hs.iter < cap) {
      ++restarts;
      std::fprintf(stderr, "[pe] rank %d: residual gap %.3e > %.1e at iteration %lld; restarting the recurrence from w\n",
                   blk_.rank, res.res_gap, gap_bound_, (long long)hs.iter);
      dev::launch_zero_p(*kp_, 0, stream_);
      dev::launch_restart3(*kp_, stream_);
      ov_epoch_ = 0;
      dev::launch_pack(*kp_, 0, stream_);
      enqueue_exchange(0, false);
      dev::launch_S(*kp_, 1, stream_);
      enqueue_exchange(1);
      enqueue_fs_reduce(1);
      par_ = 0;
      enq = hs.iter;
      stop = false;
      continue;
    }
    break;
  }
  res.restarts = restarts;
  PE_HIP_CHECK(hipEventRecord(t1_, stream_));
  PE_HIP_CHECK(hipEventSynchronize(t1_));
  harvest(recs_.size());
  float ms = 0;
  PE_HIP_CHECK(hipEventElapsedTime(&ms, t0_, t1_));
  res.t.iterate = secs(t_loop, clk::now()) - check_s;
  res.t.check = check_s;
  roctxRangePop();

  if (opt_.compute_error) {
    dev::launch_error(*kp_, stream_, exact_dev_);
    comm_->allreduce_sum(st_->err, 1, stream_);
    comm_->allreduce_max(st_->err + 1, 2, stream_);
  }
  read_state(&hs);
  res.iters = hs.iter;
  res.converged = hs.status == 1;
  res.breakdown = hs.status == 2;
  res.nonfinite = hs.status == 4;
  res.resident_fallback = resident_fallback_;
  if (resident_fallback_) res.algo = "fused (resident fallback)";
  if (hs.status == 5) throw std::runtime_error("single-sweep: internal error (status 5: a grid barrier or item sums never completed)");
  res.last_diff = hs.last_diff;
  if (hist_ && hs.iter > 0) {
    res.history.resize(size_t(std::min<long long>(hs.iter, kp_->hist_n)));
    PE_HIP_CHECK(hipMemcpyAsync(res.history.data(), hist_, sizeof(double) * res.history.size(), hipMemcpyDeviceToHost,
                                stream_));
    PE_HIP_CHECK(hipStreamSynchronize(stream_));
  }
  res.zr = hs.rz_cur;
  if (res_rule) {  // (the terminal paths of the rule leave g_K in rz_cur)
    res.res_nat0 = hs.err[3];
    res.stop_thr = hs.red_G[1];
    if (res.converged) res.res_nat = std::sqrt(hs.rz_cur);
  }
  if (opt_.compute_error) {
    // (a user right-hand side, a shifted operator or a reaction field without a user exact solution has nothing to
    // compare with: -1)
    const bool no_exact = (rhs_dev_ || prob_.shift != 0.0 || prob_.reaction) && !exact_dev_;
    res.l2_err = no_exact ? -1.0 : std::sqrt(hs.err[0] * prob_.h1() * prob_.h2());
    res.max_err = no_exact ? -1.0 : hs.err[1];
    res.max_outside = hs.err[2];
  }
  // Per-phase totals: mean per sampled live iteration (samples taken after
  // the solve had stopped time no-op kernels and are dropped) × iterations
  // run; the state read per chunk likewise × chunks run.
  {
    const int64_t run = std::max<int64_t>(0, hs.iter - start_iter);
    double sum[kNPhase] = {};
    std::vector<char> seen(size_t(std::max<int64_t>(1, run)), 0);
    int64_t nit = 0, ncopy = 0;
    for (const PhaseSample& x : samples_) {
      if (x.iter >= hs.iter) continue;
      sum[x.ph] += x.ms * 1e-3;
      if (x.ph == kPhCopy) {
        ++ncopy;
      } else if (x.n > 1) {  // a resident launch: the iterations it ran before the solve stopped
        nit += std::min<int64_t>(x.n, hs.iter - x.iter);
      } else if (x.iter >= start_iter && !seen[size_t(x.iter - start_iter)]) {
        seen[size_t(x.iter - start_iter)] = 1;
        ++nit;
      }
    }
    const double scale = nit > 0 ? double(run) / double(nit) : 0.0;
    const int64_t chunks_run = (run + chunk_ - 1) / chunk_;
    res.t.gpu = (sum[kPhSweep] + sum[kPhDot]) * scale;
    res.t.dot = sum[kPhDot] * scale;
    res.t.halo = sum[kPhHalo] * scale;
    res.t.reduce = sum[kPhReduce] * scale;
    res.t.copy = copy_s + (ncopy > 0 ? sum[kPhCopy] * double(chunks_run) / double(ncopy) : 0.0);
    res.t.sampled = double(nit);
    // in-sweep cross-rank sum: the final blocks' wait for the peers' flags
    // (ticks of the 100 MHz s_memrealtime clock)
    res.t.wait = double(hs.xr_wait) * 1e-8;
    res.t.dot_fused = !(fused_ && kp_->order == 3);
    if (nit == 0) res.t.gpu = ms * 1e-3;  // sampling off: the loop's device span
  }
  // T_solver spans the whole solve, the end-of-solve residual check included
  // (it drives the residual-replacement restart: part of the solve, as the
  // reference's time_solver spans its whole gradient_solver_mpi call); t_check
  // reports it separately and T_iterate excludes it
  res.t.solver = construct + secs(t_start, clk::now());
  // Timers: max over ranks (reference MPI_Reduce(MAX), :962-966).
  double tv[11] = {res.t.gpu, res.t.copy, res.t.halo, res.t.reduce, res.t.setup, res.t.solver, res.t.iterate,
                   res.t.dot, res.t.construct, res.t.wait, res.t.check};
  comm_->host_max(tv, 11, stream_);
  res.t.check = tv[10];
  res.t.wait = tv[9];
  res.t.gpu = tv[0];
  res.t.copy = tv[1];
  res.t.halo = tv[2];
  res.t.reduce = tv[3];
  res.t.setup = tv[4];
  res.t.solver = tv[5];
  res.t.iterate = tv[6];
  res.t.dot = tv[7];
  res.t.construct = tv[8];
  return res;
}

void DeviceSolver::copy_w(double* host, bool owned_only) {
  const KParams& k = *kp_;
  enqueue_wflush();
  if (owned_only) {
    PE_HIP_CHECK(hipMemcpy2DAsync(host, sizeof(double) * blk_.ny, k.w + k.wpitch + 1, sizeof(double) * k.wpitch,
                                  sizeof(double) * blk_.ny, blk_.nx, hipMemcpyDeviceToHost, stream_));
  } else {
    PE_HIP_CHECK(hipMemcpyAsync(host, k.w, sizeof(double) * blk_.rows * k.wpitch, hipMemcpyDeviceToHost, stream_));
  }
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSolver::copy_w_device(double* dst, int64_t si, int64_t sj, int64_t off_i, int64_t off_j,
                                 hipStream_t consumer) {
  if (!dst) throw std::invalid_argument("w: null destination");
  if (si < 0 || sj < 0 || off_i < 0 || off_j < 0) throw std::invalid_argument("w: negative stride or offset");
  // (the check spans the destination from its element [0][0] to this block's last element)
  check_device_span(dst, (off_i + blk_.nx - 1) * si + (off_j + blk_.ny - 1) * sj, sizeof(double), "w");
  io_events();
  PE_HIP_CHECK(hipEventRecord(ev_io_[0], consumer));
  PE_HIP_CHECK(hipStreamWaitEvent(stream_, ev_io_[0], 0));
  enqueue_wflush();
  dev::launch_gather_w(*kp_, dst, si, sj, off_i, off_j, stream_);
  PE_HIP_CHECK(hipGetLastError());
  PE_HIP_CHECK(hipEventRecord(ev_io_[1], stream_));
  PE_HIP_CHECK(hipStreamWaitEvent(consumer, ev_io_[1], 0));
}

int64_t DeviceSolver::field_rows() const { return fused_ ? blk_.nx + 4 : blk_.rows; }
int64_t DeviceSolver::field_cols() const { return fused_ ? geo_.plane : blk_.pitch; }

void DeviceSolver::copy_field(int which, double* host) {
  const KParams& k = *kp_;
  if (fused_) {
    import_halos();
    // rows -1..nx+2 of one plane, columns -1.. (plane width)
    const double* base = which == 0 ? k.x[0] : which == 1 ? k.w : which == 2 ? k.x[0] + k.poff
                         : which == 3 ? k.x[1] + k.poff : k.x[1];
    const int64_t stride = which == 1 ? k.wpitch : k.pitch;
    PE_HIP_CHECK(hipMemcpy2DAsync(host, sizeof(double) * geo_.plane, base - stride - 1, sizeof(double) * stride,
                                  sizeof(double) * geo_.plane, blk_.nx + 4, hipMemcpyDeviceToHost, stream_));
  } else {
    const double* src = which == 0 ? k.r : which == 1 ? k.w : which == 2 ? k.p[0] : k.p[1];
    PE_HIP_CHECK(hipMemcpyAsync(host, src, sizeof(double) * blk_.rows * k.pitch, hipMemcpyDeviceToHost, stream_));
  }
  PE_HIP_CHECK(hipStreamSynchronize(stream_));
}

// ---------------------------------------------------------------------------
// Virtual ranks on one device.
// ---------------------------------------------------------------------------
SolveResult device_solve_group(const Problem& P, int ranks, DecompMode mode, const SolveOptions& opt,
                               std::vector<double>* w_out, const UserFields& uf) {
  return device_solve_group(P, choose_process_grid(ranks, P.M, P.N, mode), opt, w_out, uf);
}

SolveResult device_solve_group(const Problem& P, const ProcessGrid& pg, const SolveOptions& opt,
                               std::vector<double>* w_out, const UserFields& uf, const DeviceFields& df,
                               const GroupGradient& gg) {
  const auto t_start = clk::now();
  const int ranks = pg.Px * pg.Py;
  // the reaction field: a host array is checked here, a device array by its producer (before any launch either way)
  if (df.reaction) {
    if (!P.reaction) throw std::invalid_argument("device_solve_group: a reaction field without Problem::reaction");
  } else {
    check_reaction(P, uf.reaction, "device_solve_group");
  }
  std::vector<std::unique_ptr<DeviceSolver>> s;
  std::vector<Block> blks;
  for (int r = 0; r < ranks; ++r) {
    blks.push_back(decompose(P.M, P.N, pg, r));
    s.push_back(std::make_unique<DeviceSolver>(P, blks.back(), nullptr, opt));
    if (df.reaction) s.back()->set_reaction_device(df.reaction, df.reaction_si, df.reaction_sj, df.reaction_f32, df.stream);
    else if (uf.reaction) s.back()->set_reaction(block_field(uf.reaction, P.M, P.N, blks.back(), 1).data());
    if (df.rhs) s.back()->set_rhs_device(df.rhs, df.rhs_si, df.rhs_sj, df.rhs_f32, df.stream);
    else if (uf.rhs) s.back()->set_rhs(block_field(uf.rhs, P.M, P.N, blks.back(), 0).data());
    if (df.w0) s.back()->set_w0_device(df.w0, df.w0_si, df.w0_sj, df.w0_f32, df.stream);
    else if (uf.w0) s.back()->set_w0(block_field(uf.w0, P.M, P.N, blks.back(), 1).data());
    if (df.exact) s.back()->set_exact_device(df.exact, df.exact_si, df.exact_sj, df.exact_f32, df.stream);
    else if (uf.exact) s.back()->set_exact(block_field(uf.exact, P.M, P.N, blks.back(), 0).data());
  }
  const bool fused = s[0]->fused();
  // multi-step sweeps (three-step on blocks of >= 12 x 12): one launch per
  // `steps` iterations, the exchange after each, the kNS3 sums summed here
  const int steps = s[0]->sweep_steps();
  const bool ms = s[0]->two_step();
  const int nsum = dev::sweep_sums(steps);
  std::vector<hipEvent_t> ev(ranks);
  for (auto& e : ev) PE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // Device pointer tables for the cross-rank reduction kernel:
  // [red_F | red_G | err | fs0 | fs1] × ranks (multi-step: fs2[0] / fs2[1]
  // in the fs slots).
  std::vector<double*> hp(5 * ranks);
  for (int r = 0; r < ranks; ++r) {
    hp[r] = s[r]->red_F_dev();
    hp[ranks + r] = s[r]->red_G_dev();
    hp[2 * ranks + r] = s[r]->err_dev();
    hp[3 * ranks + r] = ms ? s[r]->fs2_dev(0) : s[r]->fs_dev(0);
    hp[4 * ranks + r] = ms ? s[r]->fs2_dev(1) : s[r]->fs_dev(1);
  }
  double** dp = nullptr;
  PE_HIP_CHECK(hipMalloc(&dp, sizeof(double*) * 5 * ranks));
  PE_HIP_CHECK(hipMemcpy(dp, hp.data(), sizeof(double*) * 5 * ranks, hipMemcpyHostToDevice));
  hipStream_t s0 = s[0]->stream();

  auto join_all = [&]() {
    for (int r = 0; r < ranks; ++r) PE_HIP_CHECK(hipEventRecord(ev[r], s[r]->stream()));
    for (int r = 1; r < ranks; ++r) PE_HIP_CHECK(hipStreamWaitEvent(s0, ev[r], 0));
  };
  auto fork_all = [&]() {
    PE_HIP_CHECK(hipEventRecord(ev[0], s0));
    for (int r = 1; r < ranks; ++r) PE_HIP_CHECK(hipStreamWaitEvent(s[r]->stream(), ev[0], 0));
  };
  auto reduce = [&](double* const* table, int n, int is_max) {
    join_all();
    dev::launch_group_reduce(table, ranks, n, is_max, s0);
    fork_all();
  };
  // Same halo phases as under RCCL; the transport is a D2D copy from the
  // peer's send region once the peer's stream has produced it.
  auto exchange = [&](int buf, bool after_sweep) {
    // (multi-step sweeps do not store their y strips: packed here)
    if (ms && after_sweep)
      for (int r = 0; r < ranks; ++r) s[r]->enqueue_pack(buf);
    std::vector<std::vector<DeviceSolver::HaloPhase>> plan(ranks);
    for (int r = 0; r < ranks; ++r) plan[r] = s[r]->halo_phases(buf);
    for (size_t ph = 0; ph < plan[0].size(); ++ph) {
      for (int r = 0; r < ranks; ++r) PE_HIP_CHECK(hipEventRecord(ev[r], s[r]->stream()));
      for (int r = 0; r < ranks; ++r)
        for (const auto& e : plan[r][ph].ex) {
          const Exchange* src = nullptr;
          for (const auto& pe : plan[e.peer][ph].ex)
            if (pe.dir == opposite(e.dir)) src = &pe;
          if (!src || src->count != e.count) throw std::runtime_error("group halo plan mismatch");
          PE_HIP_CHECK(hipStreamWaitEvent(s[r]->stream(), ev[e.peer], 0));
          PE_HIP_CHECK(hipMemcpyAsync(e.recv, src->send, sizeof(double) * e.count, hipMemcpyDeviceToDevice,
                                      s[r]->stream()));
        }
      for (int r = 0; r < ranks; ++r)
        if (plan[r][ph].unpack) s[r]->enqueue_unpack(buf);
    }
  };

  for (int r = 0; r < ranks; ++r) s[r]->enqueue_init();
  if (fused) {
    for (int r = 0; r < ranks; ++r) s[r]->enqueue_pack(0);
    exchange(0, false);
    for (int r = 0; r < ranks; ++r) s[r]->enqueue_S(1);
    exchange(1, true);
    reduce(dp + 4 * ranks, nsum, 0);
  } else {
    exchange(0, false);
    reduce(dp + ranks, 1, 0);
  }
  PE_HIP_CHECK(hipStreamSynchronize(s0));
  const bool res_rule = P.stop == Stop::Residual;
  if (res_rule) {  // the threshold from the reduced g_0 into every block's state, each on its own stream
    DevState st0;
    s[0]->read_state(&st0);
    const double g0 = s[0]->stop_g0(st0);
    for (int r = 0; r < ranks; ++r) s[r]->enqueue_stop_threshold(stop_threshold(P, g0), std::sqrt(g0));
  }
  SolveResult res;
  res.t.setup = secs(t_start, clk::now());
  const auto t_loop = clk::now();
  const int64_t cap = P.iter_cap();
  const int chunk = s[0]->chunk();
  DevState hs;
  int64_t k = 0;
  int64_t nsweep = 0;  // launches (parity)
  for (;;) {
    for (int it = 0; it < chunk; it += steps, k += steps, ++nsweep) {
      const int par = int(nsweep & 1);
      if (fused) {
        // (multi-step: the sweep applies min(steps, cap - K) iterations and
        // resolves its predecessor's stop tests itself)
        for (int r = 0; r < ranks; ++r) s[r]->enqueue_S(par);
        exchange(par, true);
        reduce(dp + (3 + par) * ranks, nsum, 0);
        continue;
      }
      for (int r = 0; r < ranks; ++r) s[r]->enqueue_F(par);
      reduce(dp, 2, 0);
      for (int r = 0; r < ranks; ++r) s[r]->enqueue_G(par);
      exchange(0, false);
      reduce(dp + ranks, 1, 0);
    }
    s[0]->read_state(&hs);
    if (hs.done || k >= cap + (ms ? steps : 0)) break;
  }
  for (int r = 0; r < ranks; ++r) s[r]->synchronize();
  res.t.iterate = secs(t_loop, clk::now());
  res.t.gpu = res.t.iterate;
  for (int r = 0; r < ranks; ++r) s[r]->enqueue_wflush();
  if (opt.compute_error) {
    for (int r = 0; r < ranks; ++r) s[r]->enqueue_error();
    reduce(dp + 2 * ranks, 1, 0);
    // max over the two max slots: table entries point at err[0]; offset by one.
    std::vector<double*> hm(ranks);
    for (int r = 0; r < ranks; ++r) hm[r] = s[r]->err_dev() + 1;
    double** dm = nullptr;
    PE_HIP_CHECK(hipMalloc(&dm, sizeof(double*) * ranks));
    PE_HIP_CHECK(hipMemcpy(dm, hm.data(), sizeof(double*) * ranks, hipMemcpyHostToDevice));
    reduce(dm, 2, 1);
    PE_HIP_CHECK(hipStreamSynchronize(s0));
    PE_HIP_CHECK(hipFree(dm));
  }
  // The gradient (DeviceSolver::gradient's phases on every block): w into the
  // plane the layout exchanges, the halo exchange of buffer 0, then every
  // block's kGradField writes its position of the global arrays; Σ, Σ, max of
  // the blocks' res slots through kGroupReduce.
  const bool grad_field = gg.host || df.grad_x;
  double* gbuf = nullptr;  // gx then gy of the global interior, when the host wants them
  if (gg.stats || grad_field) {
    if ((df.grad_x == nullptr) != (df.grad_y == nullptr)) throw std::invalid_argument("grad: gx and gy go together");
    if (df.grad_x && gg.host) throw std::invalid_argument("grad: a host or a device destination, not both");
    const int64_t gny = P.N - 1, gn = (int64_t(P.M) - 1) * gny;
    if (gg.host) PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&gbuf), sizeof(double) * 2 * size_t(gn)));
    std::vector<double*> hg(2 * ranks);
    for (int r = 0; r < ranks; ++r) {
      hg[r] = s[r]->res_dev();
      hg[ranks + r] = s[r]->res_dev() + 2;
    }
    double** dg = nullptr;
    PE_HIP_CHECK(hipMalloc(&dg, sizeof(double*) * 2 * ranks));
    PE_HIP_CHECK(hipMemcpy(dg, hg.data(), sizeof(double*) * 2 * ranks, hipMemcpyHostToDevice));
    if (df.grad_x) {  // the caller's arrays: checked before any launch, ordered with the caller's stream by events
      for (int r = 0; r < ranks; ++r)
        s[r]->check_grad_span(df.grad_x, df.grad_y, df.grad_si, df.grad_sj, blks[r].i0 - 1, blks[r].j0 - 1);
      PE_HIP_CHECK(hipEventRecord(ev[0], df.stream));
      for (int r = 0; r < ranks; ++r) PE_HIP_CHECK(hipStreamWaitEvent(s[r]->stream(), ev[0], 0));
    }
    for (int r = 0; r < ranks; ++r) s[r]->enqueue_grad_stage();
    exchange(0, false);
    for (int r = 0; r < ranks; ++r) {
      if (df.grad_x) s[r]->enqueue_grad(df.grad_x, df.grad_y, df.grad_si, df.grad_sj, blks[r].i0 - 1, blks[r].j0 - 1);
      else if (gbuf) s[r]->enqueue_grad(gbuf, gbuf + gn, gny, 1, blks[r].i0 - 1, blks[r].j0 - 1);
      else s[r]->enqueue_grad(nullptr, nullptr, 0, 0, 0, 0);
    }
    reduce(dg, 2, 0);
    reduce(dg + ranks, 1, 1);
    if (df.grad_x) {  // (reduce() joined every block's stream into s0)
      PE_HIP_CHECK(hipEventRecord(ev[0], s0));
      PE_HIP_CHECK(hipStreamWaitEvent(df.stream, ev[0], 0));
    }
    PE_HIP_CHECK(hipStreamSynchronize(s0));
    PE_HIP_CHECK(hipFree(dg));
  }
  for (int r = 0; r < ranks; ++r) s[r]->synchronize();
  s[0]->read_state(&hs);
  if (gg.stats || grad_field) {
    const double hh = P.h1() * P.h2();
    res.grad.integral = hh * hs.res[0];
    res.grad.energy = hh * hs.res[1];
    res.grad.grad_max = std::sqrt(hs.res[2]);
    if (gg.host) {
      const size_t gn = size_t((int64_t(P.M) - 1) * (int64_t(P.N) - 1));
      gg.host->resize(2 * gn);
      PE_HIP_CHECK(hipMemcpy(gg.host->data(), gbuf, sizeof(double) * 2 * gn, hipMemcpyDeviceToHost));
    }
    if (gbuf) PE_HIP_CHECK(hipFree(gbuf));
  }
  res.iters = hs.iter;
  res.converged = hs.status == 1;
  res.breakdown = hs.status == 2;
  res.nonfinite = hs.status == 4;
  if (hs.status == 5) throw std::runtime_error("single-sweep: boundary partials never arrived (internal error)");
  res.last_diff = hs.last_diff;
  res.zr = hs.rz_cur;
  if (res_rule) {
    res.res_nat0 = hs.err[3];
    res.stop_thr = hs.red_G[1];
    if (res.converged) res.res_nat = std::sqrt(hs.rz_cur);
  }
  if (opt.compute_error) {
    const bool no_exact = (uf.rhs || df.rhs || P.shift != 0.0 || P.reaction) && !(uf.exact || df.exact);
    res.l2_err = no_exact ? -1.0 : std::sqrt(hs.err[0] * P.h1() * P.h2());
    res.max_err = no_exact ? -1.0 : hs.err[1];
    res.max_outside = hs.err[2];
  }
  if (df.w_dst)  // every block into its position of the one global array
    for (int r = 0; r < ranks; ++r)
      s[r]->copy_w_device(df.w_dst, df.w_si, df.w_sj, blks[r].i0 - 1, blks[r].j0 - 1, df.stream);
  if (w_out) {
    const int64_t ny = P.N - 1;
    w_out->assign(size_t((P.M - 1) * ny), 0.0);
    for (int r = 0; r < ranks; ++r) {
      const Block& b = blks[r];
      std::vector<double> tmp(size_t(b.nx * b.ny));
      s[r]->copy_w(tmp.data());
      for (int64_t li = 0; li < b.nx; ++li)
        std::copy(tmp.begin() + li * b.ny, tmp.begin() + (li + 1) * b.ny,
                  w_out->begin() + (b.i0 - 1 + li) * ny + (b.j0 - 1));
    }
  }
  PE_HIP_CHECK(hipFree(dp));
  for (auto& e : ev) PE_HIP_CHECK(hipEventDestroy(e));
  res.backend = "hip-group";
  res.algo = algo_name(fused, steps, false);
  res.Px = pg.Px;
  res.Py = pg.Py;
  res.t.solver = secs(t_start, clk::now());
  return res;
}


double device_apply_group(const Problem& P, const ProcessGrid& pg, const SolveOptions& opt, const OperatorFields& f,
                          bool residual) {
  if (!f.v && !f.v_host) throw std::invalid_argument("field: null array");
  if (f.dst && f.host) throw std::invalid_argument("out: a host or a device destination, not both");
  const int ranks = pg.Px * pg.Py;
  const int64_t gny = int64_t(P.N) - 1, gn = (int64_t(P.M) - 1) * gny;
  if (f.reaction) {
    if (!P.reaction) throw std::invalid_argument("device_apply_group: a reaction field without Problem::reaction");
  } else {
    check_reaction(P, f.reaction_host, "device_apply_group");
  }
  std::vector<std::unique_ptr<DeviceSolver>> s;
  std::vector<Block> blks;
  for (int r = 0; r < ranks; ++r) {
    blks.push_back(decompose(P.M, P.N, pg, r));
    s.push_back(std::make_unique<DeviceSolver>(P, blks.back(), nullptr, opt));
    if (f.reaction) s.back()->set_reaction_device(f.reaction, f.reaction_si, f.reaction_sj, f.reaction_f32, f.stream);
    else if (f.reaction_host) s.back()->set_reaction(block_field(f.reaction_host, P.M, P.N, blks.back(), 1).data());
    if (!residual) continue;
    if (f.rhs) s.back()->set_rhs_device(f.rhs, f.rhs_si, f.rhs_sj, f.rhs_f32, f.stream);
    else if (f.rhs_host) s.back()->set_rhs(block_field(f.rhs_host, P.M, P.N, blks.back(), 0).data());
  }
  hipStream_t s0 = s[0]->stream();
  // staging: the host operand, and the result when only the host wants it
  double* vbuf = nullptr;
  double* obuf = nullptr;
  double** dp = nullptr;
  std::vector<hipEvent_t> ev(size_t(ranks), nullptr);
  double sum = 0.0;
  try {
    const void* v = f.v;
    int64_t si = f.v_si, sj = f.v_sj;
    bool f32 = f.v_f32;
    if (!v) {
      PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&vbuf), sizeof(double) * size_t(gn)));
      PE_HIP_CHECK(hipMemcpyAsync(vbuf, f.v_host, sizeof(double) * size_t(gn), hipMemcpyHostToDevice, s0));
      v = vbuf, si = gny, sj = 1, f32 = false;
    }
    double* dst = f.dst;
    int64_t dsi = f.dst_si, dsj = f.dst_sj;
    if (!dst && f.host) {
      PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&obuf), sizeof(double) * size_t(gn)));
      dst = obuf, dsi = gny, dsj = 1;
    }
    // every refusal before any launch
    for (int r = 0; r < ranks; ++r) s[r]->check_apply_span(v, si, sj, f32, dst, dsi, dsj, blks[r].i0 - 1, blks[r].j0 - 1);
    for (auto& e : ev) PE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    std::vector<double*> hp(static_cast<size_t>(ranks));
    for (int r = 0; r < ranks; ++r) hp[size_t(r)] = s[r]->res_dev();
    PE_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dp), sizeof(double*) * size_t(ranks)));
    PE_HIP_CHECK(hipMemcpyAsync(dp, hp.data(), sizeof(double*) * size_t(ranks), hipMemcpyHostToDevice, s0));
    // s0 waits for the caller; every block's stream waits for s0 (the staged operand, the pointer table)
    PE_HIP_CHECK(hipEventRecord(ev[0], f.stream));
    PE_HIP_CHECK(hipStreamWaitEvent(s0, ev[0], 0));
    PE_HIP_CHECK(hipEventRecord(ev[0], s0));
    for (int r = 1; r < ranks; ++r) PE_HIP_CHECK(hipStreamWaitEvent(s[r]->stream(), ev[0], 0));
    for (int r = 0; r < ranks; ++r)
      s[r]->enqueue_apply(v, si, sj, f32, residual, dst, dsi, dsj, blks[r].i0 - 1, blks[r].j0 - 1);
    for (int r = 1; r < ranks; ++r) {
      PE_HIP_CHECK(hipEventRecord(ev[r], s[r]->stream()));
      PE_HIP_CHECK(hipStreamWaitEvent(s0, ev[r], 0));
    }
    dev::launch_group_reduce(dp, ranks, 1, 0, s0);
    PE_HIP_CHECK(hipGetLastError());
    if (f.dst) {  // (s0 has joined every block's stream)
      PE_HIP_CHECK(hipEventRecord(ev[0], s0));
      PE_HIP_CHECK(hipStreamWaitEvent(f.stream, ev[0], 0));
    }
    DevState hs;
    s[0]->read_state(&hs);  // (synchronizes s0)
    sum = P.h1() * P.h2() * hs.res[0];
    if (f.host) {
      f.host->resize(size_t(gn));
      PE_HIP_CHECK(hipMemcpy(f.host->data(), obuf, sizeof(double) * size_t(gn), hipMemcpyDeviceToHost));
    }
  } catch (...) {
    (void)hipDeviceSynchronize();
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    (void)hipFree(vbuf);
    (void)hipFree(obuf);
    (void)hipFree(dp);
    throw;
  }
  for (auto& e : ev) PE_HIP_CHECK(hipEventDestroy(e));
  PE_HIP_CHECK(hipFree(vbuf));
  PE_HIP_CHECK(hipFree(obuf));
  PE_HIP_CHECK(hipFree(dp));
  return sum;
}

}  // namespace pe
