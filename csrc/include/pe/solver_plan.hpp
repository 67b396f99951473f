// Host-only plan of a DeviceSolver: which kernel family a block gets, the
// iterations per sweep, rows per item and item order, whether the heights are
// tuned, the starting static layout, the buffer capacities and the chunk
// length; the LDS-resident kernel's tile geometry; the halo-path candidate
// list.  Pure arithmetic over the problem, the block, the options, the parsed
// PE_* knobs and a few device facts: no device, no environment.  The item
// lists themselves are the planner's (pe/item_layout.hpp).
#pragma once

#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "pe/decomp.hpp"
#include "pe/item_layout.hpp"
#include "pe/problem.hpp"
#include "pe/solver.hpp"

namespace pe {

// The parsed values of the PE_* knobs the plan reads (std::atoi of the
// variable); an empty optional: the variable is unset.
struct SolverKnobs {
  std::optional<int> resident;  // PE_RESIDENT: 0 switches the LDS-resident kernel off
  std::optional<int> steps;     // PE_STEPS: caps the iterations per sweep (1 / 2 / 3)
  std::optional<int> ti;        // PE_TI: rows per item (> 0), the bands mode (< 0)
  std::optional<int> order;     // PE_ORDER: item order
  std::optional<int> ti_tune;   // PE_TI_TUNE: 0 keeps the untuned rows per item
};

// What the plan needs to know of the device.  per_cu: resident 256-thread
// blocks per CU of the applying sweep (the classic kernels on that path),
// per_cu0: of the deferring sweep; <= 0: the occupancy API gave nothing.
struct DeviceFacts {
  int cus = 256;
  int per_cu = 0, per_cu0 = 0;
};

// LDS-resident tile geometry (resident.hip): tiles of one 124-column strip × R
// rows, one workgroup each, at most one per CU, R >= 8 where the block allows
// and <= kResTileRows.
constexpr int kResTileRows = 64;  // (dev::kResMaxRows)
constexpr int kResTiles = 256;    // (dev::kResMaxTiles: the kernel's sum gather covers 256 tiles)
struct ResidentTiling {
  int nstrips = 0, ntr = 0;   // strips across, row bands down: ntr × nstrips tiles
  std::vector<int> rowstart;  // ntr + 1: first local row of band t (rowstart[ntr] = nx + 1)
  int rcap = 0;               // rows of the tallest band
};
// The tiling of an nx × ny block on `cus` compute units, or nothing when the
// geometry refuses the block.  (PE_RESIDENT, the variant and the kernel's
// other limits — band table, LDS bytes, occupancy, kResTiles — are the callers'.)
std::optional<ResidentTiling> resident_tiling(int64_t nx, int64_t ny, int cus);

struct SolverPlan {
  // ---- stage one (plan_solver): from the CU count alone
  bool fused = false;   // a single-sweep kernel (else the classic two-kernel iteration)
  bool sstep = false;   // several iterations per sweep
  int steps = 1;        // iterations per sweep launch (1, 2, 3)
  bool resident_likely = false;  // the estimate of setup_resident's geometry test
  int ti_env = 0;       // PE_TI (0: unset)
  int ti = 8;           // rows per item
  int ti_query = 8;     // KParams::ti while the occupancy is asked (the bands mode: long items → general kernel)
  int order = 0;        // item order (KParams::order)
  std::string lay_name = "lpt";  // starting three-step static layout: lpt / fill / equal
  SweepGeometry geo;
  // ---- stage two (finish_plan): from the occupancy of the sweep stage one selected
  int wave_caps[2] = {0, 0};  // resident waves of the applying / deferring sweep
  bool tune_ti = false;       // rows per item chosen by timing candidate sweeps
  std::vector<int> ti_cands;  // the candidates (tune_ti)
  int ti_min = 8;             // the smallest height the item-sum slots must hold
  int64_t npart = 0;          // block partials (doubles)
  int64_t nitems_max = 0;
  int nslot_cap = 0;          // item-sum slots
};

// Stage one.  Refuses (std::invalid_argument) what no kernel runs, in this
// order: the algo range, the shift (check_shift), a shift with algo >= 2, the
// single-sweep precondition, the two-step and the three-step preconditions,
// and last the residual stop rule with algo two-step / three-step (the stop
// fields themselves, check_stop, right after the shift).  Under that rule
// algo auto plans one iteration per launch, as PE_STEPS=1 does.
SolverPlan plan_solver(const Problem& prob, const Block& blk, int comm_size, const SolveOptions& opt,
                       const SolverKnobs& knobs, int cus);
// Stage two: `facts` are the occupancy figures asked with plan.ti_query / plan.order.
void finish_plan(SolverPlan& plan, const Block& blk, const DeviceFacts& facts);

// Iterations per host check (`chunk`; `stream_chunk`: of the streaming sweep
// after a resident fallback) once it is known whether the resident kernel runs.
struct ChunkPlan {
  int chunk = 16, stream_chunk = 16;
};
ChunkPlan plan_chunk(const SolverPlan& plan, const Block& blk, int comm_size, int opt_chunk, bool resident);

// SolveResult::algo
std::string algo_name(bool fused, int steps, bool resident);

// ---- the halo-path candidates (DeviceSolver::choose_halo_path)
struct HaloInputs {
  int steps = 1;            // iterations per sweep (the two-step sweep has no boundary-item signal)
  bool put_ok = false, push_ok = false;  // the put / the push set up on every rank
  bool shared_dev = false;  // another rank of the job runs on this rank's GPU
  int nheights = 1;         // heights every rank times the overlap at (agreed: the max over ranks)
  std::vector<int> heights; // this rank's heights (the tuning's best; 0: the construction's)
  std::optional<std::string> halo;  // PE_HALO
  std::optional<int> overlap;       // PE_OVERLAP
};
struct HaloCandidate {
  std::string path;  // exchange / put / push
  bool overlap;
  int ti;            // rows per item (0: the construction's)
};
struct HaloCandidates {
  std::vector<HaloCandidate> list;  // in timing order
  bool put_ov_late = false;         // the put's overlap is timed after the list, at the exchange overlap's best height
};
// Every rank must build the same list (each timing ends in a collective):
// a function of its inputs only.
HaloCandidates halo_candidates(const HaloInputs& in);

}  // namespace pe
