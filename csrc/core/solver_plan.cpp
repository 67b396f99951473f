// The DeviceSolver's decisions as host arithmetic (pe/solver_plan.hpp): the
// kernel family, iterations per sweep, rows per item, item order, tuning,
// capacities and chunk of a block; the resident kernel's tile geometry; the
// halo-path candidates.  No device, no environment.
#include "pe/solver_plan.hpp"

#include <algorithm>
#include <stdexcept>

#include "pe/fields.hpp"

namespace pe {

// Can the single-sweep kernel run this block?  It needs the fast arithmetic
// variant and neighbours at least two nodes deep in every split direction
// (its halo is two rows / columns deep).
static bool fused_possible(const Problem& P, const Block& b) {
  const int64_t min_rows = (P.M - 1) / b.Px, min_cols = (P.N - 1) / b.Py;
  return (b.Px == 1 || min_rows >= 2) && (b.Py == 1 || min_cols >= 2);
}

std::optional<ResidentTiling> resident_tiling(int64_t nx, int64_t ny, int cus) {
  const int64_t ns = (ny + dev::kFSW - 1) / dev::kFSW;
  if (ns > cus) return std::nullopt;
  const int64_t ntr = std::max<int64_t>(1, std::min<int64_t>(cus / ns, nx / 8));
  if (nx < 2 * ntr) return std::nullopt;
  ResidentTiling t;
  t.nstrips = int(ns);
  t.ntr = int(ntr);
  t.rowstart.resize(size_t(ntr) + 1);
  for (int64_t b = 0; b <= ntr; ++b) t.rowstart[size_t(b)] = 1 + int(b * nx / ntr);
  for (int64_t b = 0; b < ntr; ++b) t.rcap = std::max(t.rcap, t.rowstart[size_t(b) + 1] - t.rowstart[size_t(b)]);
  if (t.rcap > kResTileRows) return std::nullopt;
  return t;
}

SolverPlan plan_solver(const Problem& prob, const Block& blk, int comm_size, const SolveOptions& opt,
                       const SolverKnobs& knobs, int cus) {
  SolverPlan pl;
  if (opt.algo < 0 || opt.algo > 4)
    throw std::invalid_argument("algo: 0 auto, 1 classic, 2 fused, 3 two-step, 4 three-step (got " +
                                std::to_string(opt.algo) + ")");
  // A shifted operator (Problem::shift ≠ 0) runs the classic two-kernel path
  // on every decomposition: the single-sweep, multi-step and resident kernels
  // do not carry the shift, and nothing below may launch one of them.
  check_shift(prob, "DeviceSolver");
  check_stop(prob, "DeviceSolver");
  // A reaction field (Problem::reaction) is planned as a shift is: the same
  // kernels carry it (their FIELD instantiations), and no others.
  if (prob.reaction && prob.shift != 0.0)
    throw std::invalid_argument("DeviceSolver: reaction together with shift != 0 (got " + std::to_string(prob.shift) +
                                "): add the constant to the field");
  if (prob.reaction && opt.algo >= 2)
    throw std::invalid_argument(
        "algo fused / two-step / three-step: the single-sweep kernels implement the operator without a reaction field "
        "only; a problem with reaction runs algo auto or classic");
  const bool shifted = prob.shift != 0.0 || prob.reaction;
  if (shifted && opt.algo >= 2)
    throw std::invalid_argument(
        "algo fused / two-step / three-step: the single-sweep kernels implement the unshifted operator only; a problem "
        "with shift != 0 (got " + std::to_string(prob.shift) + ") runs algo auto or classic");
  const bool can_fuse = !shifted && opt.variant == 0 && fused_possible(prob, blk);
  if (opt.algo >= 2 && !can_fuse)
    throw std::invalid_argument("single-sweep algorithm needs variant 0 and >= 2 rows/columns per split block");
  pl.fused = opt.algo >= 2 || (opt.algo == 0 && can_fuse);
  // Several iterations per sweep (fused2.hip: 2, fused3.hip: 3): single-rank
  // blocks of ≥ 8 × 8 nodes, or row slabs (Py = 1) over a multi-rank
  // transport of ≥ 4s rows per rank (the 2s-deep halo comes from one
  // neighbour and the pushed edge rows are distinct).  Every input is global: every rank
  // decides the same.  algo 3 / 4 force two / three steps; auto takes three
  // where it can (PE_STEPS=1/2/3 caps the iterations per sweep).
  {
    auto single = [&](int64_t m) { return comm_size == 1 && blk.Px * blk.Py == 1 && blk.nx >= m && blk.ny >= m; };
    auto slabs = [&](int64_t m) {
      return comm_size > 1 && blk.Py == 1 && (prob.M - 1) / blk.Px >= m && prob.N - 1 >= m;
    };
    // 2-D splits (three-step only): the 6-deep halo through the comm's
    // exchange — y strips packed after the sweep, then the x rows with their
    // halo columns (corners) — from blocks of >= 12 rows and columns each
    auto grid2d = [&](int64_t m) {
      return comm_size > 1 && blk.Py > 1 && (prob.M - 1) / blk.Px >= m && (prob.N - 1) / blk.Py >= m;
    };
    // virtual ranks on one device (device_solve_group: no comm, a split block;
    // the group driver exchanges the halos and sums the sweeps' sums)
    auto vgroup = [&](int64_t m) {
      return comm_size == 1 && blk.Px * blk.Py > 1 && (prob.M - 1) / blk.Px >= m &&
             (prob.N - 1) / blk.Py >= m;
    };
    const bool two_ok = pl.fused && (single(8) || slabs(8));
    const bool three_ok = pl.fused && (single(8) || slabs(12) || grid2d(12) || vgroup(12));
    if (opt.algo == 3 && !two_ok)
      throw std::invalid_argument("two-step sweep: single-rank blocks of >= 8 x 8 nodes or row slabs of >= 8 rows");
    if (opt.algo == 4 && !three_ok)
      throw std::invalid_argument(
          "three-step sweep: single-rank blocks of >= 8 x 8 nodes, row slabs of >= 12 rows or 2-D blocks of >= 12 x 12");
    // The residual stop rule (Problem::stop) tests an iterate at the top of the
    // next iteration: the one-iteration kernels do (kF, kS / kRed, kResident);
    // the multi-step sweeps do not carry it.  After every other refusal.
    const bool res_rule = prob.stop == Stop::Residual;
    if (res_rule && opt.algo >= 3)
      throw std::invalid_argument(
          "algo two-step / three-step: the multi-step sweeps implement the step-size stop rule only; a problem with "
          "stop = \"residual\" runs algo auto, classic or fused");
    // auto: every single-rank block the LDS-resident kernel cannot hold
    // (1x MI355X, fresh processes, T_solver two-step vs single sweep:
    // 1600×2400 0.110 vs 0.127 s, 2048² 0.113 vs 0.133, 4096² 0.378 vs 0.584,
    // 8192² 2.60 vs 3.24, 16384² 13.7 vs 21.7; the resident kernel keeps
    // ≤ 800×1200: 0.044 vs 0.059 s — profiles/r3_grids_two.txt).  The
    // estimate is setup_resident's geometry test (resident_tiling).
    if (!(knobs.resident && *knobs.resident == 0) && opt.variant == 0) {
      const std::optional<ResidentTiling> t = resident_tiling(blk.nx, blk.ny, cus);
      pl.resident_likely = t && t->ntr * t->nstrips <= kResTiles;
    }
    bool auto_ms = slabs(8) || grid2d(12) || vgroup(12) || !pl.resident_likely;
    int want = 3;
    if (knobs.steps) want = std::max(1, std::min(3, *knobs.steps));
    if (res_rule) want = 1;  // one iteration per launch on every decomposition (PE_STEPS is ignored)
    pl.steps = 1;
    if (opt.algo == 3) pl.steps = 2;
    else if (opt.algo == 4) pl.steps = 3;
    else if (opt.algo == 0 && auto_ms)
      pl.steps = (want >= 3 && three_ok) ? 3 : (want >= 2 && two_ok) ? 2 : 1;
    pl.sstep = pl.steps > 1;
  }

  const int64_t nx = blk.nx, ny = blk.ny;
  int ti = pl.fused ? 16 : 8;  // 8192² sweeps: classic 8 rows, single-sweep 16 (4 halo rows per item)
  const int ti_env = knobs.ti ? *knobs.ti : 0;
  if (ti_env > 0) ti = ti_env;
  pl.geo = sweep_geometry(nx, ny, pl.steps, pl.fused);
  // rows per item and item order first: they select the sweep kernel variant
  // whose occupancy sizes the grid
  const double npts = double(nx) * double(ny);
  const bool big = npts >= double(1 << 24), huge = npts > double(1 << 26);
  // Single-sweep item order and rows per item (profiles/r2_order.txt,
  // profiles/r2_bench_static.txt; one memory placement per comparison):
  //  * blocks > 2²⁶ nodes (16384²): the per-XCD dynamic queue, 18 rows —
  //    with ≈45 items per wave a static layout's per-wave durations drift
  //    apart (2150 vs 2195 µs per iteration static 24 rows);
  //  * 2²⁴ .. 2²⁶ (8192², the 2-rank 8192² block): the cost-aware static LPT
  //    layout, 24 rows, untuned — no item-sum reduction kernel, no queue
  //    atomics, and with 6-12 items per wave its load is even (8192²: 540-542
  //    vs 548 µs dynamic; 2-rank block 315-318 vs 333);
  //  * smaller blocks: static, rows per item tuned below (small blocks: the
  //    queue's pull latency and the reduction launch never pay — 4-rank block
  //    155-159 vs 188 µs, 2400×3200 80 vs 109).
  if (pl.fused && ti_env == 0) ti = huge ? 18 : big ? 24 : 10;
  pl.order = (pl.fused && huge) ? 3 : 0;
  if (pl.sstep) {  // static LPT layout only; taller items (2·hdep pipeline-fill rows each)
    // (three-step beyond 2²⁶ nodes: 128 rows — 16384² 978 vs 999 µs/iteration
    // at 80, one placement, profiles/r3_ti_final.txt)
    if (ti_env == 0) ti = pl.steps >= 3 ? (huge ? 448 : npts >= double(1 << 25) ? 112 : big ? 80 : 48) : (big ? 40 : 24);
    ti = std::max(4, std::min(ti, pl.steps >= 3 ? dev::kTImax3 : dev::kTImax2));
    pl.order = 0;
  }
  if (knobs.order) pl.order = *knobs.order;
  if (!pl.fused && pl.order > 1) pl.order = 0;
  if (pl.sstep) pl.order = 0;
  pl.ti_env = ti_env;
  pl.ti = ti;
  pl.ti_query = (pl.fused && ti_env < 0) ? 1 << 20 : ti;  // bands mode: long items → general kernel
  // Three-step static layout by block size, one placement per block
  // (tools/layout_probe.py, profiles/r4_layout2.txt, µs per iteration): the
  // LPT layout of whole items for ≥ 5·10⁷ nodes (8192²: 253 vs 260 filling,
  // 275 equal-cost), the filling layout from 2.5·10⁷ (the 2-rank 8192² block:
  // 137 vs 145-147), the equal-cost one below (4-rank block 83.4-84.2 vs
  // 87.4-87.9 LPT, 8-rank block 45.1 vs 47.6-49.6); tuned blocks also try the
  // other two at their best rows per item.
  if (pl.steps >= 3) pl.lay_name = npts >= 5e7 ? "lpt" : npts >= 2.5e7 ? "fill" : "equal";
  // Rows per item: fixed (PE_TI, the classic path, blocks ≥ 2²⁴ nodes), or
  // tuned among ti_candidates() for smaller static sweeps.
  pl.tune_ti = pl.fused && ti_env == 0 && pl.order == 0 && npts >= double(1 << 20) && !big;
  // (from 2²⁰ nodes: a tuned layout depends on the timings, so two
  // constructions of a smaller block — a checkpointed solve and its resume —
  // could lay it out differently and the resume would not be bitwise; round 5
  // tuned from 2¹⁷ and test_three_step_checkpoint_resume_bitwise caught it)
  if (pl.sstep) pl.tune_ti = ti_env == 0 && npts >= double(1 << 20) && npts < double(1 << 25);
  if (knobs.ti_tune) pl.tune_ti = pl.tune_ti && *knobs.ti_tune != 0;
  return pl;
}

void finish_plan(SolverPlan& pl, const Block& blk, const DeviceFacts& facts) {
  const int64_t nx = blk.nx, ny = blk.ny, strips = pl.geo.strips;
  const int cus = facts.cus;
  int per_cu = facts.per_cu;
  if (per_cu <= 0) per_cu = 4;
  int wave_cap = cus * per_cu * dev::kWPB;
  // PE_TI=-1 (single-sweep): "bands" — one item per resident wave, the rows
  // split into wave_cap/nstrips bands that the waves of a band march down
  // together (halo rows re-read once per band, perfect balance).
  if (pl.fused && pl.ti_env < 0) {
    const int64_t bands = std::max<int64_t>(1, wave_cap / std::max<int64_t>(1, strips));
    pl.ti = int((nx + bands - 1) / bands);
  }
  int wave_cap0 = wave_cap;
  if (pl.fused && facts.per_cu0 > 0) wave_cap0 = cus * facts.per_cu0 * dev::kWPB;
  pl.wave_caps[0] = wave_cap;
  pl.wave_caps[1] = wave_cap0;
  pl.ti_cands.clear();
  if (pl.tune_ti) pl.ti_cands = ti_candidates(pl.geo, nx, ny, std::min(wave_cap, wave_cap0));
  pl.ti_min = pl.tune_ti ? pl.ti_cands.front() : pl.ti;
  // block partials: interior grid, then (overlap) the boundary grid after it
  pl.npart = 8 * std::max<int64_t>(2 * int64_t(std::max(wave_cap, wave_cap0) / dev::kWPB + 1), 4096);
  // item-sum slots: one per item (static sweeps split heavy items into up to
  // ti pieces: the planner)
  pl.nitems_max = strips * ((nx + pl.ti_min - 1) / pl.ti_min);
  pl.nslot_cap = pl.fused ? int((pl.order == 0 ? pl.ti + 1 : 2) * pl.nitems_max + 64) : 0;
}

ChunkPlan plan_chunk(const SolverPlan& pl, const Block& blk, int comm_size, int opt_chunk, bool resident) {
  // Iterations per host check: aim for ~0.5 ms of device work per chunk.
  const double pts = double(blk.nx) * double(blk.ny);
  const double t_iter = pts * (pl.sstep ? 48.0 / pl.steps : pl.fused ? 48.0 : 64.0) / 4.5e12 + 6e-6 + (comm_size > 1 ? 40e-6 : 0.0);
  int c = int(0.5e-3 / t_iter);
  c = std::max(8, std::min(128, c));
  c += c & 1;
  if (pl.sstep) c = (c + 2 * pl.steps - 1) / (2 * pl.steps) * (2 * pl.steps);  // whole sweeps, an even number of them (graph parity)
  ChunkPlan out;
  out.stream_chunk = opt_chunk > 0 ? (opt_chunk + (opt_chunk & 1)) : c;
  if (resident) c = 512;  // one launch per chunk (≈ 5 ms of iterations at 800×1200)
  out.chunk = opt_chunk > 0 ? (opt_chunk + (opt_chunk & 1)) : c;
  if (pl.sstep) {
    out.chunk = (out.chunk + 2 * pl.steps - 1) / (2 * pl.steps) * (2 * pl.steps);
    out.stream_chunk = out.chunk;
  }
  return out;
}

std::string algo_name(bool fused, int steps, bool resident) {
  return resident ? "resident" : steps == 3 ? "three-step" : steps == 2 ? "two-step" : fused ? "fused" : "classic";
}

HaloCandidates halo_candidates(const HaloInputs& in) {
  HaloCandidates out;
  std::vector<HaloCandidate>& cands = out.list;
  const std::optional<std::string>& hm = in.halo;
  const std::optional<int>& ov = in.overlap;
  // (the two-step sweep has no boundary-item signal; every rank decides this
  // from global inputs — a rank without neighbours still takes part, its
  // overlap is simply off in apply_layout)
  const bool ov_able = in.steps != 2;
  // The overlapped candidates run at each of the rows-per-item tuning's three
  // best heights (its boundary-first layout ranks them differently); with the
  // exchange among the candidates the put's overlap runs only at the height
  // the exchange's overlap timed best (the halo path does not move that rank).
  std::vector<int> heights = in.heights;
  heights.resize(size_t(std::max(1, in.nheights)));
  auto add = [&](const char* path, bool o) {
    if (o && !ov_able) return;
    if (ov && (*ov != 0) != o) return;
    if (!o) {
      cands.push_back(HaloCandidate{path, o, 0});
      return;
    }
    for (int h : heights) cands.push_back(HaloCandidate{path, o, h});
  };
  // (the plain-layout candidates first, then the overlapped ones, height by height)
  const bool ex_ok = !hm || *hm == "exchange";
  if (ex_ok) add("exchange", false);
  if (in.put_ok) add("put", false);
  if (in.push_ok && !(ov && *ov != 0)) cands.push_back(HaloCandidate{"push", false, 0});
  if (ex_ok) add("exchange", true);
  // (not when ranks share a GPU — test jobs: put blocks spinning on the halo
  // stream under another process's persistent sweep can starve it of CUs; a
  // 6-process 2×3 job on one GPU stalled past 3 minutes, round 6)
  const bool put_ov_forced = hm && *hm == "put" && ov && *ov != 0;
  const bool put_ov = in.put_ok && (!in.shared_dev || put_ov_forced) && ov_able && !(ov && *ov == 0);
  out.put_ov_late = put_ov && ex_ok && !cands.empty() && cands.back().overlap;  // (after the exchange's heights)
  if (put_ov && !out.put_ov_late) add("put", true);
  if (cands.empty()) {  // (the forced path is not available here: the exchange, at every height when overlapped)
    if (ov && *ov != 0 && ov_able) {
      for (int h : heights) cands.push_back(HaloCandidate{"exchange", true, h});
    } else {
      cands.push_back(HaloCandidate{"exchange", false, 0});
    }
  }
  return out;
}

}  // namespace pe
