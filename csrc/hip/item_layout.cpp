// The solver's side of the item layout: the host planner's list uploaded and
// handed to the kernels (apply_layout / prepare_layout), the rows-per-item
// tuning (tune_rows_per_item) and the LDS-resident kernel's tiles (setup_resident).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "../hip/kernels.hpp"
#include "env_knobs.hpp"
#include "pe/device.hpp"
#include "solver_internal.hpp"

namespace pe {

using detail::clk;
using detail::Range;
using detail::secs;
using dev::KParams;

static_assert(sizeof(Entry) == sizeof(int2) && offsetof(Entry, x) == offsetof(int2, x) && offsetof(Entry, y) == offsetof(int2, y),
              "the planner's list entries are uploaded as the kernels' int2");

// The planner's layout at `ti` rows per item for the solver's occupancy figures
// and the PE_* layout knobs, read from the environment at every call (*asked:
// that request) — from the cache while the rows per item are tuned and the halo
// path is chosen (their candidates come back to layouts already built: 0.3-2.6
// ms of host work each).
// Halo/interior overlap: the construction's choice (choose_halo_path times
// the exchange with and without it on the job's transport; PE_OVERLAP=1 / 0
// restricts the choice).  Only where the sweep can signal its boundary items
// (single sweep; the three-step sweep's kSignal variant, fused3.hip — not
// the two-step sweep) and the halo is exchanged, not pushed.
ItemLayout DeviceSolver::plan_layout(int ti, bool want_overlap, bool push, LayoutRequest* asked) {
  const bool nb = blk_.has(LEFT) || blk_.has(RIGHT) || blk_.has(DOWN) || blk_.has(UP);
  const bool overlap = want_overlap && fused_ && (!sstep_ || steps_ >= 3) && comm_->size() > 1 && nb && !push;
  LayoutRequest rq{ti, kp_->order, overlap, lay_name_, {plan_.wave_caps[0], plan_.wave_caps[1]},
                   std::min(plan_.wave_caps[0], plan_.wave_caps[1]),
                   cus_, 8, nslot_cap_, read_env_knobs().layout};
  if (asked) *asked = rq;
  if (!lay_cache_on_) return planner_->build(rq);
  const auto key = std::make_tuple(ti, overlap, lay_name_);
  auto it = lay_cache_.find(key);
  if (it == lay_cache_.end()) it = lay_cache_.emplace(key, planner_->build(rq)).first;
  return it->second;
}

// Lays out (ti, overlap) into the cache, host work only: the halo-path choice builds its next
// candidates' layouts while the GPU times the current one.  (The overlap's list: the push never overlaps.)
void DeviceSolver::prepare_layout(int ti, bool overlap) {
  if (fused_ && lay_cache_on_) (void)plan_layout(ti, overlap, false, nullptr);
}

// Item lists at `ti` rows per item for the current halo path: static layout
// or dynamic per-XCD shards, boundary items first under the overlap.
void DeviceSolver::apply_layout(int ti) {
  KParams& k = *kp_;
  LayoutRequest asked;
  ItemLayout next = plan_layout(ti, want_overlap_, push_, &asked);
  overlap_ = asked.overlap;
  k.ti = ti;
  k.nitems = next.nitems;
  k.nblocks = next.nblocks;
  k.nblocks0 = next.nblocks0;
  k.nslots = next.nslots;
  if (next.list.empty()) return;  // (a walk without a list)
  if (!next.static_waves) next.name = lay_.name;
  const auto tc = clk::now();
  // (re-laid out by the rows-per-item tuning: the list buffer is reused while
  // it is large enough — a free per candidate synchronised the device)
  if (next.list.size() > ilist_cap_) {
    // (the rows-per-item tuning lays out while the previous candidate's
    // sweeps, which read the old list, may still run)
    PE_HIP_CHECK(hipStreamSynchronize(stream_));
    if (ilist_) PE_HIP_CHECK(hipFree(ilist_));
    ilist_cap_ = std::max(next.list.size(), ilist_cap_ + ilist_cap_ / 2);
    PE_HIP_CHECK(hipMalloc(&ilist_, sizeof(int2) * ilist_cap_));
  }
  upload(ilist_, next.list.data(), sizeof(int2) * next.list.size());
  copy_setup_s_ += secs(tc, clk::now());
  nslot_cap_ = std::max<int>(nslot_cap_, int(next.list.size()));
  lay_ = std::move(next);
  lay_req_ = asked;
  // Every listed sweep walks the list (the plain one counts no boundary
  // items: lnb = 0; the overlapped iteration's launch carries lay_.lnb).
  k.ilist = ilist_;
  k.lnsh = lay_.lnsh;
  k.lwaves = lay_.lwaves;
  for (int x = 0; x <= 8; ++x) k.lbase[x] = lay_.lbase[x];
  for (int x = 0; x < 8; ++x) k.lnb[x] = 0;
  if (overlap_) create_halo_stream();
}

// Rows per item by timing: S_0 + 1 + kTimed local sweeps per candidate on
// real data (no communication: the in-sweep cross-rank sum is not set up yet),
// the fastest kept; every rank tunes its own block.
void DeviceSolver::tune_rows_per_item(const std::vector<int>& cands, int ti) {
  Range range("pe.tune_rows_per_item");
  const EnvKnobs env = read_env_knobs();
  const bool ctor_trace = env.ctor_trace >= 1;
  float best_ms = 0.f;
  int best = ti;
  // one candidate: S_0 + 1 + kTimed local sweeps on real data, the last
  // kTimed timed (round 3: S_0 + 2 + 6 — construction is inside T_solver)
  constexpr int kTimed = 4;
  // Trials run pipelined: the host lays out trial i+1 while the GPU times
  // trial i (the list upload is stream-ordered after those sweeps), and
  // layouts already built come from the cache (the finalists, the final
  // one).  The host layouts were ≈ half of the tuning's time (4096²: 1-2.4
  // ms each against 1.7-2 ms of timing, PE_CTOR_TRACE=3,
  // profiles/r6_ctor_tuning.txt).
  struct Trial {
    int ti;
    std::string lay;
  };
  lay_cache_.clear();
  lay_cache_on_ = true;
  auto run_trials = [&](const std::vector<Trial>& trials) {
    std::vector<float> out;
    for (size_t i = 0; i <= trials.size(); ++i) {
      const auto tl = clk::now();
      if (i < trials.size()) {
        lay_name_ = trials[i].lay;
        apply_layout(trials[i].ti);  // (its upload waits for trial i-1's sweeps)
      }
      const auto tg = clk::now();
      if (i > 0) {
        PE_HIP_CHECK(hipEventSynchronize(t1_));
        float ms = 0.f;
        PE_HIP_CHECK(hipEventElapsedTime(&ms, t0_, t1_));
        out.push_back(ms);
        if (ctor_trace)
          std::fprintf(stderr, "[pe] ctor   tune %3d rows %-5s %8.4f ms per sweep\n", trials[i - 1].ti,
                       trials[i - 1].lay.c_str(), ms / float(kTimed));
      }
      if (i == trials.size()) break;
      enqueue_init();
      dev::launch_S(*kp_, 1, stream_);
      dev::launch_S(*kp_, 0, stream_);
      PE_HIP_CHECK(hipEventRecord(t0_, stream_));
      for (int j = 0; j < kTimed; ++j) dev::launch_S(*kp_, (j + 1) & 1, stream_);
      PE_HIP_CHECK(hipEventRecord(t1_, stream_));
      if (ctor_trace)
        std::fprintf(stderr, "[pe] ctor   tune %3d rows %-5s layout %7.3f ms\n", trials[i].ti, trials[i].lay.c_str(),
                     1e3 * secs(tl, tg));
    }
    return out;
  };
  {
    std::vector<Trial> tr;
    for (int cand : cands) tr.push_back(Trial{cand, lay_name_});
    const std::vector<float> ms = run_trials(tr);
    for (size_t i = 0; i < tr.size(); ++i) {
      ti_ms_.push_back(ms[i] / float(kTimed));
      ti_rows_.push_back(tr[i].ti);
      if (best_ms == 0.f || ms[i] < best_ms) {
        best_ms = ms[i];
        best = tr[i].ti;
      }
    }
  }
  // three-step: the other static layouts at the best height
  std::string keep = lay_name_;
  struct Tried {
    int ti;
    std::string lay;
    float ms;
  };
  std::vector<Tried> tried;
  for (size_t i = 0; i < ti_rows_.size(); ++i) tried.push_back(Tried{ti_rows_[i], lay_name_, ti_ms_[i] * float(kTimed)});
  if (steps_ >= 3 && env.layout.force_layout.empty()) {  // (PE_LAYOUT unset)
    const std::string base = lay_name_;
    std::vector<Trial> tr;
    for (const char* alt : {"equal", "fill", "lpt"})
      if (base != alt) tr.push_back(Trial{best, alt});
    const std::vector<float> ms = run_trials(tr);
    for (size_t i = 0; i < tr.size(); ++i) {
      ti_ms_.push_back(ms[i] / float(kTimed));
      ti_rows_.push_back(-best);  // (negative: a layout candidate at that height)
      tried.push_back(Tried{best, tr[i].lay, ms[i]});
      if (ms[i] < best_ms) {
        best_ms = ms[i];
        keep = tr[i].lay;
      }
    }
  }
  // Finalists: the two fastest candidates timed once more, each keeping its
  // faster timing — the GPU clock ramps up during construction, so the first
  // candidates were timed slow, and two within ≈2 % swapped places from one
  // process to the next (2400×3200: equal layout at 80 rows or filling at
  // 96, T_iterate 0.099 vs 0.095 s, profiles/r5_prio.txt).  Three-step only.
  if (steps_ >= 3 && tried.size() >= 2) {
    std::stable_sort(tried.begin(), tried.end(), [](const Tried& a, const Tried& b) { return a.ms < b.ms; });
    const std::vector<float> ms = run_trials({Trial{tried[0].ti, tried[0].lay}, Trial{tried[1].ti, tried[1].lay}});
    for (int f = 0; f < 2; ++f) {
      Tried& t = tried[size_t(f)];
      ti_ms_.push_back(ms[size_t(f)] / float(kTimed));
      ti_rows_.push_back(t.lay == keep && t.ti == best ? best : -t.ti);
      t.ms = std::min(t.ms, ms[size_t(f)]);
    }
    const Tried& w = tried[0].ms <= tried[1].ms ? tried[0] : tried[1];
    best = w.ti;
    keep = w.lay;
  }
  // the three best heights (any layout), for the overlap's own layout: its
  // boundary-first filling list ranks them differently (8-rank slab of
  // 8192²: 64, 80 and 96 rows tie within 1 % on the plain layout, 117-119 µs
  // per sweep, but the overlapped sweep runs 146, 157 and 128 µs —
  // profiles/r6_overlap_ti.txt)
  std::stable_sort(tried.begin(), tried.end(), [](const Tried& a, const Tried& b) { return a.ms < b.ms; });
  ti_alt_ = {best};
  for (const Tried& t : tried)
    if (ti_alt_.size() < 3 && std::find(ti_alt_.begin(), ti_alt_.end(), t.ti) == ti_alt_.end()) ti_alt_.push_back(t.ti);
  lay_name_ = keep;
  apply_layout(best);
  lay_cache_on_ = false;
  lay_cache_.clear();
}

static_assert(kResTileRows == dev::kResMaxRows && kResTiles == dev::kResMaxTiles,
              "the plan's resident geometry (pe/solver_plan.hpp) uses the kernel's limits");

// LDS-resident geometry: the plan's tiling (resident_tiling: tiles of one
// 124-column strip × R rows — the streaming sweep's strips — one workgroup
// each, at most one per CU, R ≥ 8 where the block allows and ≤ kResMaxRows);
// the band-coefficient table is sized from the host row classes (the kernel's
// exact band test).
void DeviceSolver::setup_resident() {
  KParams& k = *kp_;
  resident_ = false;
  const EnvKnobs env = read_env_knobs();
  if (env.plan.resident && *env.plan.resident == 0) return;
  if (!fused_ || sstep_ || comm_->size() != 1 || blk_.Px * blk_.Py != 1 || overlap_ || k.stamps || opt_.variant != 0)
    return;
  const int cus = cus_;
  const std::optional<ResidentTiling> tiling = resident_tiling(blk_.nx, blk_.ny, cus);
  if (!tiling) return;
  const int nstrips = tiling->nstrips, ntr = tiling->ntr, rcap = tiling->rcap;
  const std::vector<int>& rs = tiling->rowstart;
  // band nodes per tile region (rows I0-2 .. I0+R+1, columns J0-2 .. J0+125)
  const int64_t rows_tab = int64_t(rowcls_host_.size() / 4);
  int nb_max = 0;
  for (int t = 0; t < ntr; ++t)
    for (int sx = 0; sx < nstrips; ++sx) {
      int nb = 0;
      const int J0 = 1 + dev::kFSW * sx;
      for (int q = rs[size_t(t)] - 2; q < rs[size_t(t) + 1] + 2; ++q) {
        if (q + 1 < 0 || q + 1 >= rows_tab) continue;
        const int* r = &rowcls_host_[size_t(q - geo_.tab_lo) * 4];
        for (int c = J0 - 2; c < J0 + 126; ++c)
          if (c >= r[2] && c <= r[3] && !(c >= r[0] && c <= r[1])) ++nb;
      }
      nb_max = std::max(nb_max, nb);
    }
  const int nbcap = nb_max + 8;
  const size_t lds = dev::resident_lds_bytes(rcap, nbcap);
  if (lds > 163840) return;
  const int per_cu = dev::resident_max_blocks_per_cu(lds, k.stop_res != 0);
  const int nwg = ntr * nstrips;
  if (per_cu < 1 || nwg > per_cu * cus) return;
  if (nwg > dev::kResMaxTiles) return;  // the kernel's sum gather covers 256 tiles (parts with > 256 CUs)
  rp_ = std::make_unique<dev::ResParams>();
  dev::ResParams& r = *rp_;
  std::memset(&r, 0, sizeof(r));
  r.nstrips = nstrips;
  r.ntr = ntr;
  r.nwg = nwg;
  r.rcap = rcap;
  r.nbcap = nbcap;
  r.lds_bytes = unsigned(lds);
  r.timeout_ticks = 200000000LL;  // 2 s per barrier wait
  if (env.res_timeout_s) r.timeout_ticks = (long long)(*env.res_timeout_s * 1e8);
  PE_HIP_CHECK(hipMalloc(&res_rowstart_, sizeof(int) * rs.size()));
  upload(res_rowstart_, rs.data(), sizeof(int) * rs.size());
  const size_t nedge = size_t(2) * size_t(nwg) * dev::kResEdge, npart = size_t(2) * size_t(nwg) * 8;
  PE_HIP_CHECK(hipMalloc(&res_buf_, sizeof(double) * (nedge + npart)));
  // stream-ordered: a null-stream operation would create that stream's
  // hardware queue (≈10 ms inside T_solver in a fresh process, profiles/r2_ctor_phases.txt)
  PE_HIP_CHECK(hipMemsetAsync(res_buf_, 0, sizeof(double) * (nedge + npart), stream_));
  PE_HIP_CHECK(hipMalloc(&res_ctr_, sizeof(unsigned) * 8 * 32));
  if (env.res_stamps) {
    nstamps_ = size_t(nwg) * dev::kResStampIters * 8;
    PE_HIP_CHECK(hipMalloc(&stamps_, sizeof(unsigned long long) * nstamps_));
    PE_HIP_CHECK(hipMemsetAsync(stamps_, 0, sizeof(unsigned long long) * nstamps_, stream_));
    r.stamps = stamps_;
  }
  r.rowstart = res_rowstart_;
  r.edges = res_buf_;
  r.partials = res_buf_ + nedge;
  r.ctr = res_ctr_;
  r.fault_wg = -1;
  r.fault_late = 0;
  if (env.fault.resbarrier || env.fault.reslate) {
    r.fault_wg = nwg - 1;
    r.fault_late = env.fault.reslate ? 1 : 0;
  }
  resident_ = true;
}

}  // namespace pe
