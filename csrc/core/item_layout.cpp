// Host-only item-layout planner (pe/item_layout.hpp): sweep geometry,
// rows-per-item candidates and the four list layouts — dynamic per-XCD shards,
// LPT, filling and equal-cost — over one shared context.
#include "pe/item_layout.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <queue>
#include <stdexcept>

namespace pe {

SweepGeometry sweep_geometry(int64_t nx, int64_t ny, int steps, bool fused) {
  SweepGeometry g;
  g.fused = fused;
  g.steps = steps;
  g.rows_hi = nx + 2;
  g.cols_hi = ny + 2;
  if (!fused) {
    g.strips = (ny + dev::kSW - 1) / dev::kSW;
    return g;
  }
  // Planes: columns -1 .. 124·nstrips+2 (strip loads never leave the row),
  // rows -1 .. nx+4 (two prefetch rows past the halo).  x[b] interleaves the
  // r and p planes by row.  Two-step sweep: halo depth 4 — columns -3 ..
  // 120·nstrips+4, rows -3 .. nx+6.
  g.fsw = steps >= 3 ? dev::kFSW3 : steps == 2 ? dev::kFSW2 : dev::kFSW;
  g.hdep = 2 * steps;
  g.xorg = steps >= 3 ? dev::kHL3 - 1 : g.hdep - 1;
  g.strips = (ny + g.fsw - 1) / g.fsw;
  g.plane = ((g.fsw * g.strips + 2 * g.hdep + 7) / 8) * 8;
  // Three-step: strip s loads columns 48s-7 .. 48s+56 (one per lane) and
  // outputs 48s+1 .. 48s+48.  Element 0 of a row is column -7 and the
  // plane a whole number of 128-B lines, so every strip's loads are 4 whole
  // lines and its stores 6 whole 64-B segments of r, p and w (52 outputs of
  // 64 loaded straddled 64-B segments: partial writes from two strips, and
  // 5 lines touched for 4 lines of data).
  if (steps >= 3) g.plane = ((g.xorg + g.fsw * (g.strips - 1) + 64 - dev::kHL3 + 1 + 15) / 16) * 16;
  const int64_t rows = nx + 2 * g.hdep + 2;
  g.xsize = ((rows * 2 * g.plane + 64 + 31) / 32) * 32;
  g.wsize = ((rows * g.plane + 64 + 31) / 32) * 32;
  // (multi-step: rows -hdep .. nx+hdep+2, columns -hdep .. fsw·strips+hdep+3)
  const bool sstep = steps > 1;
  g.rows_hi = sstep ? nx + g.hdep + 2 : nx + 3;
  g.cols_hi = sstep ? g.fsw * g.strips + g.hdep + 3 : dev::kFSW * g.strips + 3;
  g.tab_lo = sstep ? -g.hdep : -1;
  if (steps >= 3) {  // the last strip's last lane + 3; the first strip's lane 0 is column -xorg
    g.cols_hi = g.fsw * (g.strips - 1) + 64 - dev::kHL3 + 3;
    g.tab_lo = -(g.xorg + 1);
  }
  return g;
}

// Single sweep: tuned among kTiCands (the best depends on the block:
// 2400×3200 18 rows 76 µs vs 84 at 10; 1600×2400 and the 8-rank 8192² block 10
// rows — profiles/r2_mid_tune.txt).
// Two-step sweep: tuned among {16, 24, 32, 40, 48} below 2²⁵ nodes (the
// best height moves with the block: 1600×2400 16 rows 39.9 µs/iter vs 47.7
// at 40, 2048² 24 rows, 4096² 32 rows 102.3 vs 108.7; 8192² and 16384²
// within ±2 % over 24-48 rows: fixed 40 — one placement per grid,
// tools/ti_probe.py, profiles/r3_ti_probe.txt).  Three-step sweep (12
// pipeline-fill rows per item): among {32 .. 96} (2400×3200 32 rows 45.7
// µs/iter vs 57.1 at 64, 1600×2400 and 2048² 48, 4096² 64); fixed above,
// with the aligned 48-column strips: 8192² 112 rows (240-247 µs/iter vs
// 253-256 at 80, 266-271 at 104, 249 at 120, 255 at 128 — the same on two
// boxes and with padded rows; a scan of 64-224 found only 132 as good),
// 16384² 448 (867 vs 880 at 272, 891-899 at 256, 975 at 288, 934-940 at
// 512; 256 was 939 vs 959 at 128 on another box) — tools/layout_probe.py,
// tools/block_probe.py, profiles/r4_ti48.txt.
//
// Candidates: the fixed set plus, for q = 2..5 items per wave, the
// smallest item height that gives every wave at most q items — a static
// layout's sweep lasts as long as its most loaded wave, and 3.4 items per
// wave means a quarter of the waves runs a 4th item while the rest idle
// (8-rank 8192² block at 10 rows: busy fraction 0.74-0.78,
// tools/stamp_probe.py).  (Round 5 measured one short item per wave — down
// to 4 rows — on the 2-rank blocks of 1600×2400 and 2048²: 86.9-88.2 µs per
// sweep against 58.9-64 at 32-96 rows; the 12 pipeline-fill rows of a short
// item cost more than the waves it adds — profiles/r5_ab_layout.txt.)
std::vector<int> ti_candidates(const SweepGeometry& g, int64_t nx, int64_t ny, int wave_cap) {
  static constexpr int kTiCands[4] = {8, 10, 14, 18};
  static constexpr int kTiCands2[5] = {16, 24, 32, 40, 48};
  static constexpr int kTiCands3[5] = {32, 48, 64, 80, 96};
  const bool sstep = g.steps > 1;
  const int* tic = g.steps >= 3 ? kTiCands3 : kTiCands2;
  const double npts = double(nx) * double(ny);
  std::vector<int> ti_cands(kTiCands, kTiCands + 4);
  if (sstep) ti_cands.assign(tic, tic + 5);
  // taller items for the largest tuned blocks (4096²: 30 rows 158 µs vs 165
  // at 18, one placement, profiles/r2_ti_big.txt)
  if (npts >= 12e6 && !sstep) ti_cands.insert(ti_cands.end(), {24, 30});
  const int64_t W = std::max(dev::kWPB, wave_cap);
  const int tlo = sstep ? tic[0] : kTiCands[0], thi = g.steps >= 3 ? 128 : sstep ? dev::kTImax2 : 40;
  for (int q = 2; q <= 5; ++q)
    for (int t = tlo; t <= thi; ++t)
      if (int64_t(g.strips) * ((nx + t - 1) / t) <= int64_t(q) * W) {
        ti_cands.push_back(t);
        break;
      }
  std::sort(ti_cands.begin(), ti_cands.end());
  ti_cands.erase(std::unique(ti_cands.begin(), ti_cands.end()), ti_cands.end());
  return ti_cands;
}

LayoutPlanner::LayoutPlanner(const SweepGeometry& g, int64_t nx, int64_t ny, const bool has[4], std::vector<int> rowcls)
    : g_(g), nx_(nx), ny_(ny), rowcls_(std::move(rowcls)) {
  for (int d = 0; d < 4; ++d) has_[d] = has[d];
}

namespace {
enum { LEFT = 0, RIGHT = 1, DOWN = 2, UP = 3 };
using clk = std::chrono::steady_clock;

struct Piece {
  int64_t ib, rows;
  int s;
  double cost;
  bool bnd;
};
const double overhead = 3.0;  // per-item prologue / epilogue, in row steps (stamps)
// row-step cost of a band / mixed item, uniform = 1 (profiles/r4_stamps*.txt).
// Band 2.8 since round 5 (the equal-cost / filling layouts of mid-size
// blocks; one box, two constructions each, µs per iteration at 2.45 / 2.8
// / 3.1 / 3.4: 8-rank slab of 8192² 43.0 / 40.4-40.8 / 40.4 / 40.0-40.6,
// its 4×2 block 48.0 / 45.3-45.5 / 46.2-46.5 / 44.0-44.3, 4-rank ≈74
// throughout, 2048² 28.1-28.7 / 28.4-28.5 / 29.3 / 30.5-30.7 —
// profiles/r5_costband.txt; the slab's band row step runs ≈3.0× a uniform
// one, 8192²'s 2.25×)
const double fband = 2.8, fmixed = 1.3;
}  // namespace

// Halo/interior overlap (multi-rank single-sweep).  The sweep walks an item
// list in which, per XCD shard, the boundary items (outputs sent to a
// neighbour: first / last two owned rows and columns) come first; each bumps
// st->sig when stored.  A one-wave kernel on a high-priority halo stream waits
// for the count, then the exchange runs there while the interior items are
// still being computed.  The sweep keeps its full persistent grid minus
// 8 blocks left free for the wait / exchange / unpack kernels.
//
// The context of one build: the row / band / mixed queries of the planner's
// block, the item costs and entries, and the static layouts' common tail.
struct LayoutPlanner::Ctx {
  LayoutPlanner& P;
  const LayoutRequest& rq;
  const SweepGeometry& g;
  const int64_t nx, ny;
  const bool* has;
  const int ti, ns, nchunks;
  const bool overlap;
  const int H;        // halo rows an item re-reads per side (2 single sweep, 4 two-step, 6 three-step)
  const int HL;       // a strip's left halo columns (three-step: 8, for aligned loads and stores)
  const int64_t Wc;   // columns a wave strip loads (three-step: one per lane)
  const int64_t q0, R;
  double gen_cost;
  const bool trace3;
  const clk::time_point tl0 = clk::now();
  ItemLayout out;

  Ctx(LayoutPlanner& p, const LayoutRequest& r, int nstrips)
      : P(p), rq(r), g(p.g_), nx(p.nx_), ny(p.ny_), has(p.has_), ti(r.ti), ns(nstrips), nchunks(int((p.nx_ + r.ti - 1) / r.ti)),
        overlap(r.overlap), H(p.g_.hdep), HL(p.g_.xorg + 1), Wc(p.g_.steps >= 3 ? 64 : 128), q0(1 - p.g_.hdep),
        R(p.nx_ + 2 * p.g_.hdep), trace3(r.knobs.trace >= 3) {
    // Cost of a boundary-band row in plain rows (item costs of the layouts).
    // Since the band coefficients are evaluated once per row (LDS ring) a band
    // row costs less than the round-1 weight of 3: blocks below 2²⁴ nodes lay
    // out better at 2 (8-rank 8192² block 84.2-85.1 vs 87.3-87.8 µs per
    // iteration, 4-rank 155 vs 160, 2400×3200 77.9-79.3 vs 79.5-80.3; 1 is
    // worse everywhere); larger blocks see no difference above the placement
    // noise and keep 3 (profiles/r2_gencost.txt).
    gen_cost = double(nx) * double(ny) >= double(1 << 24) ? 3.0 : 2.0;
    // three-step LPT at 2²⁵-2²⁶ nodes (8192², 112-row items): 3.25-4 run ≈1 %
    // faster than 3 on three boxes, 5-8 ≈8 % slower (profiles/r4_ti48.txt)
    if (g.steps >= 3 && double(nx) * double(ny) >= double(1 << 25) && double(nx) * double(ny) <= double(1 << 26))
      gen_cost = 3.5;
  }
  void lap(const char* what) const {
    if (trace3)
      std::fprintf(stderr, "[pe]   layout %-14s %7.3f ms\n", what, 1e3 * std::chrono::duration<double>(clk::now() - tl0).count());
  }
  // Does local row q have a boundary-band node in strip s's loaded
  // columns?  (The kernel's has_gen on the same row-class table.)
  const int* row_class(int64_t q) const {  // null outside the table
    const int64_t t = q - g.tab_lo;  // table index of local row q
    return t < 0 || t >= int64_t(P.rowcls_.size() / 4) ? nullptr : &P.rowcls_[size_t(t) * 4];
  }
  bool row_gen_x(int64_t q, int s) const {
    const int64_t J = -(HL - 1) + int64_t(s) * g.fsw;
    const int* r = row_class(q);
    if (!r) return false;
    const int64_t lo = std::max<int64_t>(J, r[2]), hi = std::min<int64_t>(J + Wc - 1, r[3]);
    return lo <= hi && (r[0] > r[1] || lo < r[0] || hi > r[1]);
  }
  // Three-step sweep: is every row of the item's window wholly interior or
  // wholly non-interior in the strip's 64 columns (kUniBit: the kernel's
  // uniform-row march)?  Rows with a band node are never uniform here: the
  // band flag wins.
  bool row_mixed_x(int64_t q, int s) const {
    const int64_t J = -(HL - 1) + int64_t(s) * g.fsw;
    const int* r = row_class(q);
    if (!r) return true;
    const int64_t lo = std::max<int64_t>(J, r[0]), hi = std::min<int64_t>(J + Wc - 1, r[1]);
    if (lo > hi) return false;                 // no interior column
    return !(r[0] <= J && r[1] >= J + Wc - 1);  // some interior, some not
  }
  // (a row wholly interior in the strip's columns: the class of a uniform row)
  bool row_inner_x(int64_t q, int s) const {
    const int64_t J = -(HL - 1) + int64_t(s) * g.fsw;
    const int* r = row_class(q);
    return r && r[0] <= J && r[1] >= J + Wc - 1;
  }
  // Per strip, prefix counts of the band / mixed / wholly interior rows q = 1-H .. nx+H (the
  // windows of every item; built once per planner: the rows-per-item tuning
  // re-lays out up to 11 times, and evaluating the rows one by one per item
  // took 4.5-5.7 ms per layout at 4096², inside T_solver).
  void prefix_counts() {
    if (!P.pgen_.empty()) return;
    P.pgen_.assign(size_t(ns) * size_t(R + 1), 0);
    P.pmix_.assign(size_t(ns) * size_t(R + 1), 0);
    P.pinn_.assign(size_t(ns) * size_t(R + 1), 0);
    for (int s = 0; s < ns; ++s) {
      int* gp = &P.pgen_[size_t(s) * size_t(R + 1)];
      int* m = &P.pmix_[size_t(s) * size_t(R + 1)];
      int* in = &P.pinn_[size_t(s) * size_t(R + 1)];
      for (int64_t i = 0; i < R; ++i) {
        gp[i + 1] = gp[i] + (row_gen_x(q0 + i, s) ? 1 : 0);
        m[i + 1] = m[i] + (row_mixed_x(q0 + i, s) ? 1 : 0);
        in[i + 1] = in[i] + (row_inner_x(q0 + i, s) ? 1 : 0);
      }
    }
  }
  // band / mixed rows among q = a .. b of strip s (inside 1-H .. nx+H)
  int among(const std::vector<int>& pre, int64_t a, int64_t b, int s) const {
    const int* p = &pre[size_t(s) * size_t(R + 1)];
    return p[b - q0 + 1] - p[a - q0];
  }
  int ngen(int64_t a, int64_t b, int s) const { return among(P.pgen_, a, b, s); }
  int nmix(int64_t a, int64_t b, int s) const { return among(P.pmix_, a, b, s); }
  int ninn(int64_t a, int64_t b, int s) const { return among(P.pinn_, a, b, s); }
  // per-item cost: rows ib-H .. ie+H, band rows weighted
  double rows_cost(int64_t ib, int64_t ie, int s) const {
    const int64_t n = ie - ib + 1 + 2 * H, ng = ngen(ib - H, ie + H, s);
    return double(n - ng) + double(ng) * gen_cost;
  }
  bool rows_band(int64_t ib, int64_t ie, int s) const { return ngen(ib - H, ie + H, s) > 0; }
  // ... and all of one class: the uniform march takes its coefficients once
  // per item, from the window's first row.  (No window of rows that are
  // uniform in a strip holds both classes — vertical neighbours share a face,
  // so a band row lies between — and the test turns that into a guarantee.)
  bool rows_uniform(int64_t ib, int64_t ie, int s) const {
    const int64_t a = ib - H, b = ie + H;
    const int in = ninn(a, b, s);
    return ngen(a, b, s) == 0 && nmix(a, b, s) == 0 && (in == 0 || in == int(b - a + 1));
  }
  double item_cost(int ch, int s) const {
    const int64_t ib = 1 + int64_t(ch) * ti, ie = std::min<int64_t>(ib + ti - 1, nx);
    return rows_cost(ib, ie, s);
  }
  // {first row | band flag, strip | rows << 20}; the band flag selects the
  // kernel's coefficient path (rows ib-H .. ie+H include a boundary-band row)
  Entry entry(int64_t ib, int64_t rows, int s) const {
    int flag = rows_band(ib, ib + rows - 1, s) ? dev::kBandBit : 0;
    // (not the last strip of a block with an UP neighbour: its output lanes
    // past ny hold that neighbour's columns, which only the lane-tested
    // march keeps out of the sums)
    const bool cut = (has[UP] && int64_t(s + 1) * g.fsw > ny);
    if (flag == 0 && g.steps >= 3 && !cut && rows_uniform(ib, ib + rows - 1, s)) flag = dev::kUniBit;
    return Entry{int(ib) | flag, s | int(rows << 20)};
  }
  // does strip s hold outputs a DOWN / UP neighbour needs?
  bool ystrip(int s) const {
    const int64_t J = -(HL - 1) + int64_t(s) * g.fsw;
    const int64_t jlo = std::max<int64_t>(1, J + HL), jhi = std::min<int64_t>(ny, J + g.fsw + HL - 1);
    return (has[DOWN] && jlo <= H) || (has[UP] && jhi >= ny - H + 1);
  }
  // outputs a neighbour needs (the H owned rows / columns next to it: what
  // the exchange sends): first in the layout under the overlap.
  // The halo push keeps the plain layout: cutting its boundary pieces off and
  // dealing them first (the pre-round-5 layout) cost the push kernel 10 % at
  // the 8-rank slab of 8192² (64.6-65.1 vs 58.2 µs per iteration) and 4 % at
  // 4 ranks, loopback probe, profiles/r5_push_release.txt
  bool is_boundary(int64_t ib, int64_t ie, int s) const {
    return (overlap && !(rq.knobs.ov_debug & 4)) &&
           ((has[LEFT] && ib <= H) || (has[RIGHT] && ie >= nx - H + 1) || ystrip(s));
  }
  // Wave capacity: workgroup b < cus is the first one dispatched to its CU,
  // b ≥ cus the second; the SIMDs' age-ordered issue runs the first
  // workgroup's waves ≈12 % faster per row step at the 8-rank slab of
  // 8192² and 2048² (0.86 vs 0.97 µs), ≈23 % at 8192² (0.77 vs 0.95) — and
  // the slow half follows the workgroup, not the rows it marches: with the
  // lists on the workgroups in reverse order the rows' speeds reverse and
  // the workgroups' stay (PE_WPERM, tools/stamp_probe.py,
  // profiles/r5_wave_age.txt).  The fill and LPT layouts can give the first
  // workgroups' waves rho times the load of the others (PE_YOUNG = rho).
  // Measured NEUTRAL on the mid-size blocks (8-rank slab 39.5-39.8 µs per
  // iteration at rho 1.0-1.3, 4×2 43.9-44.1, 4-rank 71.9-72.5) and slower
  // at 8192² from 1.2 (3975 / 3719 it/s vs 4009): a second-slot wave speeds
  // up once its SIMD partner is done, so the SIMD stays busy either way
  // (profiles/r5_epilogue.txt).  Default 1: equal loads.
  // (ties among equally loaded waves go in wave order; one wave per
  // workgroup in turn measured neutral to 1 % slower on the 8192² splits,
  // round 5 — removed in round 6)
  double capw(int w, int Wn) const { return (Wn / dev::kWPB > rq.cus && w / dev::kWPB < rq.cus) ? rq.knobs.young : 1.0; }
  int waves_avail() const { return std::max(dev::kWPB, rq.wave_cap - (overlap ? rq.ov_reserve * dev::kWPB : 0)); }

  void lay_dynamic();
  void lay_static();
  int lay_lpt(std::vector<Piece>& pcs, std::vector<std::vector<int>>& per, int& W);
  int lay_fill(std::vector<Piece>& pcs, std::vector<std::vector<int>>& per, int& W);
  int lay_equal(std::vector<Piece>& pcs, std::vector<std::vector<int>>& per, int& W);
  void deal(const std::vector<Piece>& pcs, const std::vector<std::vector<int>>& per, int W, int nbnd);
};

// Every dynamic (order 3) sweep walks such lists, overlap or not.  Item cost
// estimate (from stamps of the sweep, tools/stamp_probe.py): a row of a
// strip that contains boundary-band nodes (coefficients evaluated from the
// chord tables) costs ≈ gen_cost plain rows; an item's rows are its own plus
// the 4 halo rows it re-reads.  Shards are contiguous chunk ranges of equal
// estimated cost (consecutive chunks stay on one XCD), and each shard lists
// its boundary items (overlap) first, then its heavy items in decreasing
// cost, then the rest chunk-major: the sweep's tail is then made of light
// items, and waves steal from other shards once their own is empty.
// (no tail split of the last items: at one placement every extra item cost
// more than the shorter drain saved — 8192², 18 rows: 545.5 µs per
// iteration unsplit vs 550.6 / 552.1 / 556.1 with 5 / 10 / 30 % split; 2
// ranks 297.8 vs 307.5, profiles/r2_layout.txt; the knob was removed in round 6)
void LayoutPlanner::Ctx::lay_dynamic() {
  const int gmin = std::max(1, std::min(out.nblocks, out.nblocks0) - (overlap ? rq.ov_reserve : 0));
  const int nsh = rq.order >= 2 ? std::min(8, gmin) : 1;
  std::vector<double> cost(size_t(out.nitems));
  std::vector<double> ccost(size_t(nchunks) + 1, 0.0);  // prefix sums per chunk
  for (int ch = 0; ch < nchunks; ++ch) {
    double cc = 0.0;
    for (int s = 0; s < ns; ++s) cc += cost[size_t(ch) * ns + s] = item_cost(ch, s);
    ccost[size_t(ch) + 1] = ccost[size_t(ch)] + cc;
  }
  const double light = double(ti + 2 * H);
  std::vector<int> cut(size_t(nsh) + 1, 0);
  for (int x = 1; x < nsh; ++x) {
    const double target = ccost.back() * x / nsh;
    int c = cut[size_t(x) - 1];
    while (c < nchunks && ccost[size_t(c) + 1] <= target) ++c;
    cut[size_t(x)] = c;
  }
  cut[size_t(nsh)] = nchunks;
  std::vector<Entry>& all = out.list;
  out.lnsh = nsh;
  for (int x = 0; x < nsh; ++x) {
    std::vector<int> b, heavy, in;
    for (int ch = cut[size_t(x)]; ch < cut[size_t(x) + 1]; ++ch)
      for (int s = 0; s < ns; ++s) {
        const int id = ch * ns + s;
        const int64_t ib = 1 + int64_t(ch) * ti, ie = std::min<int64_t>(ib + ti - 1, nx);
        if (is_boundary(ib, ie, s)) b.push_back(id);
        else if (cost[size_t(id)] > 1.25 * light) heavy.push_back(id);
        else in.push_back(id);
      }
    std::stable_sort(heavy.begin(), heavy.end(), [&](int a, int c) { return cost[size_t(a)] > cost[size_t(c)]; });
    out.lbase[x] = int(all.size());
    out.lnb[x] = int(b.size());
    out.nbnd += int(b.size());
    for (const std::vector<int>* v : {&b, &heavy, &in})
      for (int id : *v) {
        const int ch = id / ns, s = id % ns;
        const int64_t ib = 1 + int64_t(ch) * ti, ie = std::min<int64_t>(ib + ti - 1, nx);
        all.push_back(entry(ib, ie - ib + 1, s));
      }
  }
  for (int x = nsh; x <= 8; ++x) out.lbase[x] = int(all.size());
  if (int(all.size()) < out.nitems || int(all.size()) > rq.nslot_cap) throw std::logic_error("item list does not fit");
  out.nslots = int(all.size());
}

// ---- Static sweeps: a longest-processing-time-first layout ----
// Every wave walks list positions w, w + W, w + 2W, … (W = the grid's
// waves), so the host decides who does what: items are cut where one
// would exceed a wave's fair share (band items cost ≈2-3× a plain one;
// on small blocks, where each wave gets about one item, the band items
// alone were the sweep's tail — profiles/r2_small_before.txt), then
// assigned heaviest first to the least-loaded wave, and a wave's k-th
// item goes to position k·W + w (empty entries fill the gaps).  Equal
// costs keep chunk-major order, so each round of positions still covers
// a compact window of rows.  Overlap: boundary items take the first
// positions (they run in the first round).
//
// Three-step LPT.  A band item runs EVERY row step on the band path
// (≈2.25× a uniform one at 8192²: 221.8 vs 98.6 µs per 112-row item,
// profiles/r4_stamps48.txt), but costed by its band rows alone it looks
// barely heavier than a uniform one, so waves that take one still get as
// many items as the rest: the sweep ended with band items of the last rows
// (6945-7169) starting 607-631 µs into a 722 µs span (a 33-40 µs tail).
// Both ways of costing items by kind measured slower, on one box against
// the round-4 build (profiles/r5_ab_kernel.txt, profiles/r5_ab_layout.txt):
// wave LOADS counted by kind (rows + 2H fill steps × the kind's factor):
// 3632-3644 vs 3985-4005 it/s (the last rows' items then went to
// whichever waves were least loaded, a 110-123 µs tail); items also
// ORDERED by kind cost: every band item in the first round, all over
// the grid, 3519-3606 (the first round lost its row window; band items ran
// 4.1 µs per row step instead of 1.8).  The round-4 tail (late items of the
// last rows) is made of UNIFORM items whose waves ran slow — the wave-time
// spread the static costs do not predict (r4 stamps: correlation -0.1).
// Band-row costs only (the kind-cost knob was removed in round 6).
int LayoutPlanner::Ctx::lay_lpt(std::vector<Piece>& pcs, std::vector<std::vector<int>>& per, int& W) {
  double total = 0.0;
  for (int id = 0; id < out.nitems; ++id) total += item_cost(id / ns, id % ns) + overhead;
  // cut only when there are fewer items than waves (small blocks): with
  // more items than waves the layout balances them, and every cut re-reads
  // 4 more halo rows (2048²: 96 vs 91 µs per iteration with cuts)
  const int W0 = std::max(1, std::min(waves_avail(), out.nitems));
  const double share =
      out.nitems >= waves_avail() ? 1e300 : std::max(total / W0, (double(ti + 2 * H) + overhead) * 1.15);
  for (int ch = 0; ch < nchunks; ++ch)
    for (int s = 0; s < ns; ++s) {
      const int64_t ib = 1 + int64_t(ch) * ti, ie = std::min<int64_t>(ib + ti - 1, nx);
      const int64_t n = ie - ib + 1;
      const bool bnd = is_boundary(ib, ie, s);
      int parts = 1;
      if (!bnd) {
        for (; 2 * (parts + 1) <= n; ++parts) {  // pieces of >= 2 rows
          double worst = 0.0;
          for (int q = 0; q < parts; ++q)
            worst = std::max(worst, rows_cost(ib + n * q / parts, ib + n * (q + 1) / parts - 1, s) + overhead);
          if (worst <= share) break;
        }
      }
      for (int q = 0; q < parts; ++q) {
        const int64_t a0 = ib + n * q / parts, a1 = ib + n * (q + 1) / parts;
        pcs.push_back(Piece{a0, a1 - a0, s, rows_cost(a0, a1 - 1, s) + overhead, bnd});
      }
    }
  lap("pieces");
  W = std::max(dev::kWPB, (std::min<int>(waves_avail(), int(pcs.size())) / dev::kWPB) * dev::kWPB);
  per.assign(size_t(W), {});
  std::vector<double> load(size_t(W), 0.0);
  std::vector<int> order;
  int nbnd = 0;
  for (int i = 0; i < int(pcs.size()); ++i) {
    if (pcs[size_t(i)].bnd) {  // boundary pieces: positions 0, 1, … in order
      per[size_t(nbnd % W)].push_back(i);
      load[size_t(nbnd % W)] += pcs[size_t(i)].cost;
      ++nbnd;
    } else {
      order.push_back(i);
    }
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pcs[size_t(a)].cost > pcs[size_t(b)].cost; });
  using LW = std::pair<double, int>;
  std::priority_queue<LW, std::vector<LW>, std::greater<LW>> heap;
  for (int w = 0; w < W; ++w) heap.push(LW{load[size_t(w)] / capw(w, W), w});
  for (int i : order) {
    const int tw = heap.top().second;
    heap.pop();
    per[size_t(tw)].push_back(i);
    load[size_t(tw)] += pcs[size_t(i)].cost;
    heap.push(LW{load[size_t(tw)] / capw(tw, W), tw});
  }
  return nbnd;
}

// Three-step sweep: a filling layout instead.  The sweep's time per row
// step depends on the item's kind — a boundary-band item ≈2.2×, a mixed
// one ≈1.3× a uniform one (tools/stamp_probe.py, profiles/r4_stamps.txt)
// — and the LPT layout, with whole items, leaves some waves one item
// more than the rest (8192²: 8 or 9 items of 92 row steps, wave busy
// time max/mean 1.08) or a single band item longer than every other
// wave's work (8-rank slab block: 1.33).  Here an item costs its steps ×
// its kind's factor + the overhead, every wave is filled up to the fair
// share T, and the item that would overflow the least-loaded wave is cut:
// the rows that fit go there, the rest goes back into the queue (each cut
// re-reads 2H fill rows, which T accounts for).  Largest first, ties in
// chunk-major order, so each round of positions still covers a compact
// window of rows.
int LayoutPlanner::Ctx::lay_fill(std::vector<Piece>& pcs, std::vector<std::vector<int>>& per, int& W) {
  auto pcost = [&](int64_t ib, int64_t rows, int sx) {
    const Entry e = entry(ib, rows, sx);
    const double f = (e.x & dev::kBandBit) ? fband : (e.x & dev::kUniBit) ? 1.0 : fmixed;
    return double(rows + 2 * H) * f + overhead;
  };
  std::vector<Piece> whole;
  double total = 0.0;
  // Overlap (2-D blocks): the outputs the exchange sends become short
  // pieces of their own — the H rows next to a LEFT / RIGHT neighbour per
  // strip, and a DOWN / UP boundary strip cut into kOvRows-row pieces — so
  // they all run in the first round and finish within ~(kOvRows + 2H) row
  // steps; the filling below then tops their waves up with interior rows
  // (later list positions).  With whole ti-row boundary items and about one
  // item per wave the boundary items ended with the sweep and a third of
  // the exchange stayed exposed (4×2 block: 56.8 vs 50.9 µs per
  // iteration at 15 / 8 µs delays, profiles/r4_overlap.txt).
  constexpr int64_t kOvRows = 8;
  const bool ov_split = overlap && !(rq.knobs.ov_debug & 4);
  auto add_whole = [&](int64_t a, int64_t rows, int sx, bool bnd) {
    whole.push_back(Piece{a, rows, sx, pcost(a, rows, sx), bnd});
    total += whole.back().cost;
  };
  for (int ch = 0; ch < nchunks; ++ch)
    for (int sx = 0; sx < ns; ++sx) {
      const int64_t ib = 1 + int64_t(ch) * ti, n = std::min<int64_t>(ib + ti - 1, nx) - ib + 1;
      const int64_t ie = ib + n - 1;
      if (!ov_split || !is_boundary(ib, ie, sx)) {
        add_whole(ib, n, sx, is_boundary(ib, ie, sx));
      } else if (ystrip(sx)) {
        for (int64_t a = ib; a <= ie; a += kOvRows) add_whole(a, std::min<int64_t>(kOvRows, ie - a + 1), sx, true);
      } else {
        const int64_t lo = has[LEFT] ? std::min<int64_t>(ie, H) : ib - 1;             // rows ib .. lo: LEFT's
        const int64_t hi = has[RIGHT] ? std::max<int64_t>(ib, nx - H + 1) : ie + 1;  // hi .. ie: RIGHT's
        if (lo >= ib) add_whole(ib, lo - ib + 1, sx, true);
        const int64_t m0 = std::max(ib, lo + 1), m1 = std::min(ie, hi - 1);
        if (m1 >= m0) add_whole(m0, m1 - m0 + 1, sx, false);
        const int64_t r0 = std::max(hi, std::max(ib, lo + 1));  // (never a row of the LEFT piece again)
        if (r0 <= ie) add_whole(r0, ie - r0 + 1, sx, true);
      }
    }
  lap("fill: pieces");
  const int64_t minr = 8;  // shortest cut piece (its 2H fill rows cost more than it)
  const double minc = double(minr + 2 * H) + overhead;
  W = std::max(dev::kWPB, (std::min<int>(waves_avail(), int(total / minc)) / dev::kWPB) * dev::kWPB);
  const double cut_cost = double(2 * H) + overhead;  // a cut's extra (uniform) row steps
  int cuts = 0, nbnd = 0;
  std::vector<double> load;
  // each piece's wave (pcs order; the per-wave lists are built once, after
  // the last pass)
  std::vector<int> own;
  // (on blocks of about one item per wave the passes alternate between
  // many cuts and few — 8-rank slab of 8192² at 96 rows: 1744 / 175 — and
  // the fourth pass's is kept; keeping the pass of the lowest estimated
  // makespan measured the same, whole pieces without cuts 1.5× slower:
  // profiles/r6_fill_passes.txt.  Once the cut count returns to an
  // earlier pass's input the rest of the passes repeat earlier ones, so
  // the loop stops there with the result the fourth pass would give.)
  struct PassRes {
    std::vector<Piece> pcs;
    std::vector<int> own;
    int nbnd = 0, ncut = 0;
  } prev;
  int in_prev = -1;
  for (int pass = 0; pass < 4; ++pass) {
    const double T = (total + cuts * cut_cost) / W;
    pcs.clear();
    own.clear();
    load.assign(size_t(W), 0.0);
    nbnd = 0;
    int ncut = 0;
    // (queued pieces by index into qp: a heap of 16-byte entries)
    struct QE {
      double cost;
      int seq, idx;
      bool operator<(const QE& o) const { return cost < o.cost || (cost == o.cost && seq > o.seq); }
    };
    std::vector<Piece> qp;
    qp.reserve(whole.size() + whole.size() / 2);
    std::vector<QE> qv;
    qv.reserve(whole.size());
    for (int i = 0; i < int(whole.size()); ++i) {
      const Piece& p = whole[size_t(i)];
      if (p.bnd) {  // boundary pieces: positions 0, 1, … in order (first round)
        own.push_back(nbnd % W);
        load[size_t(nbnd % W)] += p.cost;
        pcs.push_back(p);
        ++nbnd;
      } else {
        qv.push_back(QE{p.cost, i, int(qp.size())});
        qp.push_back(p);
      }
    }
    std::priority_queue<QE> q(std::less<QE>(), std::move(qv));
    using LW = std::pair<double, int>;
    std::priority_queue<LW, std::vector<LW>, std::greater<LW>> heap;
    double csum = 0.0;
    for (int w = 0; w < W; ++w) csum += capw(w, W);
    for (int w = 0; w < W; ++w) heap.push(LW{load[size_t(w)] / capw(w, W), w});
    while (!q.empty()) {
      const QE e = q.top();
      q.pop();
      const Piece ep = qp[size_t(e.idx)];
      const int tw = heap.top().second;
      heap.pop();
      const double room = (rq.knobs.young == 1.0 ? T : T * W * capw(tw, W) / csum) - load[size_t(tw)];
      Piece give = ep;
      if (ep.cost > room && room >= minc && ep.rows >= 2 * minr) {
        // the most rows of ep that fit the room (binary search; cost grows with rows)
        int64_t lo = minr, hi = ep.rows - minr, best = 0;
        while (lo <= hi) {
          const int64_t mid = (lo + hi) / 2;
          if (pcost(ep.ib, mid, ep.s) <= room) {
            best = mid;
            lo = mid + 1;
          } else {
            hi = mid - 1;
          }
        }
        if (best > 0) {
          give = Piece{ep.ib, best, ep.s, pcost(ep.ib, best, ep.s), false};
          const Piece rest{ep.ib + best, ep.rows - best, ep.s, pcost(ep.ib + best, ep.rows - best, ep.s), false};
          q.push(QE{rest.cost, e.seq, int(qp.size())});
          qp.push_back(rest);
          ++ncut;
        }
      }
      own.push_back(tw);
      pcs.push_back(give);
      load[size_t(tw)] += give.cost;
      heap.push(LW{load[size_t(tw)] / capw(tw, W), tw});
    }
    if (trace3) std::fprintf(stderr, "[pe]   layout fill pass %d: %zu pieces, %d cuts, W %d\n", pass, pcs.size(), ncut, W);
    lap("fill: pass");
    if (ncut == cuts) break;
    if (pass >= 1 && ncut == in_prev) {  // inputs now alternate: pass 3 repeats pass 1
      if (pass % 2 == 0) {
        pcs = std::move(prev.pcs);
        own = std::move(prev.own);
        nbnd = prev.nbnd;
        ncut = prev.ncut;
      }
      cuts = ncut;
      break;
    }
    if (pass < 3) prev = PassRes{pcs, own, nbnd, ncut};
    in_prev = cuts;
    cuts = ncut;
  }
  std::vector<int> cnt(size_t(W), 0);
  for (int w : own) ++cnt[size_t(w)];
  per.assign(size_t(W), {});
  for (int w = 0; w < W; ++w) per[size_t(w)].reserve(size_t(cnt[size_t(w)]));
  for (size_t i = 0; i < own.size(); ++i) per[size_t(own[i])].push_back(int(i));
  out.cuts = cuts;
  return nbnd;
}

// Three-step sweep: EQUAL-COST PIECES, EXACTLY k PER WAVE.  Whole items
// cannot balance ~8 items per wave: the waves hold 8 or 9 uniform items,
// or a band item of 2.3 uniform ones (8192²: wave busy time max/mean
// 1.06-1.08; the 8-rank slab block's waves with one 41-row band item ran
// 1.30× the mean — tools/stamp_probe.py, profiles/r4_stamps*.txt).  So
// every strip is cut into runs of one march kind (a row is "band" when a
// boundary-band row lies within H rows of it — the kernel marches an
// item whose window holds one on the band path — else "mixed" likewise,
// else uniform), every run into n_g pieces of equal rows, with the n_g
// chosen so that a piece costs X ≈ (its rows + 2H fill rows) × its
// kind's factor + overhead everywhere and there are exactly k·W pieces;
// the pieces, sorted by cost (ties in row order), are dealt in rounds of
// W, snaking, so each wave gets k pieces and each round a compact window
// of rows.  k follows the rows-per-item knob: uniform pieces of ≈ ti rows.
int LayoutPlanner::Ctx::lay_equal(std::vector<Piece>& pcs, std::vector<std::vector<int>>& per, int& W) {
  struct Seg {
    int64_t a, rows;
    int s;
    double f;
    bool bnd;
    int n;
  };
  // (the runs do not depend on the rows per item: found once per planner
  // and overlap setting — the scan of every row of every strip was a
  // quarter of each of the tuning's layouts)
  std::vector<std::array<int64_t, 4>>& runs = P.eq_runs_[overlap ? 1 : 0];
  if (runs.empty()) {
    for (int sx = 0; sx < ns; ++sx) {
      auto kind = [&](int64_t q) {  // 2 band, 1 mixed, 0 uniform (window q-H .. q+H)
        return ngen(q - H, q + H, sx) > 0 ? 2 : nmix(q - H, q + H, sx) > 0 ? 1 : 0;
      };
      int64_t a = 1;
      int ka = kind(1);
      for (int64_t q = 2; q <= nx + 1; ++q) {
        const int kq = q <= nx ? kind(q) : -1;
        // (pieces: also split where a neighbour's halo rows begin, so the
        // overlap's boundary pieces stay small)
        const bool cut_b = overlap && ((has[LEFT] && q == H + 1) || (has[RIGHT] && q == nx - H + 1));
        if (kq != ka || cut_b) {
          runs.push_back({a, q - a, sx, ka});
          a = q;
          ka = kq;
        }
      }
    }
  }
  std::vector<Seg> segs;
  segs.reserve(runs.size());
  for (const auto& r : runs)
    segs.push_back(Seg{r[0], r[1], int(r[2]), r[3] == 2 ? fband : r[3] == 1 ? fmixed : 1.0,
                       is_boundary(r[0], r[0] + r[1] - 1, int(r[2])), 1});
  lap("equal: runs");
  const int64_t minr = 8, maxr = 128;  // (pieces of the tuned heights' range)
  auto Fk = [&](double f) { return double(2 * H) * f + overhead; };  // a piece's fill rows + overhead
  // pieces of a run for a piece cost X: rows·f / (X − F) rounded, within [rows/maxr, rows/minr]
  auto nfor = [&](const Seg& sg, double X) {
    const double want = double(sg.rows) * sg.f / std::max(1e-9, X - Fk(sg.f));
    const int64_t lo = std::max<int64_t>(1, (sg.rows + maxr - 1) / maxr), hi = std::max<int64_t>(lo, sg.rows / minr);
    return int(std::min<int64_t>(hi, std::max<int64_t>(lo, std::llround(want))));
  };
  auto count = [&](double X) {
    int64_t n = 0;
    for (const Seg& sg : segs) n += nfor(sg, X);
    return n;
  };
  int64_t Pmax = 0, Pmin = 0;
  for (const Seg& sg : segs) {
    Pmax += std::max<int64_t>(1, sg.rows / minr);
    Pmin += std::max<int64_t>(1, (sg.rows + maxr - 1) / maxr);
  }
  W = std::max<int>(dev::kWPB, int(std::min<int64_t>(waves_avail(), Pmax) / dev::kWPB) * dev::kWPB);
  const double X0 = double(ti + 2 * H) + overhead;  // a uniform piece of ti rows
  int kr = int(std::max<int64_t>(1, std::llround(double(count(X0)) / W)));
  while (int64_t(kr) * W < Pmin) ++kr;
  while (kr > 1 && int64_t(kr) * W > Pmax) --kr;
  const int64_t Pn = std::min<int64_t>(Pmax, int64_t(kr) * W);
  // the piece cost X that gives Pn pieces (count(X) falls as X grows)
  double lo = Fk(fband) + 1e-3, hi = 1e9;
  for (int it = 0; it < 200 && hi - lo > 1e-9 * hi; ++it) {
    const double mid = 0.5 * (lo + hi);
    (count(mid) > Pn ? lo : hi) = mid;
  }
  for (Seg& sg : segs) sg.n = nfor(sg, hi);
  lap("equal: bisect");
  // exactly Pn: add pieces where they are largest, remove where the merge is cheapest
  int64_t have = count(hi);
  auto pc = [&](const Seg& sg, int n) { return double(sg.rows) * sg.f / n + Fk(sg.f); };
  while (have != Pn) {
    int best = -1;
    double bv = 0.0;
    for (int i = 0; i < int(segs.size()); ++i) {
      const Seg& sg = segs[size_t(i)];
      if (have < Pn && sg.rows / (sg.n + 1) >= minr) {
        const double v = pc(sg, sg.n);
        if (best < 0 || v > bv) best = i, bv = v;
      } else if (have > Pn && sg.n > 1 && (sg.rows + sg.n - 2) / (sg.n - 1) <= maxr) {
        const double v = pc(sg, sg.n - 1);
        if (best < 0 || v < bv) best = i, bv = v;
      }
    }
    if (best < 0) break;
    segs[size_t(best)].n += have < Pn ? 1 : -1;
    have += have < Pn ? 1 : -1;
  }
  lap("equal: exact P");
  if (trace3) std::fprintf(stderr, "[pe]   layout equal: %zu runs, %lld pieces\n", segs.size(), (long long)Pn);
  for (const Seg& sg : segs)
    for (int j = 0; j < sg.n; ++j) {
      const int64_t a0 = sg.a + sg.rows * j / sg.n, a1 = sg.a + sg.rows * (j + 1) / sg.n;
      pcs.push_back(Piece{a0, a1 - a0, sg.s, double(a1 - a0) * sg.f + Fk(sg.f), is_boundary(a0, a1 - 1, sg.s)});
    }
  // boundary pieces first (overlap), then in row order (chunk-major:
  // a round of W positions covers a compact window of rows, and the
  // neighbouring strips of the same rows run on one workgroup's waves —
  // sorting by cost first scattered the rounds: 8192² 287 vs 254 µs per
  // iteration, profiles/r4_layout2.txt)
  std::vector<int> ord(pcs.size());
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = int(i);
  // (row bands of ~ti rows by the pieces' centres, then strips: the
  // neighbouring strips of the same rows run on one workgroup's waves —
  // sorting by first row alone interleaved strips whose pieces start a
  // row apart: 8192² 279 vs 254 µs, profiles/r4_layout2.txt)
  auto band_of = [&](const Piece& p) { return (2 * p.ib + p.rows - 1) / (2 * int64_t(ti)); };
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) {
    const Piece &a = pcs[size_t(x)], &b = pcs[size_t(y)];
    if (a.bnd != b.bnd) return a.bnd;
    const int64_t ra = band_of(a), rb = band_of(b);
    if (ra != rb) return ra < rb;
    return a.s != b.s ? a.s < b.s : a.ib < b.ib;
  });
  // Dealt round by round, one piece per wave: a round's boundary pieces
  // take its first waves (the kernel's kSignal variant counts list
  // positions 0 .. nbnd-1 as the boundary items), its odd pieces (short
  // runs, rounding: up to ±50 % off the target cost) the least-loaded
  // waves so far, heaviest first, and the rest (within ±15 %) the
  // remaining waves in order, so neighbouring strips stay on
  // neighbouring waves.
  lap("equal: sorted");
  int nbnd = 0;
  per.assign(size_t(W), {});
  std::vector<double> wl(size_t(W), 0.0);
  std::vector<char> taken(size_t(W), 0);
  std::vector<int> byload(static_cast<size_t>(W), 0);
  for (size_t r0 = 0; r0 < ord.size(); r0 += size_t(W)) {
    const size_t r1 = std::min(ord.size(), r0 + size_t(W));
    std::vector<int> odd, norm;
    std::fill(taken.begin(), taken.end(), 0);
    int wb = 0;
    for (size_t i = r0; i < r1; ++i) {
      const Piece& p = pcs[size_t(ord[i])];
      if (p.bnd) {  // (ord: boundary pieces first, so these are waves 0, 1, … of the round)
        per[size_t(wb)].push_back(ord[i]);
        wl[size_t(wb)] += p.cost;
        taken[size_t(wb++)] = 1;
        ++nbnd;
        continue;
      }
      (std::fabs(p.cost - hi) > 0.15 * hi ? odd : norm).push_back(ord[i]);
    }
    if (!odd.empty()) {
      std::stable_sort(odd.begin(), odd.end(), [&](int x, int y) { return pcs[size_t(x)].cost > pcs[size_t(y)].cost; });
      for (int r = 0; r < W; ++r) byload[size_t(r)] = r;
      std::stable_sort(byload.begin(), byload.end(), [&](int x, int y) { return wl[size_t(x)] < wl[size_t(y)]; });
      size_t q = 0;
      for (size_t j = 0; j < odd.size(); ++j) {
        while (taken[size_t(byload[q])]) ++q;
        const int w = byload[q];
        per[size_t(w)].push_back(odd[j]);
        wl[size_t(w)] += pcs[size_t(odd[j])].cost;
        taken[size_t(w)] = 1;
      }
    }
    size_t w = 0;
    for (int id : norm) {
      while (taken[w]) ++w;
      per[w].push_back(id);
      wl[w] += pcs[size_t(id)].cost;
      taken[w] = 1;
    }
  }
  out.cuts = int(pcs.size());
  return nbnd;
}

// The static layouts' common tail: per[w] dealt into the rounds × W list
// through the wave permutation, then the load statistics.
void LayoutPlanner::Ctx::deal(const std::vector<Piece>& pcs, const std::vector<std::vector<int>>& per, int W, int nbnd) {
  size_t rounds = 0;
  for (const auto& v : per) rounds = std::max(rounds, v.size());
  for (int w = 0; w < W; ++w) {
    double l = 0.0;
    for (int i : per[size_t(w)]) l += pcs[size_t(i)].cost;
    out.max = std::max(out.max, l);
    out.mean += l / W;
  }
  out.items = int(rounds);
  // List w runs on physical wave w (the persistent grid's workgroup b runs
  // on XCD b mod 8).  XCD-aware maps — each XCD marching a contiguous run of
  // strips so shared halo lines are fetched once into its L2 — read 3-7 %
  // fewer DRAM bytes but ran 0-12 % slower (profiles/r3_three_ti.txt,
  // profiles/r5_dram_layout.txt); removed in round 6.
  // PE_WPERM (diagnostic: does a slow item stay slow on another wave?):
  // 1 lists on the workgroups in reverse order, 2 rotated by a quarter of
  // the grid (other co-resident workgroup pairs)
  const int nb = W / dev::kWPB, m = rq.knobs.wperm;
  out.list.assign(rounds * size_t(W), Entry{0, 0});  // {0, 0}: empty entry (0 rows)
  for (int w = 0; w < W; ++w) {
    const int b = w / dev::kWPB, l = w % dev::kWPB;
    const int pb = m == 1 ? nb - 1 - b : m == 2 ? (b + nb / 4) % nb : b;
    for (size_t r = 0; r < per[size_t(w)].size(); ++r) {
      const Piece& p = pcs[size_t(per[size_t(w)][r])];
      out.list[r * size_t(W) + size_t(pb * dev::kWPB + l)] = entry(p.ib, p.rows, p.s);
    }
  }
  out.static_waves = out.lwaves = W;
  out.nbnd = nbnd;
  out.lbase[0] = 0;
  for (int x = 1; x <= 8; ++x) out.lbase[x] = int(out.list.size());
  out.lnb[0] = nbnd;
  out.nslots = int(out.list.size());
  // static list walk: the grid is the one the list was laid out for (plus
  // the blocks the overlap keeps free for the halo stream)
  out.nblocks = out.nblocks0 = W / dev::kWPB + (overlap ? rq.ov_reserve : 0);
}

void LayoutPlanner::Ctx::lay_static() {
  // three-step layouts: the knob forces one; else the request's (the
  // construction's choice: by block size, or by the rows-per-item tuning)
  const bool forced = !rq.knobs.force_layout.empty();
  std::string lay = forced ? rq.knobs.force_layout : rq.name;
  // (the overlap's short boundary pieces: the filling layout — on
  // blocks of about one item per wave, where whole boundary items end with
  // the sweep: 4×2 block of 8192² 59.3 µs per iteration at 15 / 8 µs delays
  // vs 57.5 without delays or overlap.  Larger blocks keep their layout with
  // whole boundary items first, which already runs them in the first of
  // several rounds; the filling layout cost the 2×2 block 18 % there —
  // 108 vs 90.9 µs at zero delay, profiles/r5_overlap.txt)
  if (overlap && !forced && double(nx) * double(ny) < 1.2e7) lay = "fill";
  if (g.steps < 3) lay = "lpt";
  out.name = lay == "equal" || lay == "fill" ? lay : "lpt";
  std::vector<Piece> pcs;
  std::vector<std::vector<int>> per;
  int W = 0;
  const int nbnd = out.name == "equal" ? lay_equal(pcs, per, W) : out.name == "fill" ? lay_fill(pcs, per, W) : lay_lpt(pcs, per, W);
  lap(out.name.c_str());
  deal(pcs, per, W, nbnd);
  lap("list");
}

ItemLayout LayoutPlanner::build(const LayoutRequest& rq) {
  const int nstrips = int(g_.strips);
  Ctx c(*this, rq, nstrips);
  ItemLayout& out = c.out;
  // Items of `ti` rows: counts and the persistent grids sized for them.
  out.nitems = int(int64_t(nstrips) * ((nx_ + rq.ti - 1) / rq.ti));
  // fewest waves that keep every wave's share of the n items equal
  auto grid_for = [&](int cap, int n) {
    const int per = (n + cap - 1) / cap;
    const int waves = (n + per - 1) / per;
    return std::max(1, (waves + dev::kWPB - 1) / dev::kWPB);
  };
  out.nblocks = grid_for(rq.wave_caps[0], out.nitems);
  out.nblocks0 = grid_for(rq.wave_caps[1], out.nitems);
  out.nslots = out.nitems;
  // Lists: dynamic sweeps (order 3), static chunk-major sweeps (order 0:
  // heavy items split) and the overlap; orders 1 / 2 are plain tuning walks.
  if (!g_.fused || ((rq.order == 1 || rq.order == 2) && !rq.overlap)) return out;
  c.lap("start");
  c.prefix_counts();
  rq.order == 0 ? c.lay_static() : c.lay_dynamic();
  return std::move(out);
}

}  // namespace pe
