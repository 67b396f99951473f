// Host-only planner of the sweeps' work-item lists: which wave marches which
// rows of which strip (static LPT / filling / equal-cost layouts, dynamic
// per-XCD shards; boundary items first under the halo/interior overlap).
// Pure arithmetic over the row-class table: no device, no environment.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace pe {

namespace dev {
constexpr int kWPB = 4;          // waves per block
constexpr int kSW = 128;         // columns per wave strip (2 per lane, 16-B accesses)
constexpr int kTImax = 62;       // max rows per work item (rows ib-1..ie+1 live one per lane)
// Item-list entries {first row | band flag, strip | rows << 20}: kBandBit set
// when the item's rows ib-2 .. ie+2 contain a boundary-band row in its strip
// (general march); clear → the plain unrolled march.
constexpr int kBandBit = 1 << 30;
constexpr int kRowMask = kBandBit - 1;
// Three-step sweep only: kUniBit set when the rows ib-6 .. ie+6 of the item
// lie all wholly inside or all wholly outside the interior in its strip's
// window (the kernel's uniform march: three scalars per item, no lane tests).
constexpr int kUniBit = 1 << 29;
constexpr int kRowMask3 = kUniBit - 1;
constexpr int kFSW = 124;        // fused sweep: output columns per wave strip (128 loaded, 2-column halo per side)
constexpr int kFSW2 = 120;       // two-step sweep: output columns per strip (4-column halo per side)
constexpr int kTImax2 = 48;      // two-step sweep: max rows per item (rows ib-4 .. ie+5 live one per lane)
constexpr int kFSW3 = 48;        // three-step sweep: output columns per 64-column strip (one per lane; 6-column halo needed per side)
constexpr int kHL3 = 8;          // three-step sweep: left halo lanes of a strip (right: 64 - kFSW3 - kHL3); with the
                                 // rows' element 0 at column -(kHL3 - 1), every strip's loads are whole 128-B lines
                                 // and its outputs whole 64-B segments
constexpr int kTImax3 = 512;     // three-step sweep: max rows per item (row windows reload every ~58 rows)
}  // namespace dev

// One list position: {first row | flags, strip | rows << 20} (the device's int2).
struct Entry {
  int x, y;
};

// Field planes, strips and table ranges of a block's sweep.
struct SweepGeometry {
  bool fused = false;
  int steps = 1;          // iterations per sweep launch (1, 2, 3)
  int fsw = 124;          // output columns per strip (kFSW / kFSW2 / kFSW3)
  int hdep = 2;           // halo depth of the single-sweep layouts (2 / 4 / 6)
  int xorg = 1;           // columns stored left of column 0 (KParams::xorg)
  int64_t strips = 0, plane = 0;     // strips across the block; doubles per row of a plane
  int64_t rows_hi = 0, cols_hi = 0;  // chord tables / row classes reach local rows / columns tab_lo .. rows_hi / cols_hi
  int64_t tab_lo = -1;
  int64_t xsize = 0, wsize = 0;      // doubles of one x buffer (r and p planes interleaved by row) / of w
};
SweepGeometry sweep_geometry(int64_t nx, int64_t ny, int steps, bool fused);

// Rows-per-item candidates of the construction's tuning, ascending.
std::vector<int> ti_candidates(const SweepGeometry& g, int64_t nx, int64_t ny, int wave_cap);

struct LayoutKnobs {
  std::string force_layout;  // PE_LAYOUT: forces a three-step static layout ("": the request's name)
  double young = 1.0;        // PE_YOUNG: load ratio of the first workgroups' waves (fill / LPT)
  int wperm = 0;             // PE_WPERM: diagnostic list → workgroup permutation (0 none, 1 reversed, 2 rotated)
  int ov_debug = 0;          // PE_OV_DEBUG bits: 4 natural item order (no boundary-first list)
  int trace = 0;             // PE_CTOR_TRACE level: >= 3 prints the layout's phases to stderr
};

struct LayoutRequest {
  int ti = 16;               // rows per item
  int order = 0;             // 0 static list, 1 / 2 plain tuning walks, 3 dynamic per-XCD queues
  bool overlap = false;      // halo/interior overlap: boundary items first
  std::string name = "lpt";  // three-step static layout: lpt / fill / equal
  int wave_caps[2] = {2048, 2048};  // resident waves of the applying / deferring sweep
  int wave_cap = 2048;       // resident waves of the sweep grid (the smaller of the two)
  int cus = 256;             // compute units (a static layout's first `cus` workgroups run first on their CU)
  int ov_reserve = 8;        // blocks the overlap keeps free for the halo stream
  int nslot_cap = 1 << 30;   // item-sum slots allocated (a dynamic list must fit)
  LayoutKnobs knobs;
};

struct ItemLayout {
  std::vector<Entry> list;   // empty: a walk without a list
  int static_waves = 0;      // static list walk: waves the list is laid out for (0: no static list)
  int nbnd = 0;              // boundary items of the list (overlap)
  // shard x owns list[lbase[x] .. lbase[x+1]), its first lnb[x] entries the
  // boundary items (the overlapped launch's; the plain one counts none)
  int lnsh = 1, lbase[9] = {}, lnb[8] = {};
  int nslots = 0, lwaves = 0, nitems = 0, nblocks = 1, nblocks0 = 1;
  // static layout: most items on one wave, items cut, heaviest / mean wave load (row steps)
  int items = 0, cuts = 0;
  double max = 0, mean = 0;
  std::string name = "lpt";  // the static layout actually used
};

class LayoutPlanner {
 public:
  // has: LEFT, RIGHT, DOWN, UP neighbours; rowcls: the block's row classes from local row g.tab_lo
  LayoutPlanner(const SweepGeometry& g, int64_t nx, int64_t ny, const bool has[4], std::vector<int> rowcls);
  ItemLayout build(const LayoutRequest& rq);
  // the row classes the lists are planned from: {in_lo, in_hi, out_lo, out_hi} per local row, from row tab_lo()
  const std::vector<int>& row_classes() const { return rowcls_; }
  int64_t tab_lo() const { return g_.tab_lo; }

 private:
  struct Ctx;
  SweepGeometry g_;
  int64_t nx_, ny_;
  bool has_[4];
  std::vector<int> rowcls_;
  std::vector<int> pgen_, pmix_, pinn_;  // per strip, prefix counts of the band / mixed / wholly interior rows (built at the first list)
  std::vector<std::array<int64_t, 4>> eq_runs_[2];  // equal-cost layout: runs {first row, rows, strip, kind} (no overlap / overlap)
};

}  // namespace pe
