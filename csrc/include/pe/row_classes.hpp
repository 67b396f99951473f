// Host-side chord tables and per-row coefficient classes of a block
// (csrc/core/row_classes.cpp), and the item-layout planner built from them.
// No device code: the solver uploads what these return.
#pragma once

#include <cstdint>
#include <vector>

#include "pe/decomp.hpp"
#include "pe/item_layout.hpp"
#include "pe/problem.hpp"

namespace pe {

// Per-row coefficient classes from the chord tables (see row_classes.cpp):
// for each local row q ∈ [-1, rows_hi-1], {in_lo, in_hi, out_lo, out_hi} such
// that every face coefficient of node (q, lj) is exactly 1 for lj ∈ [in_lo,
// in_hi] and exactly 1/eps for lj ∉ [out_lo, out_hi], lj ∈ [-1, cols_hi].
// Conservative: anything else is evaluated exactly.  (rows_hi+2) × 4 ints.
// Tables and classes start at local index `lo` (-1; the two-step sweep's
// 4-deep halo: -4): entry of local q at (q - lo).
std::vector<int> row_classes(const double* colT, const double* rowT, int64_t rows_hi, int64_t cols_hi,
                             int64_t lo = -1);
// Chord tables of a block: (rows_hi+2)×4 column entries {halfA, sB, eB, x}
// for li ∈ [-1, rows_hi], then (cols_hi+2)×4 row entries {sA, eA, halfB, y}
// for lj ∈ [-1, cols_hi]; indexed by local index + 1.  The classic kernels
// use rows_hi = nx+2, cols_hi = ny+2; the single-sweep kernel reaches two
// halo nodes further and past ny into strip padding.
std::vector<double> chord_tables(const Problem& P, const Block& blk, int64_t rows_hi, int64_t cols_hi,
                                 int64_t lo = -1);
// The item-layout planner of a block (its chord tables and row classes are
// computed here): the lists a solver of `steps` iterations per sweep would
// walk, without a device.
LayoutPlanner block_planner(const Problem& P, const Block& blk, int steps, bool fused = true);
// Host mirror of the kernels' coefficient path for local (li, lj) ∈
// [0, nx+1] × [0, ny+1]: a(li, lj), b(li, lj) and the class (0 interior,
// 1 exterior, 2 boundary band).  Row-major (nx+2) × (ny+2).
void host_coefficients(const Problem& P, const Block& blk, std::vector<double>& a, std::vector<double>& b,
                       std::vector<int>& cls);

}  // namespace pe
