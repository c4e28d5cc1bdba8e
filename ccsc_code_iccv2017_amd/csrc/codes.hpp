// Threshold-and-compact of a dense column-major [M, n] fp64 matrix into a compressed
// sparse column triple (codes.hip): the geometry both the kernels and the host share, and
// the launchers.  Every offset is int64: the kept entries of a call can pass 2^32.
#pragma once

#include "kernels.hpp"

namespace ccsc {

constexpr int kCodesNT = 256;                        // threads of a workgroup: 4 waves
constexpr int kCodesSteps = 8;                       // 64-entry steps of one wave
constexpr int kCodesWaveRun = 64 * kCodesSteps;      // contiguous entries of one wave
constexpr int kCodesTile = (kCodesNT / 64) * kCodesWaveRun;   // entries of a column per workgroup
constexpr int kCodesScanPer = 8;                     // counts per thread of the scan
constexpr int kCodesScanBlock = kCodesNT * kCodesScanPer;     // counts per scan workgroup
constexpr int64_t kCodesMaxRows = (int64_t)1 << 31;  // M must stay below

// ---- the offset arithmetic, in one place (ccsc_test_codes_index evaluates it on the host) --
// Tile t of a chunk of columns is rows [row0, row0 + kCodesTile) of column t / tpc; wave w
// of its workgroup owns the kCodesWaveRun rows from row0 + w * kCodesWaveRun and takes them
// in kCodesSteps steps of 64 lanes.
__host__ __device__ inline int64_t codes_tiles_per_col(int64_t M) {
  return (M + kCodesTile - 1) / kCodesTile;
}
__host__ __device__ inline int64_t codes_tile_col(int64_t tile, int64_t tpc) { return tile / tpc; }
__host__ __device__ inline int64_t codes_row(int64_t tile, int64_t tpc, int wave, int step,
                                             int lane) {
  const int64_t row0 = (tile - codes_tile_col(tile, tpc) * tpc) * kCodesTile;
  return row0 + (int64_t)wave * kCodesWaveRun + (int64_t)step * 64 + lane;
}
// element (row, col) of the column-major matrix
__host__ __device__ inline int64_t codes_elem(int64_t col, int64_t M, int64_t row) {
  return col * M + row;
}
// slot of a kept entry: the exclusive scan of the tile counts, the kept entries of the
// tile before this wave step, the kept lanes below this one
__host__ __device__ inline int64_t codes_slot(int64_t tile_off, int64_t before, int prefix) {
  return tile_off + before + (int64_t)prefix;
}
// scan workgroups over T counts, and the workspace of a chunk of T tiles: T + 1 offsets
// (the last is the chunk's total), the scan's workgroup sums and their total, the column
// offsets of up to `cols` columns, then 16 B of staging (row index, value) per kept entry
__host__ __device__ inline int64_t codes_scan_blocks(int64_t T) {
  return (T + kCodesScanBlock - 1) / kCodesScanBlock;
}
inline int64_t codes_count_ws_bytes(int64_t T, int64_t cols) {
  return 8 * ((T + 1) + (codes_scan_blocks(T) + 1) + (cols + 1));
}
inline int64_t codes_stage_bytes(int64_t kept) { return 16 * kept; }

// ---- codes.hip ---------------------------------------------------------------------
// a: device [M, m] fp64, column-major.  An entry is kept iff !(|a| <= eps).
// off[0 .. T] (T = m * tiles per column): the exclusive scan of the kept entries per tile,
// off[T] their total; bsum: codes_scan_blocks(T) + 1 entries of scratch; cols[0 .. m]: the
// offset of every column's first kept entry, cols[m] the total.
hipError_t launch_codes_count(const double* a, int64_t M, int64_t m, double eps, int64_t* off,
                              int64_t* bsum, int64_t* cols, hipStream_t st);
// ir[s], pr[s] for slot s of every kept entry, rows ascending inside a column, columns in
// order: off as launch_codes_count left it for the same a, M, m and eps.
hipError_t launch_codes_scatter(const double* a, int64_t M, int64_t m, double eps,
                                const int64_t* off, int64_t* ir, double* pr, hipStream_t st);

}  // namespace ccsc
