// Synthesis from sparse codes (synth_codes.hip): out[:, :, :, c, j] = sum_k d_k (*) z_kj as a
// direct circular convolution over the entries of a compressed sparse column matrix, and the
// inverse of the threshold-and-compact (CSC -> dense).  The geometry and index arithmetic
// the kernels and the host share, and the launchers.  Every offset into ir / pr / out is
// int64; a row index stays below 2^31.
#pragma once

#include "kernels.hpp"

namespace ccsc {

constexpr int kSynthNT = 256;                  // threads of a workgroup: 4 waves
constexpr int kSynthTX = 16, kSynthTY = 16;    // output tile of one t-plane: a pixel per thread
constexpr int kSynthCG = 4;                    // channel accumulators a thread holds
constexpr int kSynthList = 512;                // hits an LDS list takes before it is flushed
constexpr int kExpandSeg = 4096;               // entries of a column per k_codes_expand workgroup
constexpr int64_t kSynthMaxRows = (int64_t)1 << 31;    // M = X Y T K must stay below
constexpr int64_t kSynthMaxTaps = (int64_t)1 << 31;    // C K s0 s1 s2 must stay below
static_assert(kSynthTX * kSynthTY == kSynthNT, "one output pixel per thread");
static_assert(kSynthList >= kSynthNT, "a list takes at least one chunk of entries");

struct SynthGeom {
  int32_t g[3];    // grid X, Y, T
  int32_t ks[3];   // filter extents s0, s1, s2 (odd, <= g)
  int32_t C, K;
};

// ---- the index arithmetic, in one place (ccsc_test_synth_index evaluates it on the host) ----
__host__ __device__ inline int64_t synth_rows(const SynthGeom& G) {
  return (int64_t)G.g[0] * G.g[1] * G.g[2] * G.K;
}
__host__ __device__ inline int64_t synth_taps(const SynthGeom& G) {   // of one (c, k) filter
  return (int64_t)G.ks[0] * G.ks[1] * G.ks[2];
}
// row = x + X (y + Y (t + T k)), 0 <= row < M
__host__ __device__ inline void synth_decode(const SynthGeom& G, int64_t row, int32_t* x,
                                             int32_t* y, int32_t* t, int32_t* k) {
  const int64_t q0 = row / G.g[0];
  *x = (int32_t)(row - q0 * G.g[0]);
  const int64_t q1 = q0 / G.g[1];
  *y = (int32_t)(q0 - q1 * G.g[1]);
  const int64_t q2 = q1 / G.g[2];
  *t = (int32_t)(q1 - q2 * G.g[2]);
  *k = (int32_t)q2;
}
// (a - b + r) mod g for a, b in [0, g) and 0 <= r < g, without leaving int32 (g may be
// close to 2^31): the tap coordinate of output a for an entry at b, a tap iff below ks
__host__ __device__ inline int32_t synth_tap_coord(int32_t a, int32_t b, int32_t r, int32_t g) {
  int32_t v = a - b;
  if (v < 0) v += g;
  return v >= g - r ? v - (g - r) : v + r;
}
// Can an entry at coordinate e reach an output in [lo, lo + len) along an axis of g points
// with filter radius r?  The sources of those outputs are [lo - r, lo + len + r), circular.
__host__ __device__ inline bool synth_in_window(int32_t e, int32_t lo, int32_t len, int32_t r,
                                                int32_t g) {
  const int64_t span = (int64_t)len + 2 * (int64_t)r;
  return span >= g || synth_tap_coord(e, lo, r, g) < span;   // (e - (lo - r)) mod g
}
// d is column-major [s0, s1, s2, C, K]
__host__ __device__ inline int64_t synth_tap_index(const SynthGeom& G, int32_t i0, int32_t i1,
                                                   int32_t i2, int32_t c, int32_t k) {
  return i0 + (int64_t)G.ks[0] * (i1 + (int64_t)G.ks[1] * (i2 + (int64_t)G.ks[2] *
                                                          (c + (int64_t)G.C * k)));
}
// out is column-major [X, Y, T, C, n]
__host__ __device__ inline int64_t synth_out_index(const SynthGeom& G, int32_t x, int32_t y,
                                                   int32_t t, int32_t c, int64_t col) {
  return x + (int64_t)G.g[0] * (y + (int64_t)G.g[1] * (t + (int64_t)G.g[2] *
                                                       (c + (int64_t)G.C * col)));
}
__host__ __device__ inline int64_t synth_tiles_x(const SynthGeom& G) {
  return (G.g[0] + kSynthTX - 1) / kSynthTX;
}
__host__ __device__ inline int64_t synth_tiles_y(const SynthGeom& G) {
  return (G.g[1] + kSynthTY - 1) / kSynthTY;
}
__host__ __device__ inline int64_t synth_cgroups(const SynthGeom& G) {
  return (G.C + kSynthCG - 1) / kSynthCG;
}
// workgroups of one column: tiles of every t-plane, times the channel groups
__host__ __device__ inline int64_t synth_blocks_per_col(const SynthGeom& G) {
  return synth_tiles_x(G) * synth_tiles_y(G) * G.g[2] * synth_cgroups(G);
}
__host__ __device__ inline int64_t expand_segs(int64_t M) {
  return M > 0 ? (M + kExpandSeg - 1) / kExpandSeg : 1;
}

// ---- synth_codes.hip (every pointer on the device) --------------------------------------
// out[X, Y, T, C, m] of the m columns jc[0 .. m]; jc's values index ir / pr [0, nnz).  *flag
// is set to 1 when a column range or a row is out of range (such entries are skipped).
hipError_t launch_synth_codes(const SynthGeom& G, const double* d, const int64_t* jc,
                              const int64_t* ir, const double* pr, int64_t m, int64_t nnz,
                              double* out, int32_t* flag, hipStream_t st);
// out[M, m] dense; rows strictly ascending inside a column or *flag is set.
hipError_t launch_codes_expand(const int64_t* jc, const int64_t* ir, const double* pr, int64_t M,
                               int64_t m, int64_t nnz, double* out, int32_t* flag,
                               hipStream_t st);

}  // namespace ccsc
