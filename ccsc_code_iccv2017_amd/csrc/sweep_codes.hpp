// Threshold sweep of sparse codes against the data (sweep_codes.hip): for every threshold
// eps[e] and column j of a compressed sparse column matrix, in one pass over the entries,
//   nnz[e, j] = #{entries with !(|v| <= eps[e])},  l1[e, j] = sum |v| over them,
//   sse[e, j] = sum over the compared region of (b - R_e)^2,
// R_e being the reconstruction ccsc_synthesize defines, restricted to those entries and never
// stored.  The geometry and the index arithmetic are synth_codes.hpp's; what is added here is
// the threshold class of a value, the layout of b and the launchers.
#pragma once

#include "synth_codes.hpp"

namespace ccsc {

constexpr int kSweepEG = 8;    // thresholds of one launch: a thread holds kSweepEG x kSynthCG sums

// the thresholds of one launch, ascending (the host sorts), by value to the kernels
struct SweepEps {
  double v[kSweepEG];
  int32_t n;    // 1 .. kSweepEG
};

// The threshold class of a value: how many of eps[0 .. n), n <= kSweepEG, it survives, an entry
// surviving eps iff !(|v| <= eps) -- the predicate of k_codes_count / k_codes_scatter, so a NaN
// survives every threshold.  The predicate is monotone in eps: over an ascending list the
// survived thresholds are the first `class` ones.  (ccsc_test_sweep_class evaluates it on the
// host, group by group.)
__host__ __device__ inline int32_t sweep_class(const double* eps, int32_t n, double v) {
  const double a = v < 0 ? -v : v;   // |v|; a NaN stays a NaN
  int32_t m = 0;
#pragma unroll
  for (int32_t e = 0; e < kSweepEG; ++e)   // n <= kSweepEG; a fixed trip count unrolls
    m += e < n && !(a <= eps[e]) ? 1 : 0;
  return m;
}

// b is column-major [g - 2 crop r, C, n]: the whole grid (crop = 0) or its interior
__host__ __device__ inline int64_t sweep_b_extent(const SynthGeom& G, int a, int32_t crop) {
  return G.g[a] - (crop ? 2 * (G.ks[a] / 2) : 0);
}
__host__ __device__ inline int64_t sweep_b_col_elems(const SynthGeom& G, int32_t crop) {
  return sweep_b_extent(G, 0, crop) * sweep_b_extent(G, 1, crop) * sweep_b_extent(G, 2, crop) *
         G.C;
}
// is grid coordinate p of axis a compared?
__host__ __device__ inline bool sweep_compared(const SynthGeom& G, int a, int32_t crop,
                                               int32_t p) {
  const int32_t r = crop ? G.ks[a] / 2 : 0;
  return p >= r && p < G.g[a] - r;
}
// index into b of the compared grid point (x, y, t), channel c, column col
__host__ __device__ inline int64_t sweep_b_index(const SynthGeom& G, int32_t crop, int32_t x,
                                                 int32_t y, int32_t t, int32_t c, int64_t col) {
  const int32_t r0 = crop ? G.ks[0] / 2 : 0, r1 = crop ? G.ks[1] / 2 : 0,
                r2 = crop ? G.ks[2] / 2 : 0;
  return (x - r0) + sweep_b_extent(G, 0, crop) * ((y - r1) + sweep_b_extent(G, 1, crop) *
         ((t - r2) + sweep_b_extent(G, 2, crop) * (c + (int64_t)G.C * col)));
}

// ---- sweep_codes.hip (every pointer on the device) ---------------------------------------
// One group of E.n ascending thresholds over the m columns jc[0 .. m].  nnz_out / l1_out /
// sse_out are [Etot, m], e fastest; threshold e of the group writes row dst[e] (host array,
// 0 <= dst[e] < Etot) and no other row is touched.  part is workspace of
// m * synth_blocks_per_col(G) * kSweepEG doubles.  *flag as in launch_synth_codes.
hipError_t launch_sweep_codes(const SynthGeom& G, const SweepEps& E, const int64_t* dst,
                              int64_t Etot, const double* d, const int64_t* jc,
                              const int64_t* ir, const double* pr, int64_t m, int64_t nnz,
                              const double* b, int32_t crop, double* part, int64_t* nnz_out,
                              double* l1_out, double* sse_out, int32_t* flag, hipStream_t st);

}  // namespace ccsc
