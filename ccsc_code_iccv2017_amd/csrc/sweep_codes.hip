// Threshold sweep of sparse codes against the data: per threshold eps[e] and column j, the
// number of entries with !(|v| <= eps[e]), their l1 mass and sum (b - R_e)^2 over the compared
// region, R_e being k_synth_codes's reconstruction from those entries alone -- formed in
// registers, never stored.  No floating-point atomics; every sum has a fixed order.
//
//   k_sweep_codes   k_synth_codes's shape: one workgroup per (column, 16 x 16 tile of one
//                   t-plane, group of kSynthCG channels), the column walked in chunks of 256,
//                   the hits compacted in order into an LDS list.  Each hit also carries its
//                   threshold class m (sweep_class over the launch's ascending thresholds: the
//                   thresholds it survives are the first m); an entry of class 0 never enters
//                   the list; m rides in the hit's 16-byte record (the tap base fits 32 bits).
//                   A thread holds EG x kSynthCG accumulators (EG = 1, 2, 4 or 8 rows, the
//                   smallest instance that takes the launch's thresholds) and a hit updates
//                   those of thresholds 0 .. m - 1; m is an LDS broadcast made scalar
//                   (readfirstlane), so the update is a chain of scalar branches.  At an
//                   output element the fmas of threshold e are those of the surviving entries
//                   in the column's storage order: the bits of k_synth_codes on the filtered
//                   triple.  The epilogue loads the thread's elements of b, squares b - acc
//                   (channels in order), and reduces per threshold over the workgroup: a
//                   shuffle tree inside each wave, then the four waves in order.  The
//                   partial goes to part[block][e].  A workgroup whose tile lies outside the
//                   compared region stores +0.0 partials and walks nothing.
//   k_sweep_sum     sse[e, column] = the column's partials summed in block order.
//   k_sweep_stats   one workgroup per column: thread i takes entries i, i + 256, ... of the
//                   column in order into its per-threshold count and sum |v|, then the same
//                   workgroup reduction.  The counts are exact (int64).
// A column range outside [0, nnz] or decreasing and a row outside [0, M) are skipped and raise
// *flag (a plain 4-byte vector store of 1); nothing out of range is read or written.
#include "sweep_codes.hpp"

#include <algorithm>

namespace ccsc {

typedef unsigned long long u64;
constexpr int64_t kSweepMaxBlocks = (int64_t)1 << 22;   // workgroups per launch
constexpr int kSweepWaves = kSynthNT / 64;
constexpr int kSweepSumCols = kSynthNT / kSweepEG;       // columns of one k_sweep_sum workgroup

struct SweepHit {   // 16 bytes: one LDS broadcast read per hit
  int32_t x, y;      // the entry's position in the plane
  int32_t base;      // tap index of (i0, i1) = (0, 0), channel 0: i2 and k folded in (the
                     // filters hold fewer than 2^31 values)
  int32_t m;         // threshold class, 1 .. E.n
};

// where the results of the launch's thresholds go: out[dst[e] + E * column]
struct SweepDst {
  int64_t dst[kSweepEG];
  int64_t E;
};

// lane 0 of the wave gets the wave's sum by a fixed tree
__device__ inline double sweep_wave_sum(double s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off);
  return s;
}
__device__ inline int64_t sweep_wave_sum(int64_t s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_down(s, off);
  return s;
}

// EG: the accumulator rows the instance holds, E.n <= EG <= kSweepEG (the host picks the
// smallest of 1, 2, 4, 8: a sweep of one threshold keeps k_synth_codes's register budget)
template <int EG>
__global__ __launch_bounds__(kSynthNT) void k_sweep_codes(
    SynthGeom G, SweepEps E, const double* __restrict__ d, const int64_t* __restrict__ jc,
    const int64_t* __restrict__ ir, const double* __restrict__ pr, int64_t nnz,
    const double* __restrict__ bdat, int32_t crop, double* __restrict__ part,
    int32_t* __restrict__ flag, int64_t block0) {
  __shared__ SweepHit hq[kSynthList];
  __shared__ double hv[kSynthList];
  __shared__ int wcnt[2][kSweepWaves];
  __shared__ double wsum[EG][kSweepWaves];

  // block -> (column, channel group, t, tile y, tile x), x fastest
  const int64_t blk = block0 + blockIdx.x;
  int64_t b = blk;
  const int64_t ntx = synth_tiles_x(G), nty = synth_tiles_y(G);
  const int32_t tx = (int32_t)(b % ntx);
  b /= ntx;
  const int32_t ty = (int32_t)(b % nty);
  b /= nty;
  const int32_t t = (int32_t)(b % G.g[2]);
  b /= G.g[2];
  const int64_t ncg = synth_cgroups(G);
  const int32_t c0 = (int32_t)(b % ncg) * kSynthCG;
  const int64_t col = b / ncg;

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int32_t X = G.g[0], Y = G.g[1], T = G.g[2];
  const int32_t r0 = G.ks[0] / 2, r1 = G.ks[1] / 2, r2 = G.ks[2] / 2;
  const int32_t x0 = tx * kSynthTX, y0 = ty * kSynthTY;
  const int32_t lx = min(kSynthTX, X - x0), ly = min(kSynthTY, Y - y0);
  const int32_t px = x0 + (int32_t)(threadIdx.x % kSynthTX);
  const int32_t py = y0 + (int32_t)(threadIdx.x / kSynthTX);
  // the thread's pixel exists and is compared
  const bool mine = px < X && py < Y && sweep_compared(G, 0, crop, px) &&
                    sweep_compared(G, 1, crop, py);
  const int ne = E.n;

  // no pixel of the tile is compared (crop: the tile or the plane lies in the border)
  const int32_t cr0 = crop ? r0 : 0, cr1 = crop ? r1 : 0;
  if (!sweep_compared(G, 2, crop, t) || x0 + lx <= cr0 || x0 >= X - cr0 || y0 + ly <= cr1 ||
      y0 >= Y - cr1) {
    if ((int)threadIdx.x < ne) part[blk * kSweepEG + threadIdx.x] = 0.0;
    return;
  }
  const int64_t M = synth_rows(G), S = synth_taps(G);

  double acc[EG][kSynthCG];
#pragma unroll
  for (int e = 0; e < EG; ++e)
#pragma unroll
    for (int c = 0; c < kSynthCG; ++c) acc[e][c] = 0.0;

  auto accumulate = [&](int cnt) {
    if (!mine) return;
    for (int h = 0; h < cnt; ++h) {
      const SweepHit q = hq[h];
      const int32_t i0 = synth_tap_coord(px, q.x, r0, X);
      const int32_t i1 = synth_tap_coord(py, q.y, r1, Y);
      if (i0 >= G.ks[0] || i1 >= G.ks[1]) continue;
      const double v = hv[h];
      const int m = __builtin_amdgcn_readfirstlane(q.m);   // the same in every lane
      const double* tap = d + ((int64_t)q.base + i0 + (int64_t)G.ks[0] * i1);
      double w[kSynthCG];
#pragma unroll
      for (int c = 0; c < kSynthCG; ++c) w[c] = c0 + c < G.C ? tap[(int64_t)c * S] : 0.0;
#pragma unroll
      for (int e = 0; e < EG; ++e) {
        if (e >= m) break;
#pragma unroll
        for (int c = 0; c < kSynthCG; ++c)
          if (c0 + c < G.C) acc[e][c] = fma(v, w[c], acc[e][c]);
      }
    }
  };

  int64_t lo = jc[col], hi = jc[col + 1];
  if (lo < 0 || hi > nnz || hi < lo) {   // a malformed column is an empty one
    if (threadIdx.x == 0) *flag = 1;
    lo = hi = 0;
  }
  const u64 below = ((u64)1 << lane) - 1;
  int cnt = 0, par = 0;
  for (int64_t e0 = lo; e0 < hi; e0 += kSynthNT) {
    if (cnt + kSynthNT > kSynthList) {   // the list could overflow: flush it
      __syncthreads();
      accumulate(cnt);
      __syncthreads();
      cnt = 0;
    }
    const int64_t e = e0 + threadIdx.x;
    bool hit = false;
    SweepHit q{};
    double v = 0.0;
    int32_t m = 0;
    if (e < hi) {
      const int64_t row = ir[e];
      v = pr[e];
      if (row < 0 || row >= M) {
        *flag = 1;
      } else {
        m = sweep_class(E.v, ne, v);
        int32_t ex, ey, et, ek;
        synth_decode(G, row, &ex, &ey, &et, &ek);
        const int32_t i2 = synth_tap_coord(t, et, r2, T);
        hit = m > 0 && i2 < G.ks[2] && synth_in_window(ex, x0, lx, r0, X) &&
              synth_in_window(ey, y0, ly, r1, Y);
        q.x = ex;
        q.y = ey;
        q.base = (int32_t)synth_tap_index(G, 0, 0, i2, c0, ek);
        q.m = m;
      }
    }
    const u64 mask = __ballot(hit);
    if (lane == 0) wcnt[par][wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSweepWaves; ++w) {
      const int n = wcnt[par][w];
      if (w < wave) before += n;
      total += n;
    }
    if (hit) {
      const int slot = cnt + before + __popcll(mask & below);   // < cnt + 256 <= kSynthList
      hq[slot] = q;
      hv[slot] = v;
    }
    cnt += total;
    par ^= 1;   // the counts of the step after next are written behind the next barrier
  }
  __syncthreads();
  accumulate(cnt);

  // (b - R_e)^2 of the thread's elements, channels in order
  double bv[kSynthCG];
#pragma unroll
  for (int c = 0; c < kSynthCG; ++c)
    bv[c] = mine && c0 + c < G.C ? bdat[sweep_b_index(G, crop, px, py, t, c0 + c, col)] : 0.0;
#pragma unroll
  for (int e = 0; e < EG; ++e) {
    if (e >= ne) break;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < kSynthCG; ++c) {
      if (mine && c0 + c < G.C) {
        const double r = bv[c] - acc[e][c];
        s = fma(r, r, s);
      }
    }
    s = sweep_wave_sum(s);
    if (lane == 0) wsum[e][wave] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < ne) {
    double s = wsum[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kSweepWaves; ++w) s += wsum[threadIdx.x][w];
    part[blk * kSweepEG + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kSynthNT) void k_sweep_sum(
    const double* __restrict__ part, int64_t bpc, int64_t m, int32_t ne, SweepDst D,
    double* __restrict__ sse, int64_t block0) {
  const int64_t col = (block0 + blockIdx.x) * kSweepSumCols + threadIdx.x / kSweepEG;
  const int e = threadIdx.x % kSweepEG;
  if (col >= m || e >= ne) return;
  const double* p = part + col * bpc * kSweepEG + e;
  double s = p[0];
  for (int64_t k = 1; k < bpc; ++k) s += p[k * kSweepEG];
  sse[D.dst[e] + D.E * col] = s;
}

__global__ __launch_bounds__(kSynthNT) void k_sweep_stats(
    SweepEps E, const int64_t* __restrict__ jc, const int64_t* __restrict__ ir,
    const double* __restrict__ pr, int64_t M, int64_t nnz, SweepDst D,
    int64_t* __restrict__ nnz_out, double* __restrict__ l1_out, int32_t* __restrict__ flag,
    int64_t block0) {
  __shared__ double wl[kSweepEG][kSweepWaves];
  __shared__ int64_t wn[kSweepEG][kSweepWaves];
  const int64_t col = block0 + blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ne = E.n;
  int64_t lo = jc[col], hi = jc[col + 1];
  if (lo < 0 || hi > nnz || hi < lo) {
    if (threadIdx.x == 0) *flag = 1;
    lo = hi = 0;
  }
  double l[kSweepEG];
  int64_t n[kSweepEG];
#pragma unroll
  for (int e = 0; e < kSweepEG; ++e) {
    l[e] = 0.0;
    n[e] = 0;
  }
  for (int64_t i = lo + threadIdx.x; i < hi; i += kSynthNT) {
    const int64_t row = ir[i];
    if (row < 0 || row >= M) {
      *flag = 1;
      continue;
    }
    const double a = fabs(pr[i]);
    const int32_t m = sweep_class(E.v, ne, a);
#pragma unroll
    for (int e = 0; e < kSweepEG; ++e) {
      if (e < m) {
        l[e] += a;
        n[e] += 1;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < kSweepEG; ++e) {
    if (e >= ne) break;
    const double s = sweep_wave_sum(l[e]);
    const int64_t c = sweep_wave_sum(n[e]);
    if (lane == 0) {
      wl[e][wave] = s;
      wn[e][wave] = c;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < ne) {
    double s = wl[threadIdx.x][0];
    int64_t c = wn[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kSweepWaves; ++w) {
      s += wl[threadIdx.x][w];
      c += wn[threadIdx.x][w];
    }
    l1_out[D.dst[threadIdx.x] + D.E * col] = s;
    nnz_out[D.dst[threadIdx.x] + D.E * col] = c;
  }
}

template <typename K, typename... A>
static void sweep_launch(K kern, int64_t total, hipStream_t st, A... args) {
  for (int64_t b0 = 0; b0 < total; b0 += kSweepMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kSweepMaxBlocks, total - b0);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(kSynthNT), 0, st, args..., b0);
  }
}

hipError_t launch_sweep_codes(const SynthGeom& G, const SweepEps& E, const int64_t* dst,
                              int64_t Etot, const double* d, const int64_t* jc,
                              const int64_t* ir, const double* pr, int64_t m, int64_t nnz,
                              const double* b, int32_t crop, double* part, int64_t* nnz_out,
                              double* l1_out, double* sse_out, int32_t* flag, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  if (!d || !jc || !b || !part || !dst || !nnz_out || !l1_out || !sse_out || !flag || nnz < 0 ||
      (nnz > 0 && (!ir || !pr)))
    return hipErrorInvalidValue;
  for (int a = 0; a < 3; ++a)
    if (G.g[a] < 1 || G.ks[a] < 1 || G.ks[a] % 2 == 0 || G.ks[a] > G.g[a])
      return hipErrorInvalidValue;
  if (G.C < 1 || G.K < 1 || synth_rows(G) >= kSynthMaxRows ||
      synth_taps(G) * G.C >= kSynthMaxTaps || synth_taps(G) * G.C * G.K >= kSynthMaxTaps)
    return hipErrorInvalidValue;
  if (E.n < 1 || E.n > kSweepEG || Etot < E.n) return hipErrorInvalidValue;
  SweepDst D{};
  D.E = Etot;
  for (int e = 0; e < E.n; ++e) {
    if (dst[e] < 0 || dst[e] >= Etot) return hipErrorInvalidValue;
    if (e > 0 && !(E.v[e - 1] <= E.v[e])) return hipErrorInvalidValue;   // ascending, no NaN
    D.dst[e] = dst[e];
  }
  const int64_t bpc = synth_blocks_per_col(G);
  const int32_t cr = crop ? 1 : 0;
  if (E.n <= 1)
    sweep_launch(k_sweep_codes<1>, m * bpc, st, G, E, d, jc, ir, pr, nnz, b, cr, part, flag);
  else if (E.n <= 2)
    sweep_launch(k_sweep_codes<2>, m * bpc, st, G, E, d, jc, ir, pr, nnz, b, cr, part, flag);
  else if (E.n <= 4)
    sweep_launch(k_sweep_codes<4>, m * bpc, st, G, E, d, jc, ir, pr, nnz, b, cr, part, flag);
  else
    sweep_launch(k_sweep_codes<kSweepEG>, m * bpc, st, G, E, d, jc, ir, pr, nnz, b, cr, part,
                 flag);
  sweep_launch(k_sweep_sum, (m + kSweepSumCols - 1) / kSweepSumCols, st,
               (const double*)part, bpc, m, E.n, D, sse_out);
  sweep_launch(k_sweep_stats, m, st, E, jc, ir, pr, synth_rows(G), nnz, D, nnz_out, l1_out, flag);
  return hipGetLastError();
}

}  // namespace ccsc
