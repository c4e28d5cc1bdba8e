// Reconstructions from sparse codes: out[x, y, t, c, j] = sum over the entries e of column j,
// in storage order, of pr[e] * d[i0, i1, i2, c, k_e] with i_a = (p_a - p_a(e) + r_a) mod g_a
// kept when i_a < ks[a] on every axis -- the circular convolution with the filters embedded
// as circshift(padarray(d), -r) -- as a direct sparse convolution, without atomics.
//
//   k_synth_codes    one workgroup per (column, 16 x 16 output tile of one t-plane, group of
//                    kSynthCG channels); a thread owns one output pixel and holds its channel
//                    accumulators in registers.  The workgroup walks the column's entries in
//                    chunks of 256 (coalesced 8-byte loads of ir and pr), every lane decodes
//                    its entry to (x, y, t, k) and tests it against the tile's source window
//                    (the tile grown by r on every axis, circularly); the hits are compacted
//                    in order into an LDS list (ballot, popcount of the lower lanes, the
//                    per-wave counts through LDS, as k_codes_scatter does).  When the list
//                    cannot take another chunk, and at the end, every thread runs down the
//                    list (LDS broadcast reads) and takes one fma(value, tap, acc) per entry
//                    whose footprint covers its pixel; the taps are read through L2 (lanes
//                    along x read consecutive taps of one filter).  The order of the fmas at
//                    an output element is the column's storage order, whatever the chunking
//                    and the other columns of the launch.
//   k_codes_zero     zero-fills the dense [M, m] matrix of k_codes_expand.
//   k_codes_expand   stores each entry at its row; an entry whose row does not exceed its
//                    predecessor's raises the flag (two entries could race otherwise).
// A column range outside [0, nnz] or decreasing and a row outside [0, M) are skipped and
// raise *flag (a plain 4-byte vector store of 1); nothing out of range is read or written.
#include "synth_codes.hpp"

#include <algorithm>

namespace ccsc {

typedef unsigned long long u64;
constexpr int64_t kSynthMaxBlocks = (int64_t)1 << 22;   // workgroups per launch

struct SynthHit {
  int32_t x, y;      // the entry's position in the plane
  int64_t base;      // tap index of (i0, i1) = (0, 0), channel 0: i2 and k folded in
};

__global__ __launch_bounds__(kSynthNT) void k_synth_codes(
    SynthGeom G, const double* __restrict__ d, const int64_t* __restrict__ jc,
    const int64_t* __restrict__ ir, const double* __restrict__ pr, int64_t nnz,
    double* __restrict__ out, int32_t* __restrict__ flag, int64_t block0) {
  __shared__ SynthHit hq[kSynthList];
  __shared__ double hv[kSynthList];
  __shared__ int wcnt[2][kSynthNT / 64];

  // block -> (column, channel group, t, tile y, tile x), x fastest
  int64_t b = block0 + blockIdx.x;
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
  const bool mine = px < X && py < Y;
  const int64_t M = synth_rows(G), S = synth_taps(G);

  double acc[kSynthCG];
#pragma unroll
  for (int c = 0; c < kSynthCG; ++c) acc[c] = 0.0;

  auto accumulate = [&](int cnt) {
    if (!mine) return;
    for (int h = 0; h < cnt; ++h) {
      const SynthHit q = hq[h];
      const int32_t i0 = synth_tap_coord(px, q.x, r0, X);
      const int32_t i1 = synth_tap_coord(py, q.y, r1, Y);
      if (i0 >= G.ks[0] || i1 >= G.ks[1]) continue;
      const double v = hv[h];
      const double* tap = d + (q.base + i0 + (int64_t)G.ks[0] * i1);
#pragma unroll
      for (int c = 0; c < kSynthCG; ++c)
        if (c0 + c < G.C) acc[c] = fma(v, tap[(int64_t)c * S], acc[c]);
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
    SynthHit q{};
    double v = 0.0;
    if (e < hi) {
      const int64_t row = ir[e];
      v = pr[e];
      if (row < 0 || row >= M) {
        *flag = 1;
      } else {
        int32_t ex, ey, et, ek;
        synth_decode(G, row, &ex, &ey, &et, &ek);
        const int32_t i2 = synth_tap_coord(t, et, r2, T);
        hit = i2 < G.ks[2] && synth_in_window(ex, x0, lx, r0, X) &&
              synth_in_window(ey, y0, ly, r1, Y);
        q.x = ex;
        q.y = ey;
        q.base = synth_tap_index(G, 0, 0, i2, c0, ek);
      }
    }
    const u64 mask = __ballot(hit);
    if (lane == 0) wcnt[par][wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSynthNT / 64; ++w) {
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

  if (mine) {
#pragma unroll
    for (int c = 0; c < kSynthCG; ++c)
      if (c0 + c < G.C) out[synth_out_index(G, px, py, t, c0 + c, col)] = acc[c];
  }
}

__global__ __launch_bounds__(kSynthNT) void k_codes_zero(double* __restrict__ out, int64_t total,
                                                         int64_t block0) {
  const int64_t i = (block0 + blockIdx.x) * kSynthNT + threadIdx.x;
  if (i < total) out[i] = 0.0;
}

__global__ __launch_bounds__(kSynthNT) void k_codes_expand(
    const int64_t* __restrict__ jc, const int64_t* __restrict__ ir, const u64* __restrict__ pr,
    int64_t M, int64_t nnz, u64* __restrict__ out, int32_t* __restrict__ flag, int64_t block0) {
  const int64_t b = block0 + blockIdx.x;
  const int64_t segs = expand_segs(M);
  const int64_t col = b / segs, seg = b - col * segs;
  const int64_t lo = jc[col], hi = jc[col + 1];
  // strictly ascending rows below M: at most M entries
  if (lo < 0 || hi > nnz || hi < lo || hi - lo > M) {
    if (threadIdx.x == 0) *flag = 1;
    return;
  }
  const int64_t s0 = lo + seg * kExpandSeg, s1 = min(hi, s0 + kExpandSeg);
  for (int64_t e = s0 + threadIdx.x; e < s1; e += kSynthNT) {
    const int64_t row = ir[e];
    const bool ok = row >= 0 && row < M && (e == lo || ir[e - 1] < row);
    if (ok) out[col * M + row] = pr[e];
    else *flag = 1;
  }
}

template <typename K, typename... A>
static void synth_launch(K kern, int64_t total, hipStream_t st, A... args) {
  for (int64_t b0 = 0; b0 < total; b0 += kSynthMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kSynthMaxBlocks, total - b0);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(kSynthNT), 0, st, args..., b0);
  }
}

hipError_t launch_synth_codes(const SynthGeom& G, const double* d, const int64_t* jc,
                              const int64_t* ir, const double* pr, int64_t m, int64_t nnz,
                              double* out, int32_t* flag, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  if (!d || !jc || !out || !flag || nnz < 0 || (nnz > 0 && (!ir || !pr)))
    return hipErrorInvalidValue;
  for (int a = 0; a < 3; ++a)
    if (G.g[a] < 1 || G.ks[a] < 1 || G.ks[a] % 2 == 0 || G.ks[a] > G.g[a])
      return hipErrorInvalidValue;
  if (G.C < 1 || G.K < 1 || synth_rows(G) >= kSynthMaxRows) return hipErrorInvalidValue;
  synth_launch(k_synth_codes, m * synth_blocks_per_col(G), st, G, d, jc, ir, pr, nnz, out, flag);
  return hipGetLastError();
}

hipError_t launch_codes_expand(const int64_t* jc, const int64_t* ir, const double* pr, int64_t M,
                               int64_t m, int64_t nnz, double* out, int32_t* flag,
                               hipStream_t st) {
  if (m <= 0 || M <= 0) return hipSuccess;
  if (!jc || !out || !flag || nnz < 0 || (nnz > 0 && (!ir || !pr)) || M >= kSynthMaxRows)
    return hipErrorInvalidValue;
  const int64_t total = M * m;
  synth_launch(k_codes_zero, (total + kSynthNT - 1) / kSynthNT, st, out, total);
  synth_launch(k_codes_expand, m * expand_segs(M), st, jc, ir, reinterpret_cast<const u64*>(pr),
               M, nnz, reinterpret_cast<u64*>(out), flag);
  return hipGetLastError();
}

}  // namespace ccsc
