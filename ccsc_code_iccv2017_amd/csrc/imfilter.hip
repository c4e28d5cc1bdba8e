// imfilter(A, k, 'same', 'conv', boundary): the call with which the reference's drivers
// compute smooth_init and blur their data (include/ccsc.h lists the call sites), for n
// column-major fp64 arrays [H, W, T] and one kernel [kh, kw, kt] of odd extents:
//
//   out[i, j, t] = sum_{u,v,s} k[u, v, s] * A_pad[i + c1 - u, j + c2 - v, t + c3 - s],
//   c = (extent - 1) / 2
//
// One direct route (no separable one: fspecial('gaussian') is rank one only to rounding,
// and two routes would be two sets of numerics).  One workgroup of 256 threads per
// 32 x 32 output tile of one plane t.  Per t-tap s the tile of plane map(t + c3 - s) with
// its (kh - 1) x (kw - 1) halo is staged in LDS, the boundary map applied while it is
// loaded, so the accumulate reads LDS only; for kt > 1 the plane is restaged per s (the
// re-reads hit L2).  A thread owns row h of four adjacent columns and walks the staged
// columns from right to left: one LDS read feeds the four outputs, whose tap column v
// then ascends, and within a column u ascends.  Every output is therefore the sum
// s outer, v middle, u inner, ascending, one fma per tap from 0, whatever the tile, the
// batch or the launch chunk: bitwise reproducible, no atomics.  The taps are read with
// wave-uniform indices from a small device buffer that holds them as [s][u][v], v
// fastest, so the four taps k[u, v .. v + 3] that meet one LDS read are adjacent.
#include "kernels.hpp"

#include "../../include/ccsc.h"

#include <algorithm>

namespace ccsc {

constexpr int kImfTile = 32;                    // tile edge in dims 1 and 2
constexpr int kImfNT = 256;
constexpr int kImfOut = kImfTile * kImfTile / kImfNT;   // outputs (adjacent columns) per thread
static_assert(kImfOut == 4, "k_imfilter dispatches on the output ranges of 4 columns");
constexpr int64_t kImfMaxBlocks = (int64_t)1 << 22;     // workgroups per launch

struct ImfArgs {
  int H, W, T;
  int kh, kw, kt;
  int tH, tW;       // tiles per plane
  int boundary;
};

// Index of the sample that A_pad reads at i (any i) of an extent n; -1: the sample is 0.
__device__ __forceinline__ int64_t imf_map(int64_t i, int n, int boundary) {
  if (i >= 0 && i < n) return i;
  if (boundary == CCSC_PAD_ZERO) return -1;
  if (boundary == CCSC_PAD_REPLICATE) return i < 0 ? 0 : n - 1;
  const int64_t p = 2 * (int64_t)n;             // symmetric: period 2n, second half mirrored
  int64_t m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

// One staged column against the tap column it meets in each of the outputs LO .. HI:
// col points at the sample of tap row 0 (rows descend as u ascends); output i meets tap
// column v0 + i of ks ([u][v], v fastest: the outputs' taps of a row u are adjacent).
template <int LO, int HI>
__device__ __forceinline__ void imf_column(const double* col, const double* __restrict__ ks,
                                           int v0, int kh, int kw, double (&acc)[kImfOut]) {
#pragma unroll 2
  for (int u = 0; u < kh; ++u) {
    const double x = col[-u];
#pragma unroll
    for (int i = LO; i <= HI; ++i) acc[i] = fma(ks[u * kw + v0 + i], x, acc[i]);
  }
}

// Workgroup block0 + blockIdx.x: tiles of a plane h fastest, then planes t, then images.
__global__ __launch_bounds__(kImfNT) void k_imfilter(const double* __restrict__ in,
                                                     double* __restrict__ out,
                                                     const double* __restrict__ taps, ImfArgs a,
                                                     int64_t block0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* pad = reinterpret_cast<double*>(smem);   // [WP][HP], h fastest
  const int HP = kImfTile + a.kh - 1, WP = kImfTile + a.kw - 1;
  const int64_t b = block0 + blockIdx.x;
  const int tpp = a.tH * a.tW;
  const int64_t pl = b / tpp;
  const int tile = (int)(b - pl * tpp);
  const int64_t img = pl / a.T;
  const int t = (int)(pl - img * a.T);
  const int tw = tile / a.tH, th = tile - tw * a.tH;
  const int h0 = th * kImfTile, w0 = tw * kImfTile;
  const int64_t N = (int64_t)a.H * a.W * a.T;
  const double* I = in + img * N;
  // staging: lane lh holds one padded row (HP <= 62), the four waves share the columns
  const int lh = threadIdx.x & 63, lw = threadIdx.x >> 6;
  const int64_t mh = lh < HP ? imf_map((int64_t)h0 - (a.kh - 1) / 2 + lh, a.H, a.boundary) : -1;
  // accumulate: row h of columns wq .. wq + kImfOut - 1 of the tile
  const int h = threadIdx.x & (kImfTile - 1);
  const int wq = (threadIdx.x / kImfTile) * kImfOut;
  double acc[kImfOut];
#pragma unroll
  for (int i = 0; i < kImfOut; ++i) acc[i] = 0;
  for (int s = 0; s < a.kt; ++s) {
    const int64_t mt = imf_map((int64_t)t + (a.kt - 1) / 2 - s, a.T, a.boundary);
    if (s) __syncthreads();                      // the previous plane has been read
    if (lh < HP)
      for (int w = lw; w < WP; w += kImfNT / 64) {
        const int64_t mw = imf_map((int64_t)w0 - (a.kw - 1) / 2 + w, a.W, a.boundary);
        double x = 0;
        if (mh >= 0 && mw >= 0 && mt >= 0) x = I[(mt * a.W + mw) * a.H + mh];
        pad[w * HP + lh] = x;
      }
    __syncthreads();
    const double* ks = taps + (int64_t)s * a.kh * a.kw;      // [u][v], v fastest
    // staged column wq + cr meets output i at tap column v = kw - 1 - cr + i
    for (int cr = a.kw + kImfOut - 2; cr >= 0; --cr) {
      const int v0 = a.kw - 1 - cr;
      const double* col = pad + (wq + cr) * HP + h + a.kh - 1;
      // outputs lo .. hi have a tap in this column (all of them away from the kernel's edges)
      const int lo = v0 < 0 ? -v0 : 0, hi = min(kImfOut - 1, a.kw - 1 - v0);
      switch (lo * kImfOut + hi) {
        case 0: imf_column<0, 0>(col, ks, v0, a.kh, a.kw, acc); break;
        case 1: imf_column<0, 1>(col, ks, v0, a.kh, a.kw, acc); break;
        case 2: imf_column<0, 2>(col, ks, v0, a.kh, a.kw, acc); break;
        case 3: imf_column<0, 3>(col, ks, v0, a.kh, a.kw, acc); break;
        case 5: imf_column<1, 1>(col, ks, v0, a.kh, a.kw, acc); break;
        case 6: imf_column<1, 2>(col, ks, v0, a.kh, a.kw, acc); break;
        case 7: imf_column<1, 3>(col, ks, v0, a.kh, a.kw, acc); break;
        case 10: imf_column<2, 2>(col, ks, v0, a.kh, a.kw, acc); break;
        case 11: imf_column<2, 3>(col, ks, v0, a.kh, a.kw, acc); break;
        case 15: imf_column<3, 3>(col, ks, v0, a.kh, a.kw, acc); break;
      }
    }
  }
  if (h0 + h < a.H) {
    double* O = out + img * N + ((int64_t)t * a.W + w0 + wq) * a.H + h0 + h;
#pragma unroll
    for (int i = 0; i < kImfOut; ++i)
      if (w0 + wq + i < a.W) O[(int64_t)i * a.H] = acc[i];
  }
}

bool imfilter_ok(const int dims[3], const int kdims[3]) {
  int64_t pix = 1, ntaps = 1;
  for (int i = 0; i < 3; ++i) {
    if (dims[i] < 1 || kdims[i] < 1 || kdims[i] > kImfMaxExt || kdims[i] % 2 == 0) return false;
    pix *= dims[i];
    ntaps *= kdims[i];
    if (pix >= ((int64_t)1 << 31)) return false;
  }
  return ntaps <= kImfMaxTaps;
}

void imfilter_pack_taps(const double* k, const int kdims[3], double* packed) {
  const int kh = kdims[0], kw = kdims[1], kt = kdims[2];
  for (int s = 0; s < kt; ++s)
    for (int u = 0; u < kh; ++u)
      for (int v = 0; v < kw; ++v)
        packed[((size_t)s * kh + u) * kw + v] = k[((size_t)s * kw + v) * kh + u];
}

hipError_t launch_imfilter(const double* in, double* out, int64_t n, const int dims[3],
                           const double* taps, const int kdims[3], int boundary,
                           hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!imfilter_ok(dims, kdims) || boundary < CCSC_PAD_SYMMETRIC || boundary > CCSC_PAD_ZERO ||
      !in || !out || !taps || in == out)
    return hipErrorInvalidValue;
  ImfArgs a;
  a.H = dims[0], a.W = dims[1], a.T = dims[2];
  a.kh = kdims[0], a.kw = kdims[1], a.kt = kdims[2];
  a.tH = (a.H + kImfTile - 1) / kImfTile;
  a.tW = (a.W + kImfTile - 1) / kImfTile;
  a.boundary = boundary;
  const size_t lds = (size_t)(kImfTile + a.kh - 1) * (kImfTile + a.kw - 1) * sizeof(double);
  const int64_t total = n * a.T * ((int64_t)a.tH * a.tW);
  for (int64_t b0 = 0; b0 < total; b0 += kImfMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kImfMaxBlocks, total - b0);
    hipLaunchKernelGGL(k_imfilter, dim3(nb), dim3(kImfNT), lds, st, in, out, taps, a, b0);
  }
  return hipGetLastError();
}

}  // namespace ccsc
