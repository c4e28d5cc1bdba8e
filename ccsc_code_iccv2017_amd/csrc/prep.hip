// The two steps the reference's reconstruction drivers run on their data before they
// filter smooth_init and call a solver (include/ccsc.h lists the call sites):
//
// Nearest-sample fill, [~, idx] = bwdist(a ~= 0); a(a == 0) = a(idx(a == 0)), per
// column-major [H, W] plane, in the separable exact form, all integer:
//   k_fill_cols  r(i, j): the row of the sample of column j nearest to row i, the smaller
//                row on a tie, -1 in a column without a sample.  One wave per column, 64
//                rows per step: a prefix maximum of the sample rows going down (kept in r),
//                then a suffix minimum going up, carried from step to step in a register.
//                r has the image's layout, so both passes read and write it coalesced.
//   k_fill_rows  pixel (i, j) minimises (d2, j') = ((j - j')^2 + (i - r(i, j'))^2, j')
//                lexicographically over the columns j', walking outward from j and stopping
//                once (j - j')^2 exceeds the best d2: that is the minimum of
//                (d2, j', i') over all samples, the smallest column-major index among the
//                nearest.  A wave holds 64 rows of one column, so j' is wave-uniform and
//                every read of r is one contiguous run.  The loop is bounded by W.
// Only non-samples are written to `out` and only samples are read from `in`, so the two
// may be the same array.
//
// Standardisation, nb = (v - mean(v, 2)) ./ std(v, 0, 2) per plane of N contiguous values,
// and its inverse: three streaming passes (sum, squared deviations from the rounded mean,
// normalise) over chunks of kStdChunk values, one workgroup per chunk.  Both sums are
// taken with one tree whose shape depends on N alone: thread t of a chunk adds its 16
// values in index order (pairs 2 (t + 256 r), r ascending), the 256 thread sums are halved
// in LDS (t += t + s, s = 128 .. 1), the chunk sums are stored, and k_std_finish adds them
// with the same two steps (thread t takes chunks t, t + 256, ...).  Values past N are not
// added.  No atomics; the batch, the launch chunks and the entry point never enter.
#include "kernels.hpp"

#include <algorithm>

namespace ccsc {

constexpr int kPrepNT = 256;
constexpr int kFillTileH = 64;                  // rows per wave step and per row-pass tile
constexpr int kFillTileW = kPrepNT / kFillTileH;   // columns (waves) per workgroup
constexpr int kStdChunk = 4096;                 // values per workgroup
constexpr int kStdPer = kStdChunk / kPrepNT;    // values per thread, as pairs
constexpr int64_t kPrepMaxBlocks = (int64_t)1 << 22;   // workgroups per launch
static_assert(kFillTileH == 64, "a wave holds one column's rows");
static_assert(kStdPer % 2 == 0, "threads load pairs");

// ---- nearest-sample fill ------------------------------------------------------------

struct FillArgs {
  int H, W;
  int tH, tW;       // row-pass tiles per plane
};

__device__ __forceinline__ int wave_shift_up(int v, int d, int lane, int fill) {
  const int o = __shfl_up(v, d, 64);
  return lane >= d ? o : fill;
}

__device__ __forceinline__ int wave_shift_down(int v, int d, int lane, int fill) {
  const int o = __shfl_down(v, d, 64);
  return lane + d < 64 ? o : fill;
}

// Workgroup block0 + blockIdx.x: groups of kFillTileW columns, then planes.
__global__ __launch_bounds__(kPrepNT) void k_fill_cols(const double* __restrict__ src,
                                                       int* __restrict__ r, FillArgs a,
                                                       int64_t block0) {
  const int64_t b = block0 + blockIdx.x;
  const int64_t pl = b / a.tW;
  const int j = (int)(b - pl * a.tW) * kFillTileW + (int)(threadIdx.x >> 6);
  if (j >= a.W) return;                          // whole waves leave; no barrier below
  const int lane = threadIdx.x & 63;
  const int64_t col = (pl * a.W + j) * a.H;
  const double* S = src + col;
  int* R = r + col;
  const int steps = (a.H + 63) >> 6;
  constexpr int kNone = 0x7fffffff;
  int carry = -1;                                // last sample row above this step
  for (int s = 0; s < steps; ++s) {
    const int i = s * 64 + lane;
    int v = (i < a.H && S[i] != 0.0) ? i : -1;   // NaN is a sample, -0.0 is not
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = max(v, wave_shift_up(v, d, lane, -1));
    v = max(v, carry);
    carry = __shfl(v, 63, 64);
    if (i < a.H) R[i] = v;
  }
  carry = kNone;                                 // first sample row below this step
  for (int s = steps - 1; s >= 0; --s) {
    const int i = s * 64 + lane;
    const int up = i < a.H ? R[i] : -1;          // this lane's own store
    int v = (i < a.H && up == i) ? i : kNone;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = min(v, wave_shift_down(v, d, lane, kNone));
    v = min(v, carry);
    carry = __shfl(v, 0, 64);
    if (i < a.H) {
      int best = up;                             // -1: none above
      if (v != kNone && (up < 0 || v - i < i - up)) best = v;   // a tie keeps the upper row
      R[i] = best;
    }
  }
}

// Workgroup block0 + blockIdx.x: tiles of kFillTileH x kFillTileW pixels, rows fastest,
// then planes.
__global__ __launch_bounds__(kPrepNT) void k_fill_rows(const double* in, double* out,
                                                       const int* __restrict__ r,
                                                       int* __restrict__ idx, FillArgs a,
                                                       int64_t block0) {
  const int64_t b = block0 + blockIdx.x;
  const int tpp = a.tH * a.tW;
  const int64_t pl = b / tpp;
  const int tile = (int)(b - pl * tpp);
  const int tw = tile / a.tH, th = tile - tw * a.tH;
  const int i = th * kFillTileH + (int)(threadIdx.x & 63);
  const int j = tw * kFillTileW + (int)(threadIdx.x >> 6);
  if (i >= a.H || j >= a.W) return;
  const int64_t plane = pl * a.H * a.W;
  const int* R = r + plane;
  constexpr int kNone = 0x7fffffff;
  int best = kNone, bj = -1, bi = -1;
  const int kmax = max(j, a.W - 1 - j);          // k <= 32767: k * k fits
  for (int k = 0; k <= kmax && k * k <= best; ++k) {
    // j - k before j + k; the compare on (d2, j') makes the order immaterial
    for (int side = 0; side < (k ? 2 : 1); ++side) {
      const int jp = side ? j + k : j - k;
      if (jp < 0 || jp >= a.W) continue;
      const int ri = R[(int64_t)jp * a.H + i];
      if (ri < 0) continue;
      const int di = i - ri;
      const int d2 = k * k + di * di;            // <= 2 * 32767^2 < 2^31
      if (d2 < best || (d2 == best && jp < bj)) best = d2, bj = jp, bi = ri;
    }
  }
  const int q = j * a.H + i;                     // H * W < 2^31
  const int s = bj < 0 ? -1 : bj * a.H + bi;
  if (idx) idx[plane + q] = s;
  if (s < 0 || s == q) {
    if (out != in) out[plane + q] = in[plane + q];
  } else {
    out[plane + q] = in[plane + s];
  }
}

bool nn_fill_ok(int H, int W) {
  return H >= 1 && W >= 1 && H <= kFillMaxExt && W <= kFillMaxExt &&
         (int64_t)H * W < ((int64_t)1 << 31);
}

hipError_t launch_nn_fill(const double* in, const double* known, double* out, int* idx, int* r,
                          int64_t n, int H, int W, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!nn_fill_ok(H, W) || !in || !out || !r || known == out) return hipErrorInvalidValue;
  FillArgs a;
  a.H = H, a.W = W;
  a.tH = (H + kFillTileH - 1) / kFillTileH;
  a.tW = (W + kFillTileW - 1) / kFillTileW;
  const double* src = known ? known : in;
  int64_t total = n * a.tW;
  for (int64_t b0 = 0; b0 < total; b0 += kPrepMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kPrepMaxBlocks, total - b0);
    hipLaunchKernelGGL(k_fill_cols, dim3(nb), dim3(kPrepNT), 0, st, src, r, a, b0);
  }
  total = n * ((int64_t)a.tH * a.tW);
  for (int64_t b0 = 0; b0 < total; b0 += kPrepMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kPrepMaxBlocks, total - b0);
    hipLaunchKernelGGL(k_fill_rows, dim3(nb), dim3(kPrepNT), 0, st, in, out, r, idx, a, b0);
  }
  return hipGetLastError();
}

// ---- standardisation ----------------------------------------------------------------

typedef double dbl2 __attribute__((ext_vector_type(2)));

// A thread's kStdPer values of chunk c of a plane of N: pairs 2 (t + 256 r), r ascending;
// 0 past N.  `fast` (uniform over the workgroup: the plane is 16-byte aligned and the chunk
// is whole) takes them as 16-byte accesses, all issued before the first use.
__device__ __forceinline__ void std_load(const double* X, int64_t e0, int64_t N, bool fast,
                                         double (&v)[kStdPer]) {
  if (fast) {
#pragma unroll
    for (int r = 0; r < kStdPer / 2; ++r) {
      const dbl2 p = *reinterpret_cast<const dbl2*>(X + e0 + 2 * kPrepNT * r);
      v[2 * r] = p.x, v[2 * r + 1] = p.y;
    }
  } else {
#pragma unroll
    for (int r = 0; r < kStdPer; ++r) {
      const int64_t e = e0 + 2 * kPrepNT * (r >> 1) + (r & 1);
      v[r] = e < N ? X[e] : 0.0;
    }
  }
}

__device__ __forceinline__ void std_store(double* O, int64_t e0, int64_t N, bool fast,
                                          const double (&v)[kStdPer]) {
  if (fast) {
#pragma unroll
    for (int r = 0; r < kStdPer / 2; ++r) {
      dbl2 p;
      p.x = v[2 * r], p.y = v[2 * r + 1];
      *reinterpret_cast<dbl2*>(O + e0 + 2 * kPrepNT * r) = p;
    }
  } else {
#pragma unroll
    for (int r = 0; r < kStdPer; ++r) {
      const int64_t e = e0 + 2 * kPrepNT * (r >> 1) + (r & 1);
      if (e < N) O[e] = v[r];
    }
  }
}

// The sum of the 256 thread values, t += t + s for s = 128 .. 1; valid in thread 0.
__device__ __forceinline__ double std_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kPrepNT / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// part[p][c] = sum over chunk c of plane p of x (DEV = false) or of (x - mean[p])^2.
// Workgroup block0 + blockIdx.x: chunks of a plane, then planes.
template <bool DEV>
__global__ __launch_bounds__(kPrepNT) void k_std_partial(const double* __restrict__ x,
                                                         const double* __restrict__ mean,
                                                         double* __restrict__ part, int64_t N,
                                                         int nchunks, int64_t block0) {
  __shared__ double sh[kPrepNT];
  const int64_t b = block0 + blockIdx.x;
  const int64_t p = b / nchunks;
  const int64_t c = b - p * nchunks;
  const double* X = x + p * N;
  const bool fast = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (c + 1) * kStdChunk <= N;
  const double m = DEV ? mean[p] : 0.0;
  const int64_t e0 = c * kStdChunk + 2 * (int64_t)threadIdx.x;
  double v[kStdPer];
  std_load(X, e0, N, fast, v);
  double acc = 0;
#pragma unroll
  for (int r = 0; r < kStdPer; ++r) {
    if (DEV) {
      const double d = v[r] - m;
      if (e0 + 2 * kPrepNT * (r >> 1) + (r & 1) < N) acc = fma(d, d, acc);
    } else {
      acc += v[r];                               // 0 past N
    }
  }
  const double s = std_block_sum(acc, sh);
  if (threadIdx.x == 0) part[b] = s;
}

// One workgroup per plane: stat[p] = (sum of the plane's chunk sums) / N, or, with ROOT,
// sqrt(sum / (N - 1)).
template <bool ROOT>
__global__ __launch_bounds__(kPrepNT) void k_std_finish(const double* __restrict__ part,
                                                        double* __restrict__ stat, int64_t N,
                                                        int nchunks, int64_t block0) {
  __shared__ double sh[kPrepNT];
  const int64_t p = block0 + blockIdx.x;
  const double* P = part + p * nchunks;
  double acc = 0;
  for (int c = threadIdx.x; c < nchunks; c += kPrepNT) acc += P[c];
  const double s = std_block_sum(acc, sh);
  if (threadIdx.x == 0) stat[p] = ROOT ? sqrt(s / (double)(N - 1)) : s / (double)N;
}

// out = (x - mean[p]) / sdev[p] (INV = false: a true division) or x * sdev[p] + mean[p]
// (INV = true: a multiply, then an add, each rounded).  out may be x.
template <bool INV>
__global__ __launch_bounds__(kPrepNT) void k_std_apply(const double* x, double* out,
                                                       const double* __restrict__ mean,
                                                       const double* __restrict__ sdev, int64_t N,
                                                       int nchunks, int64_t block0) {
#pragma clang fp contract(off)
  const int64_t b = block0 + blockIdx.x;
  const int64_t p = b / nchunks;
  const int64_t c = b - p * nchunks;
  const double* X = x + p * N;
  double* O = out + p * N;
  const bool fast = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(O)) & 15) == 0 &&
                    (c + 1) * kStdChunk <= N;
  const double m = mean[p], s = sdev[p];
  const int64_t e0 = c * kStdChunk + 2 * (int64_t)threadIdx.x;
  double v[kStdPer];
  std_load(X, e0, N, fast, v);                   // every load before the first store
#pragma unroll
  for (int r = 0; r < kStdPer; ++r) {
    if (INV) {
      const double t = v[r] * s;
      v[r] = t + m;
    } else {
      v[r] = (v[r] - m) / s;
    }
  }
  std_store(O, e0, N, fast, v);
}

bool standardize_ok(int64_t N) { return N >= 2 && N < ((int64_t)1 << 31); }

int64_t standardize_ws_bytes(int64_t planes, int64_t N) {
  return planes * ((N + kStdChunk - 1) / kStdChunk) * (int64_t)sizeof(double);
}

template <typename K, typename... A>
static void std_launch(K kern, int64_t total, hipStream_t st, A... args) {
  for (int64_t b0 = 0; b0 < total; b0 += kPrepMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kPrepMaxBlocks, total - b0);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(kPrepNT), 0, st, args..., b0);
  }
}

hipError_t launch_standardize(const double* in, double* out, double* mean, double* sdev,
                              int64_t planes, int64_t N, void* workspace, hipStream_t st) {
  if (planes <= 0) return hipSuccess;
  if (!standardize_ok(N) || !in || !out || !mean || !sdev || !workspace)
    return hipErrorInvalidValue;
  const int nchunks = (int)((N + kStdChunk - 1) / kStdChunk);
  double* part = static_cast<double*>(workspace);
  const double* none = nullptr;
  const double* cmean = mean;
  const double* csdev = sdev;
  const double* cpart = part;
  std_launch(k_std_partial<false>, planes * nchunks, st, in, none, part, N, nchunks);
  std_launch(k_std_finish<false>, planes, st, cpart, mean, N, nchunks);
  std_launch(k_std_partial<true>, planes * nchunks, st, in, cmean, part, N, nchunks);
  std_launch(k_std_finish<true>, planes, st, cpart, sdev, N, nchunks);
  std_launch(k_std_apply<false>, planes * nchunks, st, in, out, cmean, csdev, N, nchunks);
  return hipGetLastError();
}

hipError_t launch_unstandardize(const double* in, double* out, const double* mean,
                                const double* sdev, int64_t planes, int64_t N, hipStream_t st) {
  if (planes <= 0) return hipSuccess;
  if (!standardize_ok(N) || !in || !out || !mean || !sdev) return hipErrorInvalidValue;
  const int nchunks = (int)((N + kStdChunk - 1) / kStdChunk);
  std_launch(k_std_apply<true>, planes * nchunks, st, in, out, mean, sdev, N, nchunks);
  return hipGetLastError();
}

}  // namespace ccsc
