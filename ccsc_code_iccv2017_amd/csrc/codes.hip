// Dense codes -> compressed sparse columns: keep the entries with !(|a| <= eps) of a
// column-major [M, m] fp64 matrix, in index order, without a sort and without atomics.
//
//   k_codes_count    one workgroup per tile of kCodesTile rows of one column; a wave takes
//                    its kCodesWaveRun contiguous rows in steps of 64 (one coalesced 512 B
//                    read per step), ballots the keep predicate and adds the popcounts; the
//                    four wave counts are summed through LDS into cnt[tile].
//   k_codes_scan_*   exclusive int64 scan of the tile counts, in place: each workgroup scans
//                    kCodesScanBlock counts (serial per thread, shuffles per wave, LDS over
//                    the waves) and stores its sum; one workgroup scans those sums, carrying
//                    from one 256-entry step to the next; the last kernel adds each
//                    workgroup's offset and appends the total.
//   k_codes_cols     cols[c] = off[c * tpc]: where each column starts.
//   k_codes_scatter  the count kernel's walk again: a lane's slot is the tile offset plus
//                    the kept entries of the waves and steps before plus the kept lanes
//                    below it (the ballot masked to the lower lanes), so a column's rows land
//                    in ascending order.  Row index and value go out as 8-byte vector stores
//                    into consecutive slots.
// The value is carried as its 64 bits, so pr holds the dense entry unchanged (NaN payloads
// and signed zeros included).  Tile boundaries depend on M alone, so a column's result does
// not depend on the other columns of the launch.
#include "codes.hpp"

#include <algorithm>

namespace ccsc {

typedef unsigned long long u64;
constexpr int64_t kCodesMaxBlocks = (int64_t)1 << 22;   // workgroups per launch
static_assert(kCodesNT == 256 && kCodesTile == 2048, "four waves of kCodesWaveRun rows");

__device__ __forceinline__ bool codes_keep(u64 bits, double eps) {
  return !(fabs(__longlong_as_double((long long)bits)) <= eps);   // a NaN is kept
}

// The keep masks of this wave's steps of tile `tile` and the entries behind them; returns
// the wave's kept count.
__device__ __forceinline__ int codes_wave_masks(const u64* __restrict__ a, int64_t M,
                                                int64_t tpc, double eps, int64_t tile, int wave,
                                                int lane, u64 (&mask)[kCodesSteps],
                                                u64 (&val)[kCodesSteps]) {
  const int64_t col = codes_tile_col(tile, tpc);
  int c = 0;
#pragma unroll
  for (int s = 0; s < kCodesSteps; ++s) {
    const int64_t row = codes_row(tile, tpc, wave, s, lane);
    const bool in = row < M;
    val[s] = in ? a[codes_elem(col, M, row)] : 0;
    mask[s] = __ballot(in && codes_keep(val[s], eps));
    c += __popcll(mask[s]);
  }
  return c;
}

__global__ __launch_bounds__(kCodesNT) void k_codes_count(const u64* __restrict__ a, int64_t M,
                                                          int64_t tpc, double eps,
                                                          int64_t* __restrict__ cnt,
                                                          int64_t block0) {
  __shared__ int sh[kCodesNT / 64];
  const int64_t tile = block0 + blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64 mask[kCodesSteps], val[kCodesSteps];
  const int c = codes_wave_masks(a, M, tpc, eps, tile, wave, lane, mask, val);
  if (lane == 0) sh[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[tile] = (int64_t)sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(kCodesNT) void k_codes_scatter(const u64* __restrict__ a, int64_t M,
                                                            int64_t tpc, double eps,
                                                            const int64_t* __restrict__ off,
                                                            int64_t* __restrict__ ir,
                                                            u64* __restrict__ pr, int64_t block0) {
  __shared__ int sh[kCodesNT / 64];
  const int64_t tile = block0 + blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64 mask[kCodesSteps], val[kCodesSteps];
  const int c = codes_wave_masks(a, M, tpc, eps, tile, wave, lane, mask, val);
  if (lane == 0) sh[wave] = c;
  __syncthreads();
  int64_t before = 0;
  for (int w = 0; w < wave; ++w) before += sh[w];
  const int64_t tile_off = off[tile];
  const u64 below = ((u64)1 << lane) - 1;
#pragma unroll
  for (int s = 0; s < kCodesSteps; ++s) {
    if ((mask[s] >> lane) & 1) {
      const int64_t slot = codes_slot(tile_off, before, __popcll(mask[s] & below));
      ir[slot] = codes_row(tile, tpc, wave, s, lane);
      pr[slot] = val[s];
    }
    before += __popcll(mask[s]);
  }
}

// Inclusive scan of one int64 per thread over the workgroup; *total gets the workgroup sum.
// Ends with a barrier, so sh can be reused at once.
__device__ __forceinline__ int64_t codes_block_scan(int64_t v, int64_t* sh, int64_t* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  int64_t add = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kCodesNT / 64; ++w) {
    if (w < wave) add += sh[w];
    sum += sh[w];
  }
  __syncthreads();
  *total = sum;
  return v + add;
}

// v[i] <- the exclusive scan inside workgroup b's kCodesScanBlock entries; bsum[b] their sum.
__global__ __launch_bounds__(kCodesNT) void k_codes_scan_local(int64_t* __restrict__ v, int64_t T,
                                                               int64_t* __restrict__ bsum) {
  __shared__ int64_t sh[kCodesNT / 64];
  const int64_t i0 = (int64_t)blockIdx.x * kCodesScanBlock + (int64_t)threadIdx.x * kCodesScanPer;
  int64_t x[kCodesScanPer];
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < kCodesScanPer; ++k) {
    x[k] = i0 + k < T ? v[i0 + k] : 0;
    s += x[k];
  }
  int64_t total;
  int64_t run = codes_block_scan(s, sh, &total) - s;   // exclusive over the threads
#pragma unroll
  for (int k = 0; k < kCodesScanPer; ++k) {
    if (i0 + k < T) v[i0 + k] = run;
    run += x[k];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// One workgroup: bsum[0 .. nb) <- its exclusive scan, bsum[nb] <- the total.
__global__ __launch_bounds__(kCodesNT) void k_codes_scan_top(int64_t* __restrict__ bsum,
                                                             int64_t nb) {
  __shared__ int64_t sh[kCodesNT / 64];
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += kCodesNT) {
    const int64_t i = base + threadIdx.x;
    const int64_t x = i < nb ? bsum[i] : 0;
    int64_t total;
    const int64_t incl = codes_block_scan(x, sh, &total);
    if (i < nb) bsum[i] = carry + incl - x;
    carry += total;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}

// v[i] += bsum[i / kCodesScanBlock] for i < T; v[T] = bsum[nb].
__global__ __launch_bounds__(kCodesNT) void k_codes_scan_add(int64_t* __restrict__ v, int64_t T,
                                                             const int64_t* __restrict__ bsum,
                                                             int64_t nb, int64_t block0) {
  const int64_t i = (block0 + blockIdx.x) * kCodesNT + threadIdx.x;
  if (i < T) v[i] += bsum[i / kCodesScanBlock];
  else if (i == T) v[T] = bsum[nb];
}

__global__ __launch_bounds__(kCodesNT) void k_codes_cols(const int64_t* __restrict__ off,
                                                         int64_t tpc, int64_t m,
                                                         int64_t* __restrict__ cols,
                                                         int64_t block0) {
  const int64_t c = (block0 + blockIdx.x) * kCodesNT + threadIdx.x;
  if (c <= m) cols[c] = off[c * tpc];
}

template <typename K, typename... A>
static void codes_launch(K kern, int64_t total, hipStream_t st, A... args) {
  for (int64_t b0 = 0; b0 < total; b0 += kCodesMaxBlocks) {
    const unsigned nb = (unsigned)std::min(kCodesMaxBlocks, total - b0);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(kCodesNT), 0, st, args..., b0);
  }
}

hipError_t launch_codes_count(const double* a, int64_t M, int64_t m, double eps, int64_t* off,
                              int64_t* bsum, int64_t* cols, hipStream_t st) {
  if (M <= 0 || m <= 0) return hipSuccess;
  if (M >= kCodesMaxRows || !a || !off || !bsum || !cols || !(eps >= 0))
    return hipErrorInvalidValue;
  const int64_t tpc = codes_tiles_per_col(M);
  const int64_t T = m * tpc;
  const int64_t nb = codes_scan_blocks(T);
  if (nb > 0x7fffffff) return hipErrorInvalidValue;
  codes_launch(k_codes_count, T, st, reinterpret_cast<const u64*>(a), M, tpc, eps, off);
  hipLaunchKernelGGL(k_codes_scan_local, dim3((unsigned)nb), dim3(kCodesNT), 0, st, off, T, bsum);
  hipLaunchKernelGGL(k_codes_scan_top, dim3(1), dim3(kCodesNT), 0, st, bsum, nb);
  const int64_t* cbsum = bsum;
  codes_launch(k_codes_scan_add, (T + 1 + kCodesNT - 1) / kCodesNT, st, off, T, cbsum, nb);
  const int64_t* coff = off;
  codes_launch(k_codes_cols, (m + 1 + kCodesNT - 1) / kCodesNT, st, coff, tpc, m, cols);
  return hipGetLastError();
}

hipError_t launch_codes_scatter(const double* a, int64_t M, int64_t m, double eps,
                                const int64_t* off, int64_t* ir, double* pr, hipStream_t st) {
  if (M <= 0 || m <= 0) return hipSuccess;
  if (M >= kCodesMaxRows || !a || !off || !ir || !pr || !(eps >= 0)) return hipErrorInvalidValue;
  const int64_t tpc = codes_tiles_per_col(M);
  codes_launch(k_codes_scatter, m * tpc, st, reinterpret_cast<const u64*>(a), M, tpc, eps, off, ir,
               reinterpret_cast<u64*>(pr));
  return hipGetLastError();
}

}  // namespace ccsc
