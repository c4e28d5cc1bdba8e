// Local contrast normalisation of the learners' input images:
// the 'local_cn' branch of image_helpers/CreateImages.m:299-369 followed by its
// ZERO_MEAN branch (CreateImages.m:652-657), for images of any size H, W >= 7:
//
//   k      = fspecial('gaussian', [13 13], 3*1.591)                     (CI:306)
//   lmn    = rconv2(I, k), lmnsq = rconv2(I.^2, k)                       (CI:309-310)
//            rconv2 = reflection about the edge pixels (edge not repeated) then
//            conv2(..., 'valid') (image_helpers/rconv2.m:22-58)
//   lstd   = sqrt(max(lmnsq - lmn.^2, 0))                                (CI:311-313)
//   th     = median: the round(N/2)-th smallest lstd; when it is 0, the same over the
//            nonzero lstd (0 if there are none)                          (CI:334-347)
//   lstd(lstd <= th) = th; lstd(lstd == 0) = eps                         (CI:348-352)
//   I      = single((I - lmn) ./ lstd), then I - mean(I) in single       (CI:367, :655)
//
// Two paths compute this, both column-major [H, W] (MATLAB dim 1 fastest), both with
// the one 13x13 accumulate cn_accum, so lmn, lstd and the threshold th are the same bits:
//
// LDS path (k_local_cn, images of at most 12288 pixels, local_cn_ok): one workgroup per
// image.  The image (reflect-padded, (H+12) x (W+12) fp64) sits in LDS for the two 13x13
// convolutions; every thread keeps its pixels' lmn / lstd in registers; the median is
// a radix select on the IEEE bits of the non-negative stds (8 passes of 8 bits, LDS
// histograms), no sort.
//
// Tiled path (launch_local_cn_tiled, any H, W >= 7 with H * W < 2^31): many workgroups
// per image, the stages below enqueued on one stream over a workspace of 16 B per pixel
// plus 48 KiB per image, no host read in between:
//   k_cn_stats  one workgroup per 32 x 32 tile: tile + 6-pixel halo (reflected in image
//               coordinates, so a ragged tile reflects across the tile seam) in LDS;
//               writes I - lmn and lstd, counts the exactly-zero stds, and histograms the
//               top radix digit (LDS histogram, integer atomics into the image's)
//   k_cn_pick / k_cn_hist  radix select over lstd in global memory, 6 digits
//               (5 x 11 bits, 9 bits): k_cn_pick (one workgroup per image) walks the
//               digit's histogram to the bucket of the wanted rank and keeps (prefix,
//               rank); k_cn_hist histograms the next digit of the stds under that prefix.
//               The rank is round(N/2), or, when at least that many stds are exactly 0
//               (median 0, CI:340-347), zeros + round(nnz/2): decided per image on the
//               device from the zero count, so one select serves either branch
//   k_cn_sum    o = single((I - lmn) / sd), summed in double per 4096-pixel span
//   k_cn_mean   one ordered sum of an image's span sums, rounded to single once
//   k_cn_store  out = o - mean (o recomputed from the workspace: `in` is not read after
//               k_cn_stats, so out may alias in)
// Every sum has a fixed order and every atomic is an integer one: results are bitwise
// reproducible and do not depend on the other images of the batch.
#include "kernels.hpp"

namespace ccsc {

constexpr int kCnNT = 1024;
constexpr int kCnR = 6;                  // 13 x 13 kernel: radius 6
constexpr int kCnMaxPix = 12;            // pixels per thread: H * W <= 12288

struct CnKernel {
  double k[13 * 13];
};

__device__ __forceinline__ int reflect_idx(int i, int n) {
  // MATLAB rconv2 reflection about the edge sample (edge not repeated), |i| < n
  if (i < 0) return -i;
  if (i >= n) return 2 * n - 2 - i;
  return i;
}

// conv2 'valid' of a reflect-padded image with the flipped kernel (rconv2.m:58) at one
// pixel: p points at pad(h, w) of a column-major image with column stride hp,
//   m = sum_{u,v} pad(h + u, w + v) k(12 - u, 12 - v),  q = the same over pad .^ 2.
// The one accumulate of both paths (v outer, u inner): their lmn / lstd agree bitwise.
__device__ __forceinline__ void cn_accum(const double* p, int hp, const CnKernel& kc, double& m,
                                         double& q) {
  m = 0;
  q = 0;
  for (int v = 0; v < 13; ++v) {
    const double* col = p + v * hp;
#pragma unroll
    for (int u = 0; u < 13; ++u) {
      const double x = col[u];
      const double kk = kc.k[(12 - v) * 13 + (12 - u)];   // k(12 - u, 12 - v), column-major
      m += x * kk;
      q += (x * x) * kk;
    }
  }
}

// k-th smallest (1-based) of the lanes' values v[0..cnt) (non-negative doubles: their
// bit patterns order like the values); hist: 256 ints of LDS.
__device__ uint64_t radix_select(const uint64_t (&v)[kCnMaxPix], int cnt, int64_t k, int* hist,
                                 int* shared_k) {
  uint64_t prefix = 0, mask = 0;
  for (int pass = 7; pass >= 0; --pass) {
    const int sh = pass * 8;
    for (int i = threadIdx.x; i < 256; i += kCnNT) hist[i] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kCnMaxPix; ++i)
      if (i < cnt && (v[i] & mask) == prefix) atomicAdd(&hist[(v[i] >> sh) & 255], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t acc = 0;
      int b = 0;
      for (; b < 256; ++b) {
        if (acc + hist[b] >= k) break;
        acc += hist[b];
      }
      shared_k[0] = b;
      shared_k[1] = (int)(k - acc);
    }
    __syncthreads();
    const int b = shared_k[0];
    k = shared_k[1];
    prefix |= (uint64_t)b << sh;
    mask |= (uint64_t)255 << sh;
    __syncthreads();
  }
  return prefix;
}

__global__ __launch_bounds__(kCnNT) void k_local_cn(const double* __restrict__ in,
                                                    double* __restrict__ out, int H, int W,
                                                    CnKernel kc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HP = H + 2 * kCnR, WP = W + 2 * kCnR;
  double* pad = reinterpret_cast<double*>(smem);                 // [WP][HP], h fastest
  int* hist = reinterpret_cast<int*>(pad + (size_t)HP * WP);     // 256 + 2
  double* red = reinterpret_cast<double*>(hist + 260);            // kCnNT / 64
  const int64_t img = blockIdx.x;
  const int N = H * W;
  const double* I = in + img * N;
  for (int e = threadIdx.x; e < HP * WP; e += kCnNT) {
    const int w = e / HP, h = e - w * HP;
    pad[e] = I[reflect_idx(w - kCnR, W) * H + reflect_idx(h - kCnR, H)];
  }
  __syncthreads();
  double lmn[kCnMaxPix], lstd[kCnMaxPix];
  uint64_t bits[kCnMaxPix];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < kCnMaxPix; ++i) {
    const int p = threadIdx.x + i * kCnNT;
    lmn[i] = 0;
    lstd[i] = 0;
    bits[i] = 0;
    if (p < N) {
      cnt = i + 1;
      const int w = p / H, h = p - w * H;
      double m, q;
      cn_accum(pad + w * HP + h, HP, kc, m, q);
      const double var = q - m * m;
      lmn[i] = m;
      lstd[i] = sqrt(var < 0 ? 0.0 : var);
      bits[i] = (uint64_t)__double_as_longlong(lstd[i]);
    }
  }
  // ---- median floor (CI:334-347) ----
  const int64_t lq = (int64_t)floor(N / 2.0 + 0.5);
  double th = __longlong_as_double((long long)radix_select(bits, cnt, lq, hist, hist + 256));
  if (th == 0.0) {
    int z = 0;
#pragma unroll
    for (int i = 0; i < kCnMaxPix; ++i) z += (i < cnt && bits[i] == 0) ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) hist[258] = 0;
    __syncthreads();
    if (z) atomicAdd(&hist[258], z);
    __syncthreads();
    const int zeros = hist[258];
    const int nnz = N - zeros;
    th = 0.0;
    if (nnz > 0) {
      const int64_t lq2 = (int64_t)floor(nnz / 2.0 + 0.5);
      th = __longlong_as_double((long long)radix_select(bits, cnt, zeros + lq2, hist, hist + 256));
    }
  }
  // ---- normalise in single, zero mean in single (CI:348-367, :652-657) ----
  const double* Ip = I;
  float o[kCnMaxPix];
  double s = 0;
#pragma unroll
  for (int i = 0; i < kCnMaxPix; ++i) {
    o[i] = 0.f;
    if (i < cnt) {
      const int p = threadIdx.x + i * kCnNT;
      double sd = lstd[i] <= th ? th : lstd[i];
      if (sd == 0.0) sd = 2.220446049250313e-16;
      o[i] = (float)((Ip[p] - lmn[i]) / sd);
      s += (double)o[i];
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double tot = 0;
  for (int i = 0; i < kCnNT / 64; ++i) tot += red[i];
  const float mean = (float)(tot / (double)N);
  double* O = out + img * N;
#pragma unroll
  for (int i = 0; i < kCnMaxPix; ++i)
    if (i < cnt) O[threadIdx.x + i * kCnNT] = (double)(o[i] - mean);
}

bool local_cn_ok(int H, int W) {
  if (H < 7 || W < 7) return false;          // the 13x13 reflection needs 6 samples per side
  if ((int64_t)H * W > (int64_t)kCnNT * kCnMaxPix) return false;
  const size_t lds = (size_t)(H + 12) * (W + 12) * 8 + 260 * 4 + kCnNT / 64 * 8;
  return lds <= 160 * 1024;
}

static CnKernel cn_gauss() {
  CnKernel kc;
  // fspecial('gaussian', [13 13], 3*1.591): exp(-(x^2+y^2)/(2 sigma^2)), values below
  // eps * max set to 0, normalised to sum 1
  const double sigma = 3 * 1.591;
  double mx = 0, sum = 0;
  for (int a = 0; a < 13; ++a)
    for (int b = 0; b < 13; ++b) {
      const double x = a - 6.0, y = b - 6.0;
      kc.k[b * 13 + a] = std::exp(-(x * x + y * y) / (2 * sigma * sigma));
      mx = kc.k[b * 13 + a] > mx ? kc.k[b * 13 + a] : mx;
    }
  for (int i = 0; i < 169; ++i) {
    if (kc.k[i] < 2.220446049250313e-16 * mx) kc.k[i] = 0;
    sum += kc.k[i];
  }
  for (int i = 0; i < 169; ++i) kc.k[i] /= sum;
  return kc;
}

hipError_t launch_local_cn(const double* in, double* out, int64_t n, int H, int W,
                           hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!local_cn_ok(H, W)) return hipErrorInvalidValue;
  const CnKernel kc = cn_gauss();
  const size_t lds = (size_t)(H + 12) * (W + 12) * 8 + 260 * 4 + kCnNT / 64 * 8;
  hipLaunchKernelGGL(k_local_cn, dim3((unsigned)n), dim3(kCnNT), lds, st, in, out, H, W, kc);
  return hipGetLastError();
}

// ---- tiled path ---------------------------------------------------------------------

constexpr int kCnTile = 32;                    // tile edge (synth.CN_TILE states it for the tests)
constexpr int kCnTP = kCnTile + 2 * kCnR;      // padded tile edge, 44
constexpr int kCnTNT = 256;                    // threads of every tiled-path kernel
constexpr int kCnTPix = kCnTile * kCnTile / kCnTNT;   // pixels per thread of k_cn_stats
constexpr int kCnSpan = 4096;                  // pixels per workgroup of the streaming stages
constexpr int kCnDigits = 6;                   // radix select: 5 digits of 11 bits, one of 9
constexpr int kCnBins = 2048;

__host__ __device__ constexpr int cn_shift(int digit) { return digit < 5 ? 53 - 11 * digit : 0; }
__host__ __device__ constexpr unsigned cn_digit_mask(int digit) { return digit < 5 ? 2047u : 511u; }

// Workspace of a chunk of m images (device pointers into one allocation).
struct CnWs {
  double* d;                    // [m][N] I - lmn
  double* s;                    // [m][N] lstd
  unsigned* hist;               // [m][kCnDigits][kCnBins] digit histograms, zeroed per chunk
  unsigned* zeros;              // [m] exactly-zero stds, zeroed with hist
  unsigned long long* prefix;   // [m] bits of the selected std chosen so far
  long long* rank;              // [m] wanted rank (1-based) among the stds under prefix
  double* th;                   // [m] the median floor
  double* part;                 // [m][nb] span sums of the single-precision image
  float* mean;                  // [m]
};

__device__ __forceinline__ float cn_norm1(double d, double lstd, double th) {
  // lstd(lstd <= th) = th; lstd(lstd == 0) = eps; single(d ./ lstd)        (CI:348-367)
  double sd = lstd <= th ? th : lstd;
  if (sd == 0.0) sd = 2.220446049250313e-16;
  return (float)(d / sd);
}

// Adds a workgroup's LDS histogram to the image's (integer atomics, empty bins skipped).
__device__ __forceinline__ void cn_flush_hist(const unsigned* lh, unsigned* gh) {
  for (int i = threadIdx.x; i < kCnBins; i += kCnTNT)
    if (lh[i]) atomicAdd(&gh[i], lh[i]);
}

// One workgroup per tile; tiles of an image are numbered h fastest, images follow.
__global__ __launch_bounds__(kCnTNT) void k_cn_stats(const double* __restrict__ in, CnWs ws, int H,
                                                     int W, int tH, int tW, CnKernel kc) {
  __shared__ double pad[kCnTP * kCnTP];          // [w][h], h fastest
  __shared__ unsigned hist[kCnBins];
  __shared__ unsigned zcnt;
  const int tpi = tH * tW;
  const int64_t img = blockIdx.x / (unsigned)tpi;
  const int t = (int)(blockIdx.x - img * tpi);
  const int tw = t / tH, th = t - tw * tH;
  const int h0 = th * kCnTile, w0 = tw * kCnTile;
  const int hh = min(kCnTile, H - h0), ww = min(kCnTile, W - w0);   // ragged last tiles
  const int64_t N = (int64_t)H * W;
  const double* I = in + img * N;
  for (int i = threadIdx.x; i < kCnBins; i += kCnTNT) hist[i] = 0;
  if (threadIdx.x == 0) zcnt = 0;
  // tile + halo, reflected in image coordinates; only the (hh + 12) x (ww + 12) part that
  // the tile's pixels read is loaded (its indices stay within the reflection's range)
  for (int e = threadIdx.x; e < kCnTP * kCnTP; e += kCnTNT) {
    const int w = e / kCnTP, h = e - w * kCnTP;
    if (h < hh + 2 * kCnR && w < ww + 2 * kCnR)
      pad[e] = I[(int64_t)reflect_idx(w0 + w - kCnR, W) * H + reflect_idx(h0 + h - kCnR, H)];
  }
  __syncthreads();
  const int h = threadIdx.x & (kCnTile - 1);
  unsigned z = 0;
#pragma unroll
  for (int i = 0; i < kCnTPix; ++i) {
    const int w = (threadIdx.x >> 5) + i * (kCnTNT / kCnTile);
    if (h < hh && w < ww) {
      double m, q;
      cn_accum(pad + w * kCnTP + h, kCnTP, kc, m, q);
      const double var = q - m * m;
      const double sd = sqrt(var < 0 ? 0.0 : var);
      const int64_t p = img * N + (int64_t)(w0 + w) * H + (h0 + h);
      ws.d[p] = pad[(w + kCnR) * kCnTP + h + kCnR] - m;
      ws.s[p] = sd;
      const uint64_t bits = (uint64_t)__double_as_longlong(sd);
      atomicAdd(&hist[(unsigned)(bits >> cn_shift(0))], 1u);
      z += bits == 0 ? 1u : 0u;
    }
  }
  if (z) atomicAdd(&zcnt, z);
  __syncthreads();
  cn_flush_hist(hist, ws.hist + img * (kCnDigits * kCnBins));
  if (threadIdx.x == 0 && zcnt) atomicAdd(&ws.zeros[img], zcnt);
}

// Histogram of digit `digit` (>= 1) of the stds whose higher digits equal the prefix;
// nb workgroups per image, each over one span.
__global__ __launch_bounds__(kCnTNT) void k_cn_hist(CnWs ws, int64_t N, int nb, int digit) {
  __shared__ unsigned hist[kCnBins];
  const int64_t img = blockIdx.x / (unsigned)nb;
  const int64_t base = (int64_t)(blockIdx.x - img * nb) * kCnSpan;
  for (int i = threadIdx.x; i < kCnBins; i += kCnTNT) hist[i] = 0;
  __syncthreads();
  const uint64_t prefix = ws.prefix[img];
  const uint64_t mask = ~(uint64_t)0 << cn_shift(digit - 1);
  const int sh = cn_shift(digit);
  const unsigned dm = cn_digit_mask(digit);
  const uint64_t* S = reinterpret_cast<const uint64_t*>(ws.s + img * N);
#pragma unroll 4
  for (int j = 0; j < kCnSpan / kCnTNT; ++j) {
    const int64_t p = base + threadIdx.x + j * kCnTNT;
    if (p < N) {
      const uint64_t v = S[p];
      if ((v & mask) == prefix) atomicAdd(&hist[(unsigned)(v >> sh) & dm], 1u);
    }
  }
  __syncthreads();
  cn_flush_hist(hist, ws.hist + (img * kCnDigits + digit) * kCnBins);
}

// One workgroup per image: the bucket of digit `digit` that holds the wanted rank.
// digit 0 first sets the rank (CI:334-347): round(N/2), or, when that many stds are
// exactly zero (the median is 0), zeros + round(nnz/2), the median of the nonzero stds
// (0 when there are none).  The last digit completes th.
__global__ __launch_bounds__(kCnTNT) void k_cn_pick(CnWs ws, int64_t N, int digit) {
  __shared__ long long sc[2][kCnTNT];
  const int64_t img = blockIdx.x;
  const int t = threadIdx.x;
  long long k;
  uint64_t prefix = 0;
  if (digit == 0) {
    const long long zeros = ws.zeros[img];
    k = (N + 1) / 2;
    if (zeros >= k && zeros < N) k = zeros + (N - zeros + 1) / 2;
  } else {
    k = ws.rank[img];
    prefix = ws.prefix[img];
  }
  const unsigned* gh = ws.hist + (img * kCnDigits + digit) * kCnBins;
  constexpr int kPer = kCnBins / kCnTNT;
  unsigned c[kPer];
  long long own = 0;
#pragma unroll
  for (int b = 0; b < kPer; ++b) {
    c[b] = gh[t * kPer + b];
    own += c[b];
  }
  // inclusive scan of the threads' bin sums
  sc[0][t] = own;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < kCnTNT; off <<= 1) {
    sc[cur ^ 1][t] = sc[cur][t] + (t >= off ? sc[cur][t - off] : 0);
    __syncthreads();
    cur ^= 1;
  }
  const long long incl = sc[cur][t];
  long long acc = incl - own;
  if (acc < k && k <= incl) {                 // exactly one thread: 1 <= k <= total
    int b = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      if (b == i && acc + c[i] < k) {
        acc += c[i];
        b = i + 1;
      }
    prefix |= (uint64_t)(t * kPer + b) << cn_shift(digit);
    ws.prefix[img] = prefix;
    ws.rank[img] = k - acc;
    if (digit == kCnDigits - 1) ws.th[img] = __longlong_as_double((long long)prefix);
  }
}

// Sum (in double) of the single-precision normalised pixels of one span.
__global__ __launch_bounds__(kCnTNT) void k_cn_sum(CnWs ws, int64_t N, int nb) {
  __shared__ double red[kCnTNT / 64];
  const int64_t img = blockIdx.x / (unsigned)nb;
  const int blk = (int)(blockIdx.x - img * nb);
  const int64_t base = (int64_t)blk * kCnSpan;
  const double th = ws.th[img];
  const double* D = ws.d + img * N;
  const double* S = ws.s + img * N;
  double s = 0;
#pragma unroll 4
  for (int j = 0; j < kCnSpan / kCnTNT; ++j) {
    const int64_t p = base + threadIdx.x + j * kCnTNT;
    if (p < N) s += (double)cn_norm1(D[p], S[p], th);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0;
    for (int i = 0; i < kCnTNT / 64; ++i) tot += red[i];
    ws.part[img * nb + blk] = tot;
  }
}

// One workgroup per image: the ordered sum of its span sums, the mean rounded to single.
__global__ __launch_bounds__(kCnTNT) void k_cn_mean(CnWs ws, int64_t N, int nb) {
  __shared__ double red[kCnTNT / 64];
  const int64_t img = blockIdx.x;
  const double* P = ws.part + img * nb;
  double s = 0;
  for (int i = threadIdx.x; i < nb; i += kCnTNT) s += P[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0;
    for (int i = 0; i < kCnTNT / 64; ++i) tot += red[i];
    ws.mean[img] = (float)(tot / (double)N);
  }
}

__global__ __launch_bounds__(kCnTNT) void k_cn_store(CnWs ws, double* __restrict__ out, int64_t N,
                                                     int nb) {
  const int64_t img = blockIdx.x / (unsigned)nb;
  const int64_t base = (int64_t)(blockIdx.x - img * nb) * kCnSpan;
  const double th = ws.th[img];
  const float mean = ws.mean[img];
  const double* D = ws.d + img * N;
  const double* S = ws.s + img * N;
  double* O = out + img * N;
#pragma unroll 4
  for (int j = 0; j < kCnSpan / kCnTNT; ++j) {
    const int64_t p = base + threadIdx.x + j * kCnTNT;
    if (p < N) O[p] = (double)(cn_norm1(D[p], S[p], th) - mean);
  }
}

bool local_cn_tiled_ok(int H, int W) {
  return H >= 7 && W >= 7 && (int64_t)H * W < ((int64_t)1 << 31);
}

static int64_t cn_tiles(int H, int W) {
  return (int64_t)((H + kCnTile - 1) / kCnTile) * ((W + kCnTile - 1) / kCnTile);
}
static int64_t cn_spans(int H, int W) { return ((int64_t)H * W + kCnSpan - 1) / kCnSpan; }
static size_t cn_align(size_t b) { return (b + 255) & ~(size_t)255; }

// Carves the workspace of m images out of base (nullptr: sizes only); returns its bytes.
static size_t cn_carve(char* base, int64_t m, int H, int W, CnWs* ws) {
  const size_t N = (size_t)H * W, M = (size_t)m, nb = (size_t)cn_spans(H, W);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += cn_align(bytes);
    return p;
  };
  CnWs w;
  w.d = reinterpret_cast<double*>(take(M * N * 8));
  w.s = reinterpret_cast<double*>(take(M * N * 8));
  // hist and zeros are contiguous: one memset clears both
  w.hist = reinterpret_cast<unsigned*>(take(M * kCnDigits * kCnBins * 4));
  w.zeros = reinterpret_cast<unsigned*>(take(M * 4));
  w.prefix = reinterpret_cast<unsigned long long*>(take(M * 8));
  w.rank = reinterpret_cast<long long*>(take(M * 8));
  w.th = reinterpret_cast<double*>(take(M * 8));
  w.part = reinterpret_cast<double*>(take(M * nb * 8));
  w.mean = reinterpret_cast<float*>(take(M * 4));
  if (ws) *ws = w;
  return off;
}

size_t local_cn_tiled_ws_bytes(int64_t m, int H, int W) { return cn_carve(nullptr, m, H, W, nullptr); }

int64_t local_cn_tiled_chunk(int64_t n, int H, int W, size_t budget) {
  // bytes per image (cn_carve), the alignment slack of its nine arrays taken off the budget
  const size_t per = (size_t)H * W * 16 + (size_t)kCnDigits * kCnBins * 4 +
                     (size_t)cn_spans(H, W) * 8 + 32;
  const size_t slack = 9 * 256;
  int64_t m = budget > slack ? (int64_t)((budget - slack) / per) : 0;
  // a launch stays below 2^23 workgroups (2^31 threads) unless one image alone exceeds it
  m = std::min<int64_t>(m, ((int64_t)1 << 23) / cn_tiles(H, W));
  return std::max<int64_t>(1, std::min(m, n));
}

hipError_t launch_local_cn_tiled(const double* in, double* out, int64_t m, int H, int W,
                                 void* workspace, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  if (!local_cn_tiled_ok(H, W) || !workspace) return hipErrorInvalidValue;
  const int tH = (H + kCnTile - 1) / kCnTile, tW = (W + kCnTile - 1) / kCnTile;
  const int64_t tiles = m * cn_tiles(H, W), spans = m * cn_spans(H, W);
  // HIP: grid x block threads below 2^32 (one 2^31-pixel image of 7 rows is 9.6e6 tiles)
  if (tiles >= ((int64_t)1 << 24) || m >= ((int64_t)1 << 24)) return hipErrorInvalidValue;
  const int64_t N = (int64_t)H * W;
  const int nb = (int)cn_spans(H, W);
  CnWs ws;
  cn_carve(static_cast<char*>(workspace), m, H, W, &ws);
  const CnKernel kc = cn_gauss();
  const size_t clear = (size_t)(reinterpret_cast<char*>(ws.zeros) - reinterpret_cast<char*>(ws.hist)) +
                       (size_t)m * 4;
  hipError_t e = hipMemsetAsync(ws.hist, 0, clear, st);
  if (e != hipSuccess) return e;
  const dim3 nt(kCnTNT);
  hipLaunchKernelGGL(k_cn_stats, dim3((unsigned)tiles), nt, 0, st, in, ws, H, W, tH, tW, kc);
  for (int digit = 0; digit < kCnDigits; ++digit) {
    if (digit > 0)
      hipLaunchKernelGGL(k_cn_hist, dim3((unsigned)spans), nt, 0, st, ws, N, nb, digit);
    hipLaunchKernelGGL(k_cn_pick, dim3((unsigned)m), nt, 0, st, ws, N, digit);
  }
  hipLaunchKernelGGL(k_cn_sum, dim3((unsigned)spans), nt, 0, st, ws, N, nb);
  hipLaunchKernelGGL(k_cn_mean, dim3((unsigned)m), nt, 0, st, ws, N, nb);
  hipLaunchKernelGGL(k_cn_store, dim3((unsigned)spans), nt, 0, st, ws, out, N, nb);
  return hipGetLastError();
}


}  // namespace ccsc
