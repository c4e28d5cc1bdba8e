// Host side of the dense -> compressed-sparse-column path (kernels: codes.hip): chunking,
// workspace and the ccsc_sparsify* entry points.  The sessions' entry points (engine.cpp)
// run codes_count_dev / codes_fill_dev over their natural-order z buffer.
//
// Columns go in chunks.  The workspace of a chunk -- its tile offsets, the scan's sums, the
// column offsets and, where the triple goes to the host, 16 B of staging per kept entry --
// stays within 256 MiB, or within CCSC_CODES_WS_MB (MiB, read per call; 0: one column per
// chunk); a single column that needs more gets its own.  It is allocated here and freed
// before the call returns.  The count pass needs no staging, so its chunks are larger; the
// fill pass sizes its chunks from the counts, so a sparse result moves in few large pieces.
#include "codes.hpp"
#include "host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace ccsc {

int64_t codes_budget() {
  int64_t budget = (int64_t)256 << 20;
  if (const char* e = std::getenv("CCSC_CODES_WS_MB")) {
    const long long mb = std::atoll(e);
    if (mb >= 0 && mb < 256) budget = (int64_t)mb << 20;
  }
  return budget;
}

void codes_check_eps(double eps) {
  if (!(eps >= 0))   // NaN fails too
    throw Err(CCSC_E_INVALID, "eps must be a number >= 0 (an entry is kept iff !(|z| <= eps); "
                              "+inf keeps only NaNs)");
}

void codes_check_shape(int64_t M, int64_t n) {
  if (M < 0 || n < 0) throw Err(CCSC_E_INVALID, "M and n must be >= 0");
  if (M >= kCodesMaxRows)
    throw Err(CCSC_E_UNSUPPORTED, "a column of " + std::to_string(M) + " rows: the row count "
                                  "must stay below 2^31");
}

namespace {
struct CodesWs {
  int64_t *off, *bsum, *cols, *ir;
  double* pr;
};
// the layout codes_count_ws_bytes + codes_stage_bytes size
CodesWs codes_carve(void* p, int64_t T, int64_t m, int64_t kept) {
  CodesWs w;
  w.off = static_cast<int64_t*>(p);
  w.bsum = w.off + (T + 1);
  w.cols = w.bsum + (codes_scan_blocks(T) + 1);
  w.ir = w.cols + (m + 1);
  w.pr = reinterpret_cast<double*>(w.ir + kept);
  return w;
}
}  // namespace

void codes_count_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                     int64_t* jc) {
  if (n <= 0) return;
  if (M == 0) {
    std::fill(jc + 1, jc + n + 1, jc[0]);
    return;
  }
  const int64_t tpc = codes_tiles_per_col(M);
  // what one more column adds to codes_count_ws_bytes, rounded up
  const int64_t per_col = 8 * (tpc + 1) + 8 * (tpc / kCodesScanBlock + 1);
  const int64_t chunk = std::max<int64_t>(1, std::min(n, (codes_budget() - 24) / per_col));
  DevBuf ws;
  ws.alloc((size_t)codes_count_ws_bytes(chunk * tpc, chunk));
  std::vector<int64_t> h((size_t)chunk + 1);
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    const CodesWs w = codes_carve(ws.p, m * tpc, m, 0);
    HIPCHK(launch_codes_count(a + c0 * M, M, m, eps, w.off, w.bsum, w.cols, ctx->stream));
    HIPCHK(hipMemcpyAsync(h.data(), w.cols, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int64_t c = 1; c <= m; ++c) jc[c0 + c] = jc[c0] + h[(size_t)c];
  }
}

void codes_fill_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                    const int64_t* jc, int64_t* ir, double* pr, bool out_dev) {
  if (n <= 0 || M == 0 || jc[n] == jc[0]) return;
  const int64_t tpc = codes_tiles_per_col(M);
  const int64_t budget = codes_budget();
  auto need = [&](int64_t c0, int64_t c1) {
    return codes_count_ws_bytes((c1 - c0) * tpc, c1 - c0) +
           (out_dev ? 0 : codes_stage_bytes(jc[c1] - jc[c0]));
  };
  auto chunk_end = [&](int64_t c0) {   // at least one column, then as many as fit
    int64_t c1 = c0 + 1;
    while (c1 < n && need(c0, c1 + 1) <= budget) ++c1;
    return c1;
  };
  int64_t most = 0;
  for (int64_t c0 = 0; c0 < n; c0 = chunk_end(c0)) most = std::max(most, need(c0, chunk_end(c0)));
  DevBuf ws;
  ws.alloc((size_t)most);
  for (int64_t c0 = 0; c0 < n;) {
    const int64_t c1 = chunk_end(c0), m = c1 - c0, kept = jc[c1] - jc[c0];
    const CodesWs w = codes_carve(ws.p, m * tpc, m, kept);
    HIPCHK(launch_codes_count(a + c0 * M, M, m, eps, w.off, w.bsum, w.cols, ctx->stream));
    int64_t total = -1;
    HIPCHK(hipMemcpyAsync(&total, w.cols + m, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (total != kept)   // the slots below were sized from jc
      throw Err(CCSC_E_STATE, "the matrix changed between the count and the fill");
    if (kept > 0) {
      int64_t* oi = out_dev ? ir + jc[c0] : w.ir;
      double* op = out_dev ? pr + jc[c0] : w.pr;
      HIPCHK(launch_codes_scatter(a + c0 * M, M, m, eps, w.off, oi, op, ctx->stream));
      if (!out_dev) {
        HIPCHK(hipMemcpyAsync(ir + jc[c0], w.ir, (size_t)kept * 8, hipMemcpyDeviceToHost,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(pr + jc[c0], w.pr, (size_t)kept * 8, hipMemcpyDeviceToHost,
                              ctx->stream));
      }
    }
    c0 = c1;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));   // the workspace is released on return
}

void codes_check_capacity(int64_t capacity, int64_t nnz) {
  if (capacity < nnz)
    throw Err(CCSC_E_INVALID, "capacity " + std::to_string(capacity) + " is below the " +
                                  std::to_string(nnz) + " kept entries; nothing was written");
}

void codes_check_fill_args(double eps, const int64_t* ir, const double* pr, int64_t capacity) {
  codes_check_eps(eps);
  if (capacity < 0) throw Err(CCSC_E_INVALID, "capacity must be >= 0");
  if (capacity > 0 && (!ir || !pr)) throw Err(CCSC_E_INVALID, "NULL ir or pr");
}

// after eps and the outputs: the shape, then the context
static void sparsify_check(const ccsc_ctx* ctx, const double* a, int64_t M, int64_t n) {
  codes_check_shape(M, n);
  if (!ctx) throw Err(CCSC_E_INVALID, "NULL ctx");
  if (!a && M > 0 && n > 0) throw Err(CCSC_E_INVALID, "NULL matrix");
  if (!ctx->subs.empty())
    throw Err(CCSC_E_UNSUPPORTED, "sparsify runs on a one-device context");
}

// columns of the host matrix staged per upload
static int64_t sparsify_stage_cols(int64_t M, int64_t n) {
  return std::max<int64_t>(1, std::min(n, codes_budget() / std::max<int64_t>(8, M * 8)));
}

// jc[0 .. n] of the host matrix a
static void sparsify_count_host(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                                int64_t* jc, DevBuf& in, int64_t chunk) {
  jc[0] = 0;
  if (M == 0 || n == 0) {
    std::fill(jc, jc + n + 1, 0);
    return;
  }
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    HIPCHK(hipMemcpyAsync(in.p, a + c0 * M, (size_t)(m * M) * 8, hipMemcpyHostToDevice,
                          ctx->stream));
    codes_count_dev(ctx, in.re(), M, m, eps, jc + c0);
  }
}

}  // namespace ccsc

using namespace ccsc;

extern "C" {

int32_t ccsc_sparsify_count_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                                int64_t* jc, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_eps(eps);
    if (!jc) throw Err(CCSC_E_INVALID, "NULL jc");
    sparsify_check(ctx, a, M, n);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int64_t> h((size_t)n + 1, 0);
    codes_count_dev(ctx, a, M, n, eps, h.data());
    HIPCHK(hipMemcpyAsync(jc, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

int32_t ccsc_sparsify_fill_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                               int64_t* ir, double* pr, int64_t capacity, char* err,
                               size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_fill_args(eps, ir, pr, capacity);
    sparsify_check(ctx, a, M, n);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int64_t> h((size_t)n + 1, 0);
    codes_count_dev(ctx, a, M, n, eps, h.data());
    codes_check_capacity(capacity, h[(size_t)n]);
    codes_fill_dev(ctx, a, M, n, eps, h.data(), ir, pr, true);
  });
}

int32_t ccsc_sparsify_count(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                            int64_t* jc, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_eps(eps);
    if (!jc) throw Err(CCSC_E_INVALID, "NULL jc");
    sparsify_check(ctx, a, M, n);
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t chunk = sparsify_stage_cols(M, n);
    DevBuf in;
    in.alloc((size_t)(chunk * M) * 8);
    sparsify_count_host(ctx, a, M, n, eps, jc, in, chunk);
  });
}

int32_t ccsc_sparsify_fill(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                           int64_t* ir, double* pr, int64_t capacity, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_fill_args(eps, ir, pr, capacity);
    sparsify_check(ctx, a, M, n);
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t chunk = sparsify_stage_cols(M, n);
    DevBuf in;
    in.alloc((size_t)(chunk * M) * 8);
    std::vector<int64_t> h((size_t)n + 1, 0);
    sparsify_count_host(ctx, a, M, n, eps, h.data(), in, chunk);
    codes_check_capacity(capacity, h[(size_t)n]);
    if (M == 0 || n == 0) return;
    const bool once = chunk >= n;   // the matrix is on the device already
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
      const int64_t m = std::min(chunk, n - c0);
      if (!once)
        HIPCHK(hipMemcpyAsync(in.p, a + c0 * M, (size_t)(m * M) * 8, hipMemcpyHostToDevice,
                              ctx->stream));
      codes_fill_dev(ctx, in.re(), M, m, eps, h.data() + c0, ir, pr, false);
    }
  });
}

int32_t ccsc_test_codes_index(int64_t M, int64_t tile, int32_t wave, int32_t step, int32_t lane,
                              int64_t tile_off, int64_t before, int32_t prefix, int64_t* out4,
                              char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out4) throw Err(CCSC_E_INVALID, "NULL out4");
    if (M < 1 || M >= kCodesMaxRows || tile < 0 || wave < 0 || wave >= kCodesNT / 64 || step < 0 ||
        step >= kCodesSteps || lane < 0 || lane > 63 || prefix < 0 || prefix > 63)
      throw Err(CCSC_E_INVALID, "index outside the tile geometry");
    const int64_t tpc = codes_tiles_per_col(M);
    out4[0] = codes_tile_col(tile, tpc);
    out4[1] = codes_row(tile, tpc, wave, step, lane);
    out4[2] = codes_elem(out4[0], M, out4[1]);
    out4[3] = codes_slot(tile_off, before, prefix);
  });
}

}  // extern "C"
