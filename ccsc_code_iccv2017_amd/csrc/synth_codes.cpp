// Host side of the synthesis from sparse codes and of the CSC -> dense expansion (kernels:
// synth_codes.hip): validation, chunking, workspace and the ccsc_synthesize* / ccsc_densify*
// entry points.
//
// The host forms stage columns in chunks: a chunk's entries (16 B each), its column offsets
// and its output planes stay within 256 MiB, or within CCSC_CODES_WS_MB (MiB, read per call;
// 0: one column per chunk); a single column that needs more gets its own.  The filters go
// up once.  Everything is allocated here and freed before the call returns.  A column's
// result does not depend on the chunk it travels in.
#include "synth_host.hpp"

#include <algorithm>
#include <cstring>

namespace ccsc {

const char* const kCscMalformed =
    "the sparse matrix is malformed: a column range of jc outside [0, nnz] or decreasing, or a "
    "row of ir outside [0, M)";

namespace {

void check_csc_args(const int64_t* jc, const int64_t* ir, const double* pr, int64_t n,
                    int64_t nnz, const double* out, bool need_out) {
  if (n < 0) throw Err(CCSC_E_INVALID, "n must be >= 0");
  if (nnz < 0) throw Err(CCSC_E_INVALID, "nnz must be >= 0");
  if (!jc) throw Err(CCSC_E_INVALID, "NULL jc");
  if (nnz > 0 && !ir) throw Err(CCSC_E_INVALID, "NULL ir");
  if (nnz > 0 && !pr) throw Err(CCSC_E_INVALID, "NULL pr");
  if (!out && need_out) throw Err(CCSC_E_INVALID, "NULL out");
}

}  // namespace

SynthGeom synth_check(const double* d, const int32_t* ks, int32_t C, int32_t K, const int32_t* g,
                      const int64_t* jc, const int64_t* ir, const double* pr, int64_t n,
                      int64_t nnz, const double* out) {
  if (!d) throw Err(CCSC_E_INVALID, "NULL d");
  if (!ks) throw Err(CCSC_E_INVALID, "NULL ks");
  if (!g) throw Err(CCSC_E_INVALID, "NULL g");
  SynthGeom G;
  for (int a = 0; a < 3; ++a) {
    const std::string ax = "[" + std::to_string(a) + "]";
    if (g[a] < 1) throw Err(CCSC_E_INVALID, "g" + ax + " must be >= 1");
    if (ks[a] < 1 || ks[a] % 2 == 0)
      throw Err(CCSC_E_INVALID, "ks" + ax + " = " + std::to_string(ks[a]) +
                                    " must be odd and >= 1");
    if (ks[a] > g[a])
      throw Err(CCSC_E_INVALID, "ks" + ax + " = " + std::to_string(ks[a]) + " exceeds g" + ax +
                                    " = " + std::to_string(g[a]));
    G.g[a] = g[a];
    G.ks[a] = ks[a];
  }
  if (C < 1) throw Err(CCSC_E_INVALID, "C must be >= 1");
  if (K < 1) throw Err(CCSC_E_INVALID, "K must be >= 1");
  G.C = C;
  G.K = K;
  check_csc_args(jc, ir, pr, n, nnz, out, n > 0);
  // g[a] < 2^31 each: the product of three stays below 2^93, so compare in steps
  const int64_t plane = (int64_t)g[0] * g[1];
  if (plane >= kSynthMaxRows || plane * g[2] >= kSynthMaxRows ||
      plane * g[2] * K >= kSynthMaxRows)
    throw Err(CCSC_E_UNSUPPORTED, "M = g[0] g[1] g[2] K rows: the row count must stay below 2^31");
  const int64_t taps = synth_taps(G);   // <= M < 2^31
  if (taps * C >= kSynthMaxTaps || taps * C * K >= kSynthMaxTaps)
    throw Err(CCSC_E_UNSUPPORTED, "the filters d hold C K ks[0] ks[1] ks[2] values: that count "
                                  "must stay below 2^31");
  return G;
}

void check_ctx(const ccsc_ctx* ctx, const char* what) {
  if (!ctx) throw Err(CCSC_E_INVALID, "NULL ctx");
  if (!ctx->subs.empty())
    throw Err(CCSC_E_UNSUPPORTED, std::string(what) + " runs on a one-device context");
}

// the host forms' check of the column offsets, before any launch
void check_jc_host(const int64_t* jc, int64_t n, int64_t nnz) {
  if (jc[0] < 0) throw Err(CCSC_E_INVALID, "jc[0] is negative");
  for (int64_t c = 0; c < n; ++c)
    if (jc[c + 1] < jc[c])
      throw Err(CCSC_E_INVALID, "jc decreases at column " + std::to_string(c));
  if (jc[n] > nnz)
    throw Err(CCSC_E_INVALID, "jc[n] = " + std::to_string(jc[n]) + " exceeds nnz = " +
                                  std::to_string(nnz));
}

namespace {

using Flag = CscFlag;

// Host triple -> host output [col_elems, n] through launch(jc, ir, pr, m, kept, out) on device
// copies of chunks of columns; jc has passed check_jc_host.
template <typename F>
void host_chunks(ccsc_ctx* ctx, const int64_t* jc, const int64_t* ir, const double* pr, int64_t n,
                 int64_t col_elems, double* out, F&& launch) {
  const int64_t budget = codes_budget();
  auto need = [&](int64_t c0, int64_t c1) {
    return 8 * (c1 - c0) * col_elems + 16 * (jc[c1] - jc[c0]) + 8 * (c1 - c0 + 1);
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
  std::vector<int64_t> hj;
  for (int64_t c0 = 0; c0 < n;) {
    const int64_t c1 = chunk_end(c0), m = c1 - c0, kept = jc[c1] - jc[c0];
    double* dout = ws.re();
    int64_t* dir = reinterpret_cast<int64_t*>(dout + m * col_elems);
    double* dpr = reinterpret_cast<double*>(dir + kept);
    int64_t* djc = reinterpret_cast<int64_t*>(dpr + kept);
    hj.resize((size_t)m + 1);
    for (int64_t c = 0; c <= m; ++c) hj[(size_t)c] = jc[c0 + c] - jc[c0];
    HIPCHK(hipMemcpyAsync(djc, hj.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice,
                          ctx->stream));
    if (kept > 0) {
      HIPCHK(hipMemcpyAsync(dir, ir + jc[c0], (size_t)kept * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      HIPCHK(hipMemcpyAsync(dpr, pr + jc[c0], (size_t)kept * 8, hipMemcpyHostToDevice,
                            ctx->stream));
    }
    launch(djc, dir, dpr, m, kept, dout);
    if (col_elems > 0)
      HIPCHK(hipMemcpyAsync(out + c0 * col_elems, dout, (size_t)(m * col_elems) * 8,
                            hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // hj and the workspace are reused
    c0 = c1;
  }
}

void densify_check(const int64_t* jc, const int64_t* ir, const double* pr, int64_t M, int64_t n,
                   int64_t nnz, const double* out) {
  if (M < 0) throw Err(CCSC_E_INVALID, "M must be >= 0");
  check_csc_args(jc, ir, pr, n, nnz, out, n > 0 && M > 0);
  if (M >= kSynthMaxRows)
    throw Err(CCSC_E_UNSUPPORTED, "a column of " + std::to_string(M) + " rows: the row count "
                                  "must stay below 2^31");
}

}  // namespace
}  // namespace ccsc

using namespace ccsc;

extern "C" {

int32_t ccsc_synthesize_dev(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C,
                            int32_t K, const int32_t* g, const int64_t* jc, const int64_t* ir,
                            const double* pr, int64_t n, int64_t nnz, double* out, char* err,
                            size_t errlen) {
  return guarded(err, errlen, [&] {
    const SynthGeom G = synth_check(d, ks, C, K, g, jc, ir, pr, n, nnz, out);
    check_ctx(ctx, "synthesize");
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    Flag flag;
    flag.reset(ctx->stream);
    HIPCHK(launch_synth_codes(G, d, jc, ir, pr, n, nnz, out, flag.b.as<int32_t>(), ctx->stream));
    flag.finish(ctx->stream);
  });
}

int32_t ccsc_synthesize(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C, int32_t K,
                        const int32_t* g, const int64_t* jc, const int64_t* ir, const double* pr,
                        int64_t n, int64_t nnz, double* out, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const SynthGeom G = synth_check(d, ks, C, K, g, jc, ir, pr, n, nnz, out);
    check_ctx(ctx, "synthesize");
    check_jc_host(jc, n, nnz);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t nd = synth_taps(G) * G.C * G.K;
    DevBuf dd;
    dd.alloc((size_t)nd * 8);
    HIPCHK(hipMemcpyAsync(dd.p, d, (size_t)nd * 8, hipMemcpyHostToDevice, ctx->stream));
    Flag flag;
    flag.reset(ctx->stream);
    const int64_t col_elems = (int64_t)G.g[0] * G.g[1] * G.g[2] * G.C;
    host_chunks(ctx, jc, ir, pr, n, col_elems, out,
                [&](const int64_t* djc, const int64_t* dir, const double* dpr, int64_t m,
                    int64_t kept, double* dout) {
                  HIPCHK(launch_synth_codes(G, dd.re(), djc, dir, dpr, m, kept, dout,
                                            flag.b.as<int32_t>(), ctx->stream));
                });
    flag.finish(ctx->stream);
  });
}

int32_t ccsc_densify_dev(ccsc_ctx* ctx, const int64_t* jc, const int64_t* ir, const double* pr,
                         int64_t M, int64_t n, int64_t nnz, double* out, char* err,
                         size_t errlen) {
  return guarded(err, errlen, [&] {
    densify_check(jc, ir, pr, M, n, nnz, out);
    check_ctx(ctx, "densify");
    if (n == 0 || M == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    Flag flag;
    flag.reset(ctx->stream);
    HIPCHK(launch_codes_expand(jc, ir, pr, M, n, nnz, out, flag.b.as<int32_t>(), ctx->stream));
    flag.finish(ctx->stream);
  });
}

int32_t ccsc_densify(ccsc_ctx* ctx, const int64_t* jc, const int64_t* ir, const double* pr,
                     int64_t M, int64_t n, int64_t nnz, double* out, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    densify_check(jc, ir, pr, M, n, nnz, out);
    check_ctx(ctx, "densify");
    check_jc_host(jc, n, nnz);
    if (M == 0 && jc[n] > jc[0]) throw Err(CCSC_E_INVALID, kCscMalformed);
    if (n == 0 || M == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    Flag flag;
    flag.reset(ctx->stream);
    host_chunks(ctx, jc, ir, pr, n, M, out,
                [&](const int64_t* djc, const int64_t* dir, const double* dpr, int64_t m,
                    int64_t kept, double* dout) {
                  HIPCHK(launch_codes_expand(djc, dir, dpr, M, m, kept, dout,
                                             flag.b.as<int32_t>(), ctx->stream));
                });
    flag.finish(ctx->stream);
  });
}

int32_t ccsc_test_synth_index(const int32_t* g, const int32_t* ks, int32_t C, int32_t K,
                              int64_t row, const int32_t* lo, const int32_t* len,
                              const int32_t* p, int32_t c, int64_t col, int64_t* out8, char* err,
                              size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!lo || !len || !p) throw Err(CCSC_E_INVALID, "NULL lo, len or p");
    if (!out8) throw Err(CCSC_E_INVALID, "NULL out8");
    const int64_t one[2] = {0, 0};
    const double dummy = 0;
    const SynthGeom G = synth_check(&dummy, ks, C, K, g, one, nullptr, nullptr, 0, 0, nullptr);
    const int64_t M = synth_rows(G);
    if (row < 0 || row >= M) throw Err(CCSC_E_INVALID, "row outside [0, M)");
    if (c < 0 || c >= C || col < 0) throw Err(CCSC_E_INVALID, "c outside [0, C) or col < 0");
    for (int a = 0; a < 3; ++a)
      if (lo[a] < 0 || len[a] < 1 || lo[a] + (int64_t)len[a] > g[a] || p[a] < 0 || p[a] >= g[a])
        throw Err(CCSC_E_INVALID, "lo, len or p outside the grid");
    int32_t e[4];
    synth_decode(G, row, &e[0], &e[1], &e[2], &e[3]);
    bool hit = true, tap = true;
    int32_t i[3];
    for (int a = 0; a < 3; ++a) {
      hit = hit && synth_in_window(e[a], lo[a], len[a], ks[a] / 2, g[a]);
      i[a] = synth_tap_coord(p[a], e[a], ks[a] / 2, g[a]);
      tap = tap && i[a] < ks[a];
    }
    for (int a = 0; a < 4; ++a) out8[a] = e[a];
    out8[4] = hit ? 1 : 0;
    out8[5] = tap ? synth_tap_index(G, i[0], i[1], i[2], c, e[3]) : -1;
    out8[6] = synth_out_index(G, p[0], p[1], p[2], c, col);
    out8[7] = M;
  });
}

}  // extern "C"
