// Host side of the threshold sweep (kernels: sweep_codes.hip): validation, the grouping of
// the thresholds, chunking, workspace and the ccsc_threshold_sweep* entry points.
//
// The thresholds are sorted ascending (ties keep the caller's order) and served in groups of
// kSweepEG, one group per launch; every threshold writes its results at the position the
// caller gave it.  A threshold's results do not depend on the group it is in: the entries it
// keeps and their order are its own.  Columns go in chunks.  The host form stages a chunk's
// entries (16 B each), its column offsets, its slices of b, its outputs (24 B per threshold
// and column) and the per-workgroup partials within 256 MiB, or within CCSC_CODES_WS_MB (MiB,
// read per call; 0: one column per chunk); a single column that needs more gets its own.
// The _dev form chunks for the partials alone.  Everything is allocated here and freed
// before the call returns.  A column's results do not depend on the chunk it travels in.
#include "sweep_codes.hpp"
#include "synth_host.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace ccsc {
namespace {

struct SweepGroup {
  SweepEps eps;
  int64_t dst[kSweepEG];
};

SynthGeom sweep_check(const double* d, const int32_t* ks, int32_t C, int32_t K, const int32_t* g,
                      const int64_t* jc, const int64_t* ir, const double* pr, int64_t n,
                      int64_t nnz, const double* b, const double* eps, int32_t E,
                      const int64_t* nnz_out, const double* l1_out, const double* sse_out) {
  const SynthGeom G = synth_check(d, ks, C, K, g, jc, ir, pr, n, nnz, d);   // no `out` here
  if (!b && n > 0) throw Err(CCSC_E_INVALID, "NULL b");
  if (!eps) throw Err(CCSC_E_INVALID, "NULL eps");
  if (E < 1) throw Err(CCSC_E_INVALID, "E must be >= 1");
  if (!nnz_out && n > 0) throw Err(CCSC_E_INVALID, "NULL nnz_out");
  if (!l1_out && n > 0) throw Err(CCSC_E_INVALID, "NULL l1_out");
  if (!sse_out && n > 0) throw Err(CCSC_E_INVALID, "NULL sse_out");
  for (int32_t e = 0; e < E; ++e)
    if (std::isnan(eps[e]))
      throw Err(CCSC_E_INVALID, "eps[" + std::to_string(e) + "] is NaN");
  return G;
}

// the caller's thresholds, ascending, in groups of kSweepEG
std::vector<SweepGroup> sweep_groups(const double* eps, int32_t E) {
  std::vector<int32_t> order((size_t)E);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return eps[a] < eps[b]; });
  std::vector<SweepGroup> gs;
  for (int32_t e0 = 0; e0 < E; e0 += kSweepEG) {
    SweepGroup s{};
    s.eps.n = std::min(kSweepEG, E - e0);
    for (int32_t e = 0; e < s.eps.n; ++e) {
      s.eps.v[e] = eps[order[(size_t)(e0 + e)]];
      s.dst[e] = order[(size_t)(e0 + e)];
    }
    gs.push_back(s);
  }
  return gs;
}

void sweep_run(ccsc_ctx* ctx, const SynthGeom& G, const std::vector<SweepGroup>& gs, int32_t E,
               const double* d, const int64_t* jc, const int64_t* ir, const double* pr, int64_t m,
               int64_t nnz, const double* b, int32_t crop, double* part, int64_t* nnz_out,
               double* l1_out, double* sse_out, int32_t* flag) {
  for (const SweepGroup& s : gs)
    HIPCHK(launch_sweep_codes(G, s.eps, s.dst, E, d, jc, ir, pr, m, nnz, b, crop, part, nnz_out,
                              l1_out, sse_out, flag, ctx->stream));
}

}  // namespace
}  // namespace ccsc

using namespace ccsc;

extern "C" {

int32_t ccsc_threshold_sweep_dev(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C,
                                 int32_t K, const int32_t* g, const int64_t* jc,
                                 const int64_t* ir, const double* pr, int64_t n, int64_t nnz,
                                 const double* b, int32_t crop, const double* eps, int32_t E,
                                 int64_t* nnz_out, double* l1_out, double* sse_out, char* err,
                                 size_t errlen) {
  return guarded(err, errlen, [&] {
    const SynthGeom G = sweep_check(d, ks, C, K, g, jc, ir, pr, n, nnz, b, eps, E, nnz_out,
                                    l1_out, sse_out);
    check_ctx(ctx, "threshold_sweep");
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const std::vector<SweepGroup> gs = sweep_groups(eps, E);
    const int64_t part_col = synth_blocks_per_col(G) * kSweepEG * 8;   // bytes per column
    const int64_t mc = std::min(n, std::max<int64_t>(1, codes_budget() / part_col));
    const int64_t bcol = sweep_b_col_elems(G, crop);
    DevBuf part;
    part.alloc((size_t)(mc * part_col));
    CscFlag flag;
    flag.reset(ctx->stream);
    for (int64_t c0 = 0; c0 < n; c0 += mc)
      sweep_run(ctx, G, gs, E, d, jc + c0, ir, pr, std::min(mc, n - c0), nnz, b + c0 * bcol, crop,
                part.re(), nnz_out + c0 * E, l1_out + c0 * E, sse_out + c0 * E,
                flag.b.as<int32_t>());
    flag.finish(ctx->stream);
  });
}

int32_t ccsc_threshold_sweep(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C,
                             int32_t K, const int32_t* g, const int64_t* jc, const int64_t* ir,
                             const double* pr, int64_t n, int64_t nnz, const double* b,
                             int32_t crop, const double* eps, int32_t E, int64_t* nnz_out,
                             double* l1_out, double* sse_out, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const SynthGeom G = sweep_check(d, ks, C, K, g, jc, ir, pr, n, nnz, b, eps, E, nnz_out,
                                    l1_out, sse_out);
    check_ctx(ctx, "threshold_sweep");
    check_jc_host(jc, n, nnz);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const std::vector<SweepGroup> gs = sweep_groups(eps, E);
    const int64_t nd = synth_taps(G) * G.C * G.K;
    DevBuf dd;
    dd.alloc((size_t)nd * 8);
    HIPCHK(hipMemcpyAsync(dd.p, d, (size_t)nd * 8, hipMemcpyHostToDevice, ctx->stream));
    CscFlag flag;
    flag.reset(ctx->stream);

    const int64_t budget = codes_budget();
    const int64_t bcol = sweep_b_col_elems(G, crop);
    const int64_t part_col = synth_blocks_per_col(G) * kSweepEG;   // doubles per column
    // per column: its slice of b, three outputs per threshold, the partials, a column offset
    const int64_t per_col = 8 * (bcol + 3 * (int64_t)E + part_col + 1);
    auto need = [&](int64_t c0, int64_t c1) {
      return per_col * (c1 - c0) + 16 * (jc[c1] - jc[c0]) + 8;
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
      // every piece is a multiple of 8 bytes
      double* db = ws.re();
      double* dpart = db + m * bcol;
      double* dl1 = dpart + m * part_col;
      double* dsse = dl1 + m * E;
      int64_t* dnnz = reinterpret_cast<int64_t*>(dsse + m * E);
      int64_t* dir = dnnz + m * E;
      double* dpr = reinterpret_cast<double*>(dir + kept);
      int64_t* djc = reinterpret_cast<int64_t*>(dpr + kept);
      hj.resize((size_t)m + 1);
      for (int64_t c = 0; c <= m; ++c) hj[(size_t)c] = jc[c0 + c] - jc[c0];
      HIPCHK(hipMemcpyAsync(djc, hj.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      HIPCHK(hipMemcpyAsync(db, b + c0 * bcol, (size_t)(m * bcol) * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      if (kept > 0) {
        HIPCHK(hipMemcpyAsync(dir, ir + jc[c0], (size_t)kept * 8, hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(dpr, pr + jc[c0], (size_t)kept * 8, hipMemcpyHostToDevice,
                              ctx->stream));
      }
      sweep_run(ctx, G, gs, E, dd.re(), djc, dir, dpr, m, kept, db, crop, dpart, dnnz, dl1, dsse,
                flag.b.as<int32_t>());
      const size_t ob = (size_t)(m * E) * 8;
      HIPCHK(hipMemcpyAsync(nnz_out + c0 * E, dnnz, ob, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(l1_out + c0 * E, dl1, ob, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(sse_out + c0 * E, dsse, ob, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));   // hj and the workspace are reused
      c0 = c1;
    }
    flag.finish(ctx->stream);
  });
}

int32_t ccsc_test_sweep_class(const double* eps, int32_t E, double v, int32_t* m, char* err,
                              size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!eps) throw Err(CCSC_E_INVALID, "NULL eps");
    if (E < 1) throw Err(CCSC_E_INVALID, "E must be >= 1");
    if (!m) throw Err(CCSC_E_INVALID, "NULL m");
    for (int32_t e = 0; e < E; ++e)
      if (std::isnan(eps[e]))
        throw Err(CCSC_E_INVALID, "eps[" + std::to_string(e) + "] is NaN");
    // as the entry points see a value: its class in each group of the sorted list, summed
    int32_t total = 0;
    for (const SweepGroup& s : sweep_groups(eps, E)) total += sweep_class(s.eps.v, s.eps.n, v);
    *m = total;
  });
}

}  // extern "C"
