// libccsc test hooks of the transforms (include/ccsc.h, ccsc_test_*): the plan report of
// every FFT family and the single-family forward / round-trip transforms.
#include "host.hpp"
#include "recon.hpp"
#include "slice.hpp"

#include <functional>

using namespace ccsc;

extern "C" {

int32_t ccsc_test_fft2d(ccsc_ctx* ctx, int32_t X, int32_t Y, int32_t count, const double* in,
                        double* out_halfspec, double* roundtrip, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !in || count <= 0) throw Err(CCSC_E_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    Grid2D G{};
    std::string why;
    if (!make_grid2d(X, Y, G, why)) throw Err(CCSC_E_UNSUPPORTED, why);
    DevBuf tw, a, hs, rt;
    upload_twiddles(tw, make_twiddles(G));
    const size_t P = (size_t)X * Y;
    a.alloc(P * count * 8);
    hs.alloc((size_t)G.F * count * 16);
    rt.alloc(P * count * 8);
    HIPCHK(hipMemcpy(a.p, in, a.bytes, hipMemcpyHostToDevice));
    hipStream_t st = ctx->stream;
    HIPCHK(launch_r2c_embed<double>(a.re(), P, X, Y, 0, 0, hs.cx(), G.F, count, tw.cx(), G, st));
    HIPCHK(launch_c2r_plain<double>(hs.cx(), G.F, rt.re(), P, count,
                                    tw.cx(), G, 1.0 / (double)P, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out_halfspec) HIPCHK(hipMemcpy(out_halfspec, hs.p, hs.bytes, hipMemcpyDeviceToHost));
    if (roundtrip) HIPCHK(hipMemcpy(roundtrip, rt.p, rt.bytes, hipMemcpyDeviceToHost));
  });
}

// ---- plan report and single-family transform hooks (tests) -------------------------
static_assert(kTfftAll == CCSC_FFT_INST_ALL && kTfftRm42 == CCSC_FFT_INST_RM42 &&
                  kTfftFixed38 == CCSC_FFT_INST_FIXED38,
              "ccsc.h names the t-tile instantiations of kernels.hpp");
static_assert(kPlanSlots == 4, "ccsc_fft_dir_plan holds kPlanSlots passes");

// one direction of a plan: `threads` per workgroup, `native_cap` butterflies of a native
// pass of radix R and generic_cap tasks of any other pass (the pfa pass included)
static void report_dir(ccsc_fft_dir_plan& d, const Plan1D& p, int lines, int groups, int ntw,
                       size_t lds, int threads, int twg, int generic_cap,
                       const std::function<int(int)>& native_cap) {
  d = ccsc_fft_dir_plan{};
  d.n = p.n;
  d.npass = p.npass;
  d.pfa = p.pfa;
  d.lines = lines;
  d.groups = groups;
  d.ntw = ntw;
  d.lds_bytes = (int32_t)lds;
  d.threads = threads;
  d.tw_global = twg;
  d.mask = plan_mask(p);
  for (int s = 0; s < p.npass; ++s) {
    const int R = p.rad[s];
    d.rad[s] = R;
    d.twoff[s] = p.twoff[s];
    d.cap[s] = (s == 1 && p.pfa) || !is_native_radix(R) ? generic_cap : native_cap(R);
  }
}
// slice families: kNT threads, one generic task per thread, the instantiation of pass mask rm
static void report_dir_slice(ccsc_fft_dir_plan& d, const Plan1D& p, int lines, int ntw, size_t lds,
                             int rm) {
  report_dir(d, p, lines, 1, ntw, lds, kNT, 0, kNT, [rm](int R) { return rm_maxb(rm, R) * kNT; });
}
// line families: kLineNT threads, kLineGT generic tasks per thread
static void report_dir_line(ccsc_fft_dir_plan& d, const Plan1D& p, int lines, int groups, int ntw,
                            size_t lds, int twg) {
  report_dir(d, p, lines, groups, ntw, lds, kLineNT, twg, kLineGT * kLineNT,
             [](int R) { return maxb_for_radix(R) * kLineBS * kLineNT; });
}

int32_t ccsc_test_fft_plan(int32_t family, int32_t X, int32_t Y, int32_t T, ccsc_fft_plan* out,
                           char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!out) throw Err(CCSC_E_INVALID, "NULL plan output");
    *out = ccsc_fft_plan{};
    out->inst_mask = kRmAll;
    std::string why;
    switch (family) {
      case CCSC_FFT_SLICE2D: {
        if (X <= 0 || Y <= 0) throw Err(CCSC_E_INVALID, "grid extents must be positive");
        Grid2D G{};
        if (!make_grid2d(X, Y, G, why)) throw Err(CCSC_E_UNSUPPORTED, why);
        const int rm = slice_fits(kRm74, G) ? kRm74 : kRmAll;   // the slice kernels' choice
        out->inst = rm == kRm74 ? CCSC_FFT_INST_RM74 : CCSC_FFT_INST_ALL;
        out->inst_mask = rm;
        const size_t lds = fused_smem_bytes(G, sizeof(double), 3);
        report_dir_slice(out->dir[0], G.px, G.Yp / 2, G.ntw, lds, rm);
        report_dir_slice(out->dir[1], G.py, G.Xh, G.ntw, lds, rm);
        break;
      }
      case CCSC_FFT_TTILE: {
        if (X <= 0 || T <= 0) throw Err(CCSC_E_INVALID, "Xh and Tn must be positive");
        Grid2D Gt{};
        if (!make_gridt(T, X, Gt, why)) throw Err(CCSC_E_UNSUPPORTED, why);
        out->inst = tfft_instantiation(Gt);
        const int rm = out->inst == CCSC_FFT_INST_ALL ? kRmAll : kRm42;
        out->inst_mask = rm;
        report_dir_slice(out->dir[2], Gt.py, Gt.Xh, Gt.ntw, tfft_smem_bytes(Gt, sizeof(double)), rm);
        break;
      }
      case CCSC_FFT_LINE2D:
      case CCSC_FFT_LINE3D: {
        const bool is3 = family == CCSC_FFT_LINE3D;
        if (X <= 0 || Y <= 0 || (is3 && T <= 0))
          throw Err(CCSC_E_INVALID, "grid extents must be positive");
        LinePlan lp;
        if (plan_lines(X, Y, is3 ? T : 1, is3, lp) != 0)
          throw Err(CCSC_E_UNSUPPORTED, "grid " + std::to_string(X) + "x" + std::to_string(Y) +
                                            (is3 ? "x" + std::to_string(T) : std::string()) +
                                            " has no global line plan");
        const RowGeom& rg = lp.rg;
        const ColGeom &cy = lp.cy, &ct = lp.ct;
        report_dir_line(out->dir[0], rg.G.px, rg.L, rg.groups, rg.ntw,
                        rows_smem_bytes(rg, sizeof(double)), rg.twg);
        report_dir_line(out->dir[1], cy.p, cy.TC, cy.xtiles, cy.ntw,
                        cols_smem_bytes(cy, sizeof(double)), cy.twg);
        if (is3)
          report_dir_line(out->dir[2], ct.p, ct.TC, ct.xtiles, ct.ntw,
                          cols_smem_bytes(ct, sizeof(double)), ct.twg);
        break;
      }
      default: throw Err(CCSC_E_INVALID, "unknown transform family");
    }
  });
}

int32_t ccsc_test_gfft(ccsc_ctx* ctx, int32_t X, int32_t Y, int32_t T, int32_t count,
                       const double* in, double* out_halfspec, double* roundtrip, char* err,
                       size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !in || count <= 0 || X <= 0 || Y <= 0 || T <= 0)
      throw Err(CCSC_E_INVALID, "bad arguments");
    const int Xh = X / 2 + 1;
    const int64_t P = (int64_t)X * Y * T, F = (int64_t)Xh * Y * T;
    if (P * count > INT32_MAX / 2 || (int64_t)Y * T > 65535 * 2)
      throw Err(CCSC_E_INVALID, "grid too large for the test hook");
    LinePlan lp;
    if (plan_lines(X, Y, T, T > 1, lp) != 0)
      throw Err(CCSC_E_UNSUPPORTED, "grid " + std::to_string(X) + "x" + std::to_string(Y) + "x" +
                                        std::to_string(T) + " has no global line plan");
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf twr, twy, twt, a, S, rt;
    LinePass lines;
    lines.setup(lp, ctx->stream, twr, twy, &twt);
    a.alloc((size_t)(P * count) * 8);
    S.alloc((size_t)(F * count) * 16);
    HIPCHK(hipMemcpy(a.p, in, a.bytes, hipMemcpyHostToDevice));
    hipStream_t st = ctx->stream;
    cpx<double>* Sp = S.cx();
    lines.r2c(a.re(), Sp, count);
    HIPCHK(hipStreamSynchronize(st));
    if (out_halfspec) HIPCHK(hipMemcpy(out_halfspec, S.p, S.bytes, hipMemcpyDeviceToHost));
    if (!roundtrip) return;
    rt.alloc((size_t)(P * count) * 8);
    lines.inv_cols(Sp, count);
    RowArgs<double> rr{};   // no smoothinit, no clamp, zero crop offsets, the full extent
    rr.S = Sp;
    rr.res = rt.re();
    rr.per_img = 1;
    rr.Y = Y;
    rr.sbx = X;
    rr.sby = Y;
    rr.sbt = T;
    rr.scale = 1.0 / (double)P;
    HIPCHK(launch_rows<double>(kRowRes, rr, count, lp.rg, lines.twr, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(roundtrip, rt.p, rt.bytes, hipMemcpyDeviceToHost));
  });
}

int32_t ccsc_test_tfft(ccsc_ctx* ctx, int32_t Tn, int32_t Xh, int32_t Yn, int32_t count,
                       const double* in, double* out, double* roundtrip, char* err,
                       size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !in || count <= 0 || Tn <= 0 || Xh <= 0 || Yn <= 0)
      throw Err(CCSC_E_INVALID, "bad arguments");
    const int64_t N = (int64_t)Tn * Yn * Xh * count;
    if (N > INT32_MAX / 2) throw Err(CCSC_E_INVALID, "tile set too large for the test hook");
    Grid2D Gt{};
    std::string why;
    if (!make_gridt(Tn, Xh, Gt, why)) throw Err(CCSC_E_UNSUPPORTED, why);
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf tw, a, b;
    upload_twiddles(tw, make_twiddles(Gt));
    a.alloc((size_t)N * 16);
    b.alloc((size_t)N * 16);
    HIPCHK(hipMemcpy(a.p, in, a.bytes, hipMemcpyHostToDevice));
    hipStream_t st = ctx->stream;
    const int F2 = Yn * Xh;
    HIPCHK(launch_tfft<double>(a.cx(), b.cx(), count, Yn, F2, -1, tw.cx(), Gt, st));
    if (roundtrip)
      HIPCHK(launch_tfft<double>(b.cx(), a.cx(), count, Yn, F2, +1, tw.cx(), Gt, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out) HIPCHK(hipMemcpy(out, b.p, b.bytes, hipMemcpyDeviceToHost));
    if (roundtrip) HIPCHK(hipMemcpy(roundtrip, a.p, a.bytes, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
