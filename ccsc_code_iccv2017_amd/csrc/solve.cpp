// libccsc reconstruction solvers: planning, the ADMM schedule and the C-ABI
// ccsc_solve (kernels in recon.hip).
//
// Per iteration (SI:81-139 and its siblings), one launch each:
//   rows(codes)  C2R of zhat -> z (tol partials) -> ProxSparse / dual -> R2C x-lines of xi2
//   rows(data)   C2R of sum_k dhat zhat -> v1 (objective partials) -> data prox / dual
//                -> R2C x-lines of xi1
//   cols fwd     y (and t) lines of both spectrum sets
//   solve        Sherman-Morrison (SI, SP) or the diagonal form (SD, SL, SV) per bin,
//                plus the synthesis sum_k dhat zhat that becomes the next v1
//   cols inv
// The partial sums are read back only when the tol test or the verbose trace needs
// them; the reconstruction is formed after the last iteration from z (fft2(z) ==
// zhat for the Hermitian iterates of these real problems).
#include "host.hpp"
#include "recon.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace ccsc {

// ---------------------------------------------------------------------------
// problem resolution
// ---------------------------------------------------------------------------
struct SolveSpec {
  ccsc_solve_problem p;
  int nd = 2;              // transform dims
  int X = 0, Y = 0, Tn = 1;
  int rx = 0, ry = 0, rt = 0;
  int Kc = 0;              // code channels (incl. the dirac of SP / SV)
  int W = 1;               // data channels
  int64_t P = 0, F = 0;    // voxels / half-spectrum bins per slice
  double c_gamma = 0;      // gamma_heuristic = c_gamma * lambda / max(b)
  double g1_div = 1;       // gamma(1) = gamma_heuristic / g1_div
  double rho = 0;          // z-solve rho
  LinePlan lp;             // rows over the Y Tn rows, y-lines, (video) t-lines
};

static void resolve_solve(const ccsc_solve_problem& pin, SolveSpec& S) {
  S.p = pin;
  ccsc_solve_problem& p = S.p;
  if (p.variant < CCSC_SOLVE_INPAINT2D || p.variant > CCSC_SOLVE_VIDEO3D)
    throw Err(CCSC_E_INVALID, "unknown solver variant");
  const bool v3 = p.variant == CCSC_SOLVE_VIDEO3D;
  S.nd = v3 ? 3 : 2;
  if (!v3) p.sb[2] = 1;
  for (int i = 0; i < S.nd; ++i)
    if (p.sb[i] <= 0) throw Err(CCSC_E_INVALID, "image extent must be positive");
  if (p.n <= 0) throw Err(CCSC_E_INVALID, "n must be positive");
  if (p.K <= 0) throw Err(CCSC_E_INVALID, "K must be positive");
  if (p.max_it < 0) throw Err(CCSC_E_INVALID, "max_it must be >= 0");
  if (p.verbose < CCSC_VERBOSE_NONE || p.verbose > CCSC_VERBOSE_ALL)
    throw Err(CCSC_E_INVALID, "bad verbose");
  if (!v3) p.ksize[2] = 1;
  for (int i = 0; i < S.nd; ++i)
    if (p.ksize[i] <= 0) throw Err(CCSC_E_INVALID, "filter extent must be positive");
  if (p.variant == CCSC_SOLVE_MULTICH) {
    if (p.nch <= 0) throw Err(CCSC_E_INVALID, "MULTICH needs the channel count W = size(b, 3)");
    S.W = p.nch;
  } else {
    p.nch = 1;
  }
  if (v3)
    for (int i = 0; i < 3; ++i)
      if (p.psf_size[i] <= 0) throw Err(CCSC_E_INVALID, "VIDEO3D needs the psf extent");
  // psf_radius = floor(size(kmat)/2) and the padded grid (SI:10-11, SP:10-11, SV:10-11);
  // SD/SL do not pad (psf_radius = [0 0], SD:5)
  if (p.variant != CCSC_SOLVE_MULTICH) {
    S.rx = p.ksize[0] / 2;
    S.ry = p.ksize[1] / 2;
    S.rt = v3 ? p.ksize[2] / 2 : 0;
  }
  S.X = (int)(p.sb[0] + 2 * S.rx);
  S.Y = (int)(p.sb[1] + 2 * S.ry);
  S.Tn = v3 ? (int)(p.sb[2] + 2 * S.rt) : 1;
  if (p.variant == CCSC_SOLVE_MULTICH && (p.ksize[0] > S.X || p.ksize[1] > S.Y))
    throw Err(CCSC_E_INVALID, "filters larger than the image (psf2otf)");
  if (v3 && (p.psf_size[0] > S.X || p.psf_size[1] > S.Y || p.psf_size[2] > S.Tn))
    throw Err(CCSC_E_INVALID, "psf larger than the padded grid (psf2otf)");
  for (int i = 0; i < S.nd; ++i) {
    const int r = i == 0 ? S.rx : (i == 1 ? S.ry : S.rt);
    if (r > p.sb[i]) throw Err(CCSC_E_INVALID, "symmetric padding wider than the image");
  }
  S.Kc = p.K + ((p.variant == CCSC_SOLVE_POISSON2D || v3) ? 1 : 0);
  S.P = (int64_t)S.X * S.Y * S.Tn;
  S.F = (int64_t)(S.X / 2 + 1) * S.Y * S.Tn;
  switch (p.variant) {
    case CCSC_SOLVE_INPAINT2D: S.c_gamma = 60; S.g1_div = 100; S.rho = 100; break;   // SI:36-37,178
    case CCSC_SOLVE_POISSON2D: S.c_gamma = 20; S.g1_div = 5; S.rho = 5; break;       // SP:34-35,179
    case CCSC_SOLVE_MULTICH: S.c_gamma = 60; S.g1_div = 1; S.rho = S.W; break;        // SD:31-32,126
    case CCSC_SOLVE_VIDEO3D: S.c_gamma = 500; S.g1_div = 1; S.rho = S.Tn; break;      // SV:36-37,149
  }
  if (!(p.lambda_prior > 0)) throw Err(CCSC_E_INVALID, "lambda_prior must be positive (gamma heuristic)");
  // transform plans
  if (const int bad = plan_lines(S.X, S.Y, S.Tn, v3, S.lp))
    throw Err(CCSC_E_UNSUPPORTED, "grid length " + std::to_string(bad) + " has no line plan");
  if (S.F > INT32_MAX / 2 || (int64_t)S.Kc * S.W > 65535 * 4)
    throw Err(CCSC_E_UNSUPPORTED, "spectrum too large for the per-bin kernels");
  if (p.n > 65535) throw Err(CCSC_E_UNSUPPORTED, "more than 65535 images in one call");
}

// ---------------------------------------------------------------------------
// the solver session (one call)
// ---------------------------------------------------------------------------
struct Solver {
  SolveSpec S;
  hipStream_t st;
  int64_t n;
  DevBuf tw_r, tw_y, tw_t;
  LinePass lines;   // twiddle tables, the unfused transforms (the iteration's passes are fused)
  DevBuf dhat, dhat_res, senergy;
  DevBuf Sz, Sx, Z, D2, D1, M, Mb, SM, XO;
  DevBuf part, sums, theta1, theta2, active;
  std::vector<double> h_theta1, h_theta2;

  Solver(ccsc_ctx* ctx, const ccsc_solve_problem& p) : st(ctx->stream) {
    resolve_solve(p, S);
    n = S.p.n;
  }

  // both spectrum sets (codes, data) in one launch per line direction
  void cols2(int sign, int64_t nz, int64_t nx) {
    cpx<double>* a = Sz.cx();
    cpx<double>* b = Sx.cx();
    auto y_lines = [&] {
      HIPCHK(launch_cols<double>(a, sign, nz * S.Tn, S.lp.cy, lines.twy, st, b, nx * S.Tn));
    };
    if (sign < 0) y_lines();
    if (S.lp.with_t)
      HIPCHK(launch_cols<double>(a, sign, nz * S.Y, S.lp.ct, lines.twt, st, b, nx * S.Y));
    if (sign > 0) y_lines();
  }

  void setup(const ccsc_solve_inputs& in) {
    const ccsc_solve_problem& p = S.p;
    if (!in.b || !in.kernels || !in.mask) throw Err(CCSC_E_INVALID, "b, kernels and mask are required");
    const bool v3 = p.variant == CCSC_SOLVE_VIDEO3D;
    const bool has_sm = p.variant != CCSC_SOLVE_POISSON2D;
    if (has_sm && !in.smooth_init) throw Err(CCSC_E_INVALID, "smooth_init is required");
    if (v3 && !in.psf) throw Err(CCSC_E_INVALID, "VIDEO3D needs the psf");
    const bool psnr = in.x_orig && (p.variant == CCSC_SOLVE_INPAINT2D ||
                                    p.variant == CCSC_SOLVE_POISSON2D);
    lines.setup(S.lp, st, tw_r, tw_y, &tw_t);
    const int64_t P = S.P, F = S.F;
    const int Kc = S.Kc, W = S.W;
    // ---- filter spectra (psf2otf of every filter; SI:155-162, SD:100-115, SV:121-138)
    const int kx = p.ksize[0], ky = p.ksize[1], kt = v3 ? p.ksize[2] : 1;
    const int64_t kvol = (int64_t)kx * ky * kt;
    const int64_t nfilt = (int64_t)Kc * W;
    std::vector<double> hk((size_t)(kvol * nfilt), 0.0);
    const int64_t nlearn = (int64_t)p.K * W;
    const int64_t koff = v3 ? kvol : 0;   // SV prepends the dirac (SV:7), SP appends it (SP:7)
    std::memcpy(hk.data() + koff, in.kernels, (size_t)(kvol * nlearn) * 8);
    if (p.variant == CCSC_SOLVE_POISSON2D || v3) {
      double* dk = hk.data() + (v3 ? 0 : kvol * nlearn);
      dk[(int64_t)(kt / 2) * kx * ky + (int64_t)(ky / 2) * kx + kx / 2] = 1.0;   // SP:6, SV:6
    }
    {
      DevBuf kd, grid;
      kd.alloc(hk.size() * 8);
      HIPCHK(hipMemcpyAsync(kd.p, hk.data(), kd.bytes, hipMemcpyHostToDevice, st));
      grid.alloc((size_t)(nfilt * P) * 8);
      HIPCHK(hipMemsetAsync(grid.p, 0, grid.bytes, st));
      HIPCHK(launch_embed_kernels<double>(kd.re(), grid.re(), kx, ky, kt,
                                          (int)nfilt, S.X, S.Y, S.Tn, st));
      dhat.alloc((size_t)(nfilt * F) * 16);
      lines.r2c(grid.re(), dhat.cx(), nfilt);
      if (v3) {
        // dhat = psf_hat .* dhat_k (SV:131); the reconstruction keeps dhat_k (SV:109)
        dhat_res.alloc(dhat.bytes);
        HIPCHK(hipMemcpyAsync(dhat_res.p, dhat.p, dhat.bytes, hipMemcpyDeviceToDevice, st));
        const int64_t pvol = (int64_t)p.psf_size[0] * p.psf_size[1] * p.psf_size[2];
        DevBuf pd, pg, ph;
        pd.alloc((size_t)pvol * 8);
        HIPCHK(hipMemcpyAsync(pd.p, in.psf, pd.bytes, hipMemcpyHostToDevice, st));
        pg.alloc((size_t)P * 8);
        HIPCHK(hipMemsetAsync(pg.p, 0, pg.bytes, st));
        HIPCHK(launch_embed_kernels<double>(pd.re(), pg.re(), p.psf_size[0],
                                            p.psf_size[1], p.psf_size[2], 1, S.X, S.Y, S.Tn, st));
        ph.alloc((size_t)F * 16);
        lines.r2c(pg.re(), ph.cx(), 1);
        HIPCHK(launch_spec_mul<double>(dhat.cx(), ph.cx(), F, (int)nfilt, st));
        HIPCHK(hipStreamSynchronize(st));
      }
      HIPCHK(hipStreamSynchronize(st));
    }
    // s = sum |dhat|^2 (SI:166); the diagonal solves keep invP / (rho + s) (SD:132, SV:155)
    senergy.alloc((size_t)F * 8);
    const bool diag = p.variant == CCSC_SOLVE_MULTICH || v3;
    HIPCHK(launch_spec_energy<double>(dhat.cx(), senergy.re(), F, (int)nfilt,
                                      diag ? 1 : 0, S.rho, 1.0 / (double)P, st));
    // ---- per-image data on the padded grid
    const int64_t sbv = p.sb[0] * p.sb[1] * p.sb[2];
    const int64_t nd = n * W;   // data slices
    {
      DevBuf b, mk, sm, xo;
      b.alloc((size_t)(nd * sbv) * 8);
      mk.alloc(b.bytes);
      HIPCHK(hipMemcpyAsync(b.p, in.b, b.bytes, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(mk.p, in.mask, mk.bytes, hipMemcpyHostToDevice, st));
      if (has_sm) {
        sm.alloc(b.bytes);
        HIPCHK(hipMemcpyAsync(sm.p, in.smooth_init, sm.bytes, hipMemcpyHostToDevice, st));
      }
      if (psnr) {
        xo.alloc((size_t)(n * sbv) * 8);
        HIPCHK(hipMemcpyAsync(xo.p, in.x_orig, xo.bytes, hipMemcpyHostToDevice, st));
      }
      M.alloc((size_t)(nd * P) * 8);
      Mb.alloc(M.bytes);
      if (has_sm) SM.alloc(M.bytes);
      if (psnr) XO.alloc(M.bytes);
      HIPCHK(launch_pad_inputs<double>(b.re(), mk.re(), sm.re(), xo.re(), M.re(), Mb.re(), SM.re(),
                                       XO.re(), nd, (int)p.sb[0], (int)p.sb[1], (int)p.sb[2], S.rx,
                                       S.ry, S.rt, S.X, S.Y, S.Tn, st));
      // gamma_heuristic = c * lambda / max(b(:)) per image (SI:36)
      DevBuf scratch, mx;
      scratch.alloc(2 * kNormParts * 8);
      mx.alloc((size_t)n * 8);
      for (int64_t i = 0; i < n; ++i)
        HIPCHK(launch_max<double>(b.re() + i * W * sbv, W * sbv, scratch.re(), mx.re() + i, st));
      std::vector<double> hmax((size_t)n);
      HIPCHK(hipMemcpyAsync(hmax.data(), mx.p, mx.bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      h_theta1.resize((size_t)n);
      h_theta2.resize((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        const double gh = S.c_gamma * p.lambda_prior / hmax[(size_t)i];
        h_theta1[(size_t)i] = p.lambda_residual / (gh / S.g1_div);   // lambda(1)/gamma(1) (SI:88)
        h_theta2[(size_t)i] = p.lambda_prior / gh;                   // lambda(2)/gamma(2) (SI:89)
      }
    }
    theta1.alloc((size_t)n * 8);
    theta2.alloc((size_t)n * 8);
    HIPCHK(hipMemcpyAsync(theta1.p, h_theta1.data(), theta1.bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(theta2.p, h_theta2.data(), theta2.bytes, hipMemcpyHostToDevice, st));
    // ---- state
    Sz.alloc((size_t)(n * Kc * F) * 16);
    Sx.alloc((size_t)(nd * F) * 16);
    Z.alloc((size_t)(n * Kc * P) * 8);
    D2.alloc(Z.bytes);
    D1.alloc((size_t)(nd * P) * 8);
    HIPCHK(hipMemsetAsync(Z.p, 0, Z.bytes, st));
    HIPCHK(hipMemsetAsync(D2.p, 0, D2.bytes, st));
    HIPCHK(hipMemsetAsync(D1.p, 0, D1.bytes, st));
    part.alloc((size_t)(n * (Kc + W) * S.lp.rg.groups * kRowParts) * 8);
    sums.alloc((size_t)(n * kRowParts) * 8);
    active.alloc((size_t)n * 4);
    std::vector<int> ones((size_t)n, 1);
    HIPCHK(hipMemcpyAsync(active.p, ones.data(), active.bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  RowArgs<double> code_args(bool first) {
    RowArgs<double> a{};
    a.S = Sz.cx();
    a.Z = Z.re();
    a.D = D2.re();
    a.part = part.re();
    a.part_slices = S.Kc + S.W;
    a.part_off = 0;
    a.active = active.as<int>();
    a.theta = theta2.re();
    a.per_img = S.Kc;
    a.first = first ? 1 : 0;
    a.prox = S.p.variant == CCSC_SOLVE_POISSON2D ? 1 : 0;
    a.Y = S.Y;
    return a;
  }
  RowArgs<double> data_args(bool first) {
    const ccsc_solve_problem& p = S.p;
    RowArgs<double> a{};
    a.S = Sx.cx();
    a.D = D1.re();
    a.M = M.re();
    a.Mb = Mb.re();
    a.SM = SM.p ? SM.re() : nullptr;
    a.XO = XO.p ? XO.re() : nullptr;
    a.part = part.re();
    a.part_slices = S.Kc + S.W;
    a.part_off = S.Kc;
    a.theta = theta1.re();
    a.per_img = S.W;
    a.first = first ? 1 : 0;
    a.prox = p.variant == CCSC_SOLVE_POISSON2D ? 1 : 0;
    a.mtm_sq = p.variant == CCSC_SOLVE_INPAINT2D ? 1 : 0;
    a.obj_sm = (p.variant == CCSC_SOLVE_MULTICH || p.variant == CCSC_SOLVE_VIDEO3D) ? 1 : 0;
    a.psnr_sm = p.variant == CCSC_SOLVE_INPAINT2D ? 1 : 0;
    // PSNR window: psnr_pad = psf_radius inside the cropped image (SI:59-60)
    a.px0 = 2 * S.rx;
    a.px1 = S.X - 2 * S.rx;
    a.py0 = 2 * S.ry;
    a.py1 = S.Y - 2 * S.ry;
    a.Y = S.Y;
    return a;
  }

  void solve_bins() {
    const ccsc_solve_problem& p = S.p;
    const double invP = 1.0 / (double)S.P;
    if (p.variant == CCSC_SOLVE_INPAINT2D || p.variant == CCSC_SOLVE_POISSON2D) {
      HIPCHK(launch_solve_sm<double>(Sz.cx(), Sx.cx(), dhat.cx(), senergy.re(), S.rho, invP,
                                     (int)S.F, S.Kc, n, p.variant == CCSC_SOLVE_POISSON2D ? 1 : 0,
                                     S.X, S.Y, S.X / 2 + 1, st));
    } else {
      // zhat_k = (sum_w conj(dhat_wk) xi1_w + rho xi2_k) * invP / (rho + s), then
      // v1_w = sum_k dhat_wk zhat_k: the per-bin GEMMs of hs23.hip (dhat [K][W][F])
      HIPCHK(launch_hs_analysis<double>(dhat.cx(), Sx.cx(), Sz.cx(), senergy.re(), S.rho, Sz.cx(),
                                        (int)S.F, S.W, S.Kc, (int)n, st));
      HIPCHK(launch_hs_synth<double>(dhat.cx(), Sz.cx(), Sx.cx(), (int)S.F, S.W, S.Kc, (int)n, st));
    }
  }

  void run(ccsc_solve_outputs* out, ccsc_solvelog* log) {
    const ccsc_solve_problem& p = S.p;
    const int max_it = p.max_it;
    const bool want_trace = p.verbose != CCSC_VERBOSE_NONE && log &&
                            (log->obj || log->psnr || log->diff);
    const bool need_sums = p.tol > 0 || want_trace;
    if (log && (log->obj || log->psnr || log->diff) && log->capacity < max_it + 1)
      throw Err(CCSC_E_INVALID, "solvelog capacity < max_it + 1");
    std::vector<int> iters((size_t)n, 0), act((size_t)n, 1);
    std::vector<double> hs((size_t)(n * kRowParts));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto put = [&](double* arr, int64_t img, int it, double v) {
      if (arr && want_trace) arr[img * log->capacity + it] = v;
    };
    const double psnr_count = (double)(p.sb[0] - 2 * S.rx) * (double)(p.sb[1] - 2 * S.ry);
    const int64_t nz = n * S.Kc, nx = n * S.W;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    int live = (int)n;
    for (int i = 0; i <= max_it && live > 0; ++i) {
      const bool last = i == max_it;
      HIPCHK(launch_rows_pair<double>(last ? kRowFinalZ : kRowIterZ, code_args(i == 0), nz,
                                      data_args(i == 0), nx, S.lp.rg, lines.twr, st));
      if (need_sums) {
        HIPCHK(launch_reduce_parts<double>(part.re(), sums.re(), n, S.Kc + S.W,
                                           S.lp.rg.groups, st));
        HIPCHK(hipMemcpyAsync(hs.data(), sums.p, sums.bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool changed = false;
        for (int64_t m = 0; m < n; ++m) {
          if (!act[(size_t)m]) continue;
          const double* q = hs.data() + m * kRowParts;
          const double diff = i == 0 ? 0.0 : std::sqrt(q[0]) / std::sqrt(q[1]);   // SI:124
          iters[(size_t)m] = i;
          put(log ? log->diff : nullptr, m, i, diff);
          put(log ? log->obj : nullptr, m, i,
              p.lambda_residual * 0.5 * q[3] + p.lambda_prior * q[2]);          // SI:196-200
          if (log && log->psnr) {
            double ps = nan;
            if (XO.p) {
              const double mse = q[4] / psnr_count;                            // SI:61-66
              ps = mse > std::numeric_limits<double>::epsilon() ? 10.0 * std::log10(1.0 / mse)
                                                                : std::numeric_limits<double>::infinity();
            }
            put(log->psnr, m, i, ps);
          }
          if (i > 0 && p.tol > 0 && diff < p.tol) {                              // SI:136
            act[(size_t)m] = 0;
            --live;
            changed = true;
          }
        }
        if (changed)
          HIPCHK(hipMemcpyAsync(active.p, act.data(), active.bytes, hipMemcpyHostToDevice, st));
      } else {
        for (auto& it : iters) it = i;
      }
      if (last || live == 0) break;
      cols2(-1, nz, nx);
      solve_bins();
      cols2(+1, nz, nx);
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (log) {
      if (log->iters)
        for (int64_t m = 0; m < n; ++m) log->iters[m] = iters[(size_t)m];
      if (log->seconds) log->seconds[0] = ms * 1e-3;
    }
    // ---- outputs: z, and res = crop(real(ifft(sum_k dhat_k fft(z))) + smoothinit)
    if (out && out->z)
      HIPCHK(hipMemcpyAsync(out->z, Z.p, Z.bytes, hipMemcpyDeviceToHost, st));
    if (out && out->res) {
      lines.r2c(Z.re(), Sz.cx(), nz);
      const cpx<double>* dres = dhat_res.p ? dhat_res.cx() : dhat.cx();
      HIPCHK(launch_hs_synth<double>(dres, Sz.cx(), Sx.cx(), (int)S.F, S.W, S.Kc, (int)n, st));
      lines.inv_cols(Sx.cx(), nx);
      RowArgs<double> a{};
      a.S = Sx.cx();
      a.SM = SM.p ? SM.re() : nullptr;
      a.per_img = S.W;
      a.Y = S.Y;
      a.sbx = (int)p.sb[0];
      a.sby = (int)p.sb[1];
      a.sbt = (int)p.sb[2];
      a.rx = S.rx;
      a.ry = S.ry;
      a.rt = S.rt;
      a.clamp0 = p.variant == CCSC_SOLVE_POISSON2D ? 1 : 0;   // SP:131
      a.scale = 1.0 / (double)S.P;
      DevBuf res;
      res.alloc((size_t)(nx * p.sb[0] * p.sb[1] * p.sb[2]) * 8);
      a.res = res.re();
      HIPCHK(launch_rows<double>(kRowRes, a, nx, S.lp.rg, lines.twr, st));
      HIPCHK(hipMemcpyAsync(out->res, res.p, res.bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipStreamSynchronize(st));
  }
};

}  // namespace ccsc

using namespace ccsc;

// ---- local contrast normalisation: argument checks and the choice of path ----------

static void local_cn_check(const ccsc_ctx* ctx, const double* in, const double* out, int64_t n,
                           int32_t H, int32_t W) {
  if (!ctx || !in || !out || n < 0) throw Err(CCSC_E_INVALID, "bad arguments");
  if (H < 7 || W < 7)
    throw Err(CCSC_E_UNSUPPORTED,
              "local_cn: H and W must be at least 7 pixels (the 13x13 window reflects 6 samples "
              "per side)");
  if (!local_cn_tiled_ok(H, W))
    throw Err(CCSC_E_UNSUPPORTED, "local_cn: H * W must be below 2^31 pixels");
}

// n device images in -> out on the context's stream, synchronised on return.  The LDS
// kernel where local_cn_ok holds, unless CCSC_CN_TILED=1; else the tiled path, in chunks
// of images whose workspace stays within 256 MiB, or the CCSC_CN_WS_MB (MiB) below that
// (0: one image per chunk; a single image larger than the budget still gets its own).
// Both switches are read per call.
static void local_cn_device(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t H,
                            int32_t W) {
  const char* et = std::getenv("CCSC_CN_TILED");
  if (local_cn_ok(H, W) && !(et && et[0] == '1')) {
    HIPCHK(launch_local_cn(in, out, n, H, W, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return;
  }
  if (n == 0) return;
  size_t budget = (size_t)256 << 20;
  if (const char* eb = std::getenv("CCSC_CN_WS_MB")) {
    const long long mb = std::atoll(eb);
    if (mb >= 0 && mb < 256) budget = (size_t)mb << 20;
  }
  const int64_t per = (int64_t)H * W;
  const int64_t chunk = local_cn_tiled_chunk(n, H, W, budget);
  DevBuf ws;
  ws.alloc(local_cn_tiled_ws_bytes(chunk, H, W));
  for (int64_t i0 = 0; i0 < n; i0 += chunk)
    HIPCHK(launch_local_cn_tiled(in + i0 * per, out + i0 * per, std::min(chunk, n - i0), H, W,
                                 ws.p, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // the workspace is released on return
}

// ---- imfilter: argument checks (nothing here touches the device) --------------------

struct ImfShape {
  int dims[3], kdims[3];
  int64_t per;      // pixels per array
  int64_t ntaps;
};

static ImfShape imfilter_check(const ccsc_ctx* ctx, const double* in, const double* out, int64_t n,
                               int32_t nd, const int32_t* dims, const double* k,
                               const int32_t* kdims, int32_t boundary) {
  if (!ctx || !in || !out || !dims || !k || !kdims)
    throw Err(CCSC_E_INVALID, "imfilter: NULL ctx, in, out, dims, k or kdims");
  if (n < 0) throw Err(CCSC_E_INVALID, "imfilter: n must be >= 0");
  if (nd < 1 || nd > 3)
    throw Err(CCSC_E_INVALID, "imfilter: nd must be 1, 2 or 3, got " + std::to_string(nd));
  if (boundary < CCSC_PAD_SYMMETRIC || boundary > CCSC_PAD_ZERO)
    throw Err(CCSC_E_INVALID, "imfilter: unknown boundary " + std::to_string(boundary) +
                                  " (CCSC_PAD_SYMMETRIC, _REPLICATE or _ZERO)");
  if (in == out)
    throw Err(CCSC_E_INVALID, "imfilter: out must not alias in (a stencil cannot run in place)");
  ImfShape S;
  S.per = 1;
  S.ntaps = 1;
  for (int i = 0; i < 3; ++i) {
    const std::string dim = " in dimension " + std::to_string(i + 1);
    if (dims[i] < 1 || kdims[i] < 1)
      throw Err(CCSC_E_INVALID, "imfilter: extents must be at least 1" + dim);
    if (i >= nd && (dims[i] != 1 || kdims[i] != 1))
      throw Err(CCSC_E_INVALID, "imfilter: extents past nd must be 1" + dim);
    if (kdims[i] % 2 == 0)
      throw Err(CCSC_E_UNSUPPORTED, "imfilter: kernel extents must be odd, got " +
                                        std::to_string(kdims[i]) + dim);
    if (kdims[i] > kImfMaxExt)
      throw Err(CCSC_E_UNSUPPORTED, "imfilter: kernel extents above " +
                                        std::to_string(kImfMaxExt) + " are not supported, got " +
                                        std::to_string(kdims[i]) + dim);
    S.dims[i] = dims[i];
    S.kdims[i] = kdims[i];
    S.ntaps *= kdims[i];
    S.per *= dims[i];
    if (S.per >= ((int64_t)1 << 31))
      throw Err(CCSC_E_UNSUPPORTED, "imfilter: H * W * T must be below 2^31 pixels");
  }
  if (S.ntaps > kImfMaxTaps)
    throw Err(CCSC_E_UNSUPPORTED, "imfilter: at most " + std::to_string(kImfMaxTaps) +
                                      " taps are supported, got " + std::to_string(S.ntaps));
  return S;
}

// The kernel's taps onto the device, in the layout the kernel reads (copied on return).
static void imfilter_taps(const ImfShape& S, const double* k, DevBuf& taps) {
  std::vector<double> packed((size_t)S.ntaps);
  imfilter_pack_taps(k, S.kdims, packed.data());
  taps.alloc(packed.size() * 8);
  HIPCHK(hipMemcpy(taps.p, packed.data(), taps.bytes, hipMemcpyHostToDevice));
}

// ---- nn_fill, standardize: argument checks (nothing here touches the device) ----------

static void nn_fill_check(const ccsc_ctx* ctx, const double* in, const double* known,
                          const double* out, int64_t n, int32_t H, int32_t W) {
  if (!ctx || !in || !out) throw Err(CCSC_E_INVALID, "nn_fill: NULL ctx, in or out");
  if (n < 0) throw Err(CCSC_E_INVALID, "nn_fill: n must be >= 0");
  if (H < 1 || W < 1) throw Err(CCSC_E_INVALID, "nn_fill: extents must be at least 1");
  if (known && known == out)
    throw Err(CCSC_E_INVALID, "nn_fill: out must not alias known (the fill would overwrite "
                              "the mask it reads)");
  if (H > kFillMaxExt || W > kFillMaxExt)
    throw Err(CCSC_E_UNSUPPORTED, "nn_fill: extents above " + std::to_string(kFillMaxExt) +
                                      " are not supported (a squared distance must fit int32; "
                                      "H * W then stays below 2^31)");
}

// Planes per launch group: the int32 workspace (and a host entry's staging buffers) stay
// within 256 MiB each; a single larger plane still gets its own.
static int64_t prep_chunk(int64_t n, int64_t per) {
  return std::max<int64_t>(1, std::min<int64_t>(n, (256LL << 20) / (per * 8)));
}

static void standardize_check(const char* what, const ccsc_ctx* ctx, const double* in,
                              const double* out, const double* mean, const double* sdev,
                              int64_t planes, int64_t N) {
  const std::string w(what);
  if (!ctx || !in || !out || !mean || !sdev)
    throw Err(CCSC_E_INVALID, w + ": NULL ctx, in, out, mean or sdev");
  if (planes < 0) throw Err(CCSC_E_INVALID, w + ": planes must be >= 0");
  if (N < 2)
    throw Err(CCSC_E_INVALID, w + ": N must be at least 2 (std(., 0, 2) divides by N - 1)");
  if (!standardize_ok(N))
    throw Err(CCSC_E_UNSUPPORTED, w + ": N must be below 2^31 values per plane");
}

extern "C" {

int32_t ccsc_solve_supported(const ccsc_solve_problem* p, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!p) throw Err(CCSC_E_INVALID, "NULL problem");
    SolveSpec S;
    resolve_solve(*p, S);
  });
}

int32_t ccsc_solve(ccsc_ctx* ctx, const ccsc_solve_problem* p, const ccsc_solve_inputs* in,
                   ccsc_solve_outputs* out, ccsc_solvelog* log, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !p || !in) throw Err(CCSC_E_INVALID, "NULL ctx/problem/inputs");
    if (!ctx->subs.empty())
      throw Err(CCSC_E_UNSUPPORTED, "the solvers run on a one-device context");
    HIPCHK(hipSetDevice(ctx->device));
    Solver s(ctx, *p);
    s.setup(*in);
    s.run(out, log);
  });
}

int32_t ccsc_local_cn_dev(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t H,
                          int32_t W, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    local_cn_check(ctx, in, out, n, H, W);
    HIPCHK(hipSetDevice(ctx->device));
    local_cn_device(ctx, in, out, n, H, W);
  });
}

int32_t ccsc_local_cn(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t H,
                      int32_t W, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    local_cn_check(ctx, in, out, n, H, W);
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t per = (int64_t)H * W;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (256LL << 20) / (per * 8)));
    DevBuf a, b;
    a.alloc((size_t)(chunk * per) * 8);
    b.alloc(a.bytes);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
      const int64_t m = std::min(chunk, n - i0);
      HIPCHK(hipMemcpyAsync(a.p, in + i0 * per, (size_t)(m * per) * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      local_cn_device(ctx, a.re(), b.re(), m, H, W);
      HIPCHK(hipMemcpyAsync(out + i0 * per, b.p, (size_t)(m * per) * 8, hipMemcpyDeviceToHost,
                            ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

int32_t ccsc_imfilter_dev(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t nd,
                          const int32_t dims[3], const double* k, const int32_t kdims[3],
                          int32_t boundary, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const ImfShape S = imfilter_check(ctx, in, out, n, nd, dims, k, kdims, boundary);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf taps;
    imfilter_taps(S, k, taps);
    HIPCHK(launch_imfilter(in, out, n, S.dims, taps.re(), S.kdims, boundary, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the taps are released on return
  });
}

int32_t ccsc_imfilter(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t nd,
                      const int32_t dims[3], const double* k, const int32_t kdims[3],
                      int32_t boundary, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    const ImfShape S = imfilter_check(ctx, in, out, n, nd, dims, k, kdims, boundary);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf taps, a, b;
    imfilter_taps(S, k, taps);
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (256LL << 20) / (S.per * 8)));
    a.alloc((size_t)(chunk * S.per) * 8);
    b.alloc(a.bytes);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
      const int64_t m = std::min(chunk, n - i0);
      HIPCHK(hipMemcpyAsync(a.p, in + i0 * S.per, (size_t)(m * S.per) * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      HIPCHK(launch_imfilter(a.re(), b.re(), m, S.dims, taps.re(), S.kdims, boundary, ctx->stream));
      HIPCHK(hipMemcpyAsync(out + i0 * S.per, b.p, (size_t)(m * S.per) * 8, hipMemcpyDeviceToHost,
                            ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

int32_t ccsc_nn_fill_dev(ccsc_ctx* ctx, const double* in, const double* known, double* out,
                         int32_t* idx, int64_t n, int32_t H, int32_t W, char* err,
                         size_t errlen) {
  return guarded(err, errlen, [&] {
    nn_fill_check(ctx, in, known, out, n, H, W);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t per = (int64_t)H * W;
    const int64_t chunk = prep_chunk(n, per);
    DevBuf r;
    r.alloc((size_t)(chunk * per) * 4);
    for (int64_t i0 = 0; i0 < n; i0 += chunk)
      HIPCHK(launch_nn_fill(in + i0 * per, known ? known + i0 * per : nullptr, out + i0 * per,
                            idx ? idx + i0 * per : nullptr, r.as<int>(), std::min(chunk, n - i0),
                            H, W, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the workspace is released on return
  });
}

int32_t ccsc_nn_fill(ccsc_ctx* ctx, const double* in, const double* known, double* out,
                     int32_t* idx, int64_t n, int32_t H, int32_t W, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    nn_fill_check(ctx, in, known, out, n, H, W);
    if (n == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t per = (int64_t)H * W;
    const int64_t chunk = prep_chunk(n, per);
    DevBuf a, k, ix, r;
    a.alloc((size_t)(chunk * per) * 8);          // filled in place
    if (known) k.alloc(a.bytes);
    if (idx) ix.alloc((size_t)(chunk * per) * 4);
    r.alloc((size_t)(chunk * per) * 4);
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
      const int64_t m = std::min(chunk, n - i0);
      const size_t cnt = (size_t)(m * per);
      HIPCHK(hipMemcpyAsync(a.p, in + i0 * per, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
      if (known)
        HIPCHK(hipMemcpyAsync(k.p, known + i0 * per, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(launch_nn_fill(a.re(), k.re(), a.re(), ix.as<int>(),
                            r.as<int>(), m, H, W, ctx->stream));
      HIPCHK(hipMemcpyAsync(out + i0 * per, a.p, cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
      if (idx)
        HIPCHK(hipMemcpyAsync(idx + i0 * per, ix.p, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

int32_t ccsc_standardize_dev(ccsc_ctx* ctx, const double* in, double* out, double* mean,
                             double* sdev, int64_t planes, int64_t N, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    standardize_check("standardize", ctx, in, out, mean, sdev, planes, N);
    if (planes == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf ws;
    ws.alloc((size_t)standardize_ws_bytes(planes, N));
    HIPCHK(launch_standardize(in, out, mean, sdev, planes, N, ws.p, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the workspace is released on return
  });
}

int32_t ccsc_standardize(ccsc_ctx* ctx, const double* in, double* out, double* mean, double* sdev,
                         int64_t planes, int64_t N, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    standardize_check("standardize", ctx, in, out, mean, sdev, planes, N);
    if (planes == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t chunk = prep_chunk(planes, N);
    DevBuf a, ms, ws;
    a.alloc((size_t)(chunk * N) * 8);            // normalised in place
    ms.alloc((size_t)chunk * 16);                // the chunk's means, then its sdevs
    ws.alloc((size_t)standardize_ws_bytes(chunk, N));
    for (int64_t i0 = 0; i0 < planes; i0 += chunk) {
      const int64_t m = std::min(chunk, planes - i0);
      double* dm = ms.re();
      double* ds = dm + chunk;
      HIPCHK(hipMemcpyAsync(a.p, in + i0 * N, (size_t)(m * N) * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      HIPCHK(launch_standardize(a.re(), a.re(), dm, ds, m, N, ws.p, ctx->stream));
      HIPCHK(hipMemcpyAsync(out + i0 * N, a.p, (size_t)(m * N) * 8, hipMemcpyDeviceToHost,
                            ctx->stream));
      HIPCHK(hipMemcpyAsync(mean + i0, dm, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipMemcpyAsync(sdev + i0, ds, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

int32_t ccsc_unstandardize_dev(ccsc_ctx* ctx, const double* in, double* out, const double* mean,
                               const double* sdev, int64_t planes, int64_t N, char* err,
                               size_t errlen) {
  return guarded(err, errlen, [&] {
    standardize_check("unstandardize", ctx, in, out, mean, sdev, planes, N);
    if (planes == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(launch_unstandardize(in, out, mean, sdev, planes, N, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

int32_t ccsc_unstandardize(ccsc_ctx* ctx, const double* in, double* out, const double* mean,
                           const double* sdev, int64_t planes, int64_t N, char* err,
                           size_t errlen) {
  return guarded(err, errlen, [&] {
    standardize_check("unstandardize", ctx, in, out, mean, sdev, planes, N);
    if (planes == 0) return;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t chunk = prep_chunk(planes, N);
    DevBuf a, ms;
    a.alloc((size_t)(chunk * N) * 8);            // restored in place
    ms.alloc((size_t)chunk * 16);
    for (int64_t i0 = 0; i0 < planes; i0 += chunk) {
      const int64_t m = std::min(chunk, planes - i0);
      double* dm = ms.re();
      double* ds = dm + chunk;
      HIPCHK(hipMemcpyAsync(a.p, in + i0 * N, (size_t)(m * N) * 8, hipMemcpyHostToDevice,
                            ctx->stream));
      HIPCHK(hipMemcpyAsync(dm, mean + i0, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(ds, sdev + i0, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(launch_unstandardize(a.re(), a.re(), dm, ds, m, N, ctx->stream));
      HIPCHK(hipMemcpyAsync(out + i0 * N, a.p, (size_t)(m * N) * 8, hipMemcpyDeviceToHost,
                            ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
  });
}

}  // extern "C"
