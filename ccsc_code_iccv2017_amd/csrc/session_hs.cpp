// libccsc session of the 2-3D hyperspectral learner (L23 = 2-3D/DictionaryLearning/
// admm_learn.m).
#include "recon.hpp"
#include "session.hpp"
#include "slice.hpp"

#include <chrono>

namespace ccsc {
namespace {

// One non-consensus ADMM over all n images (one block).  Its d-solve sums over every image
// per frequency.  Several ranks (one process per GPU, images sharded in contiguous runs,
// shard()): each rank forms the Gram of its images (gramchol_big.hip, rho on rank 0 only) and
// the right-hand sides Z^H xi1 of its images, both are summed over the ranks (allreduce), and
// every rank factors and solves the same system; the objective's sums, the z change norms
// and max(b) (L23:36) are reduced too.  (Device state: mem_plan_hs, plan.cpp.)
struct SessionHS final : Session {
  Geom g;
  Grid2D G;
  Route rt;
  std::vector<BufRow> rows;   // the memory plan: buf[i] is allocated from rows[i]
  int r, s, SS, K, W, KG, P, F, sbx, sby;
  int n;
  double th_D1 = 0, th_Z1 = 0, th_Z2 = 0, gamma_h = 0;

  DevBuf buf[bh::count];
  DevBuf &tw = buf[bh::tw], &bdev = buf[bh::b], &smp = buf[bh::smp], &v = buf[bh::v],
         &eD = buf[bh::eD], &eZ = buf[bh::eZ], &D = buf[bh::D], &yD = buf[bh::yD],
         &Dold = buf[bh::Dold], &z = buf[bh::z], &eZ2 = buf[bh::eZ2], &zold = buf[bh::zold],
         &Zh = buf[bh::Zh], &Xw = buf[bh::Xw], &Xi = buf[bh::Xi], &Ch = buf[bh::Ch],
         &Dh = buf[bh::Dh], &Dhold = buf[bh::Dhold], &L = buf[bh::L], &h = buf[bh::h],
         &sden = buf[bh::sden], &Usup = buf[bh::Usup], &supp = buf[bh::supp],
         &dnorm = buf[bh::dnorm], &part = buf[bh::part], &pair = buf[bh::pair];
  // slices past one CU's LDS (Geom::gp): the global line passes of recon.hip with the
  // elementwise halves of the fused slice kernels in gslice.hip over the real scratch gR
  bool gp = false;
  DevBuf& gR = buf[bh::gR];
  SliceXf xf;   // the slice transforms both learners run

  bool dist = false;   // rt.dist
  int64_t i0 = 0;      // first image of this rank
  double obj = std::numeric_limits<double>::quiet_NaN();
  double obj_filter = obj, obj_z = obj;

  SessionHS(ccsc_ctx* c, const ccsc_problem& pin, const double* b, const double* smooth_init,
            const double* d0, const double* z0)
      : Session(c, pin) {
    resolve_problem(p);
    if (p.variant != CCSC_HS23) throw Err(CCSC_E_INVALID, "SessionHS runs the 2-3D learner only");
    check_supported(p, &g);
    rt = route_hs(p, g, ctx->rank, ctx->nranks, ctx->rccl_self);
    dist = rt.dist;
    i0 = rt.b0;
    if (!b || !smooth_init) throw Err(CCSC_E_INVALID, "b and smooth_init must not be NULL");
    G = g.G;
    gp = g.gp;
    rows = mem_plan_hs(p, g, rt);
    r = p.psf / 2;
    s = p.psf;
    SS = s * s;
    K = p.K;
    W = p.views[0];
    KG = K * W;
    P = G.X * G.Y;
    F = G.F;
    sbx = (int)p.sb[0];
    sby = (int)p.sb[1];
    n = (int)rt.nb;   // this rank's images
    if (r > sbx || r > sby)
      throw Err(CCSC_E_UNSUPPORTED, "symmetric padding wider than the image (L23:19)");

    alloc_plan(rows, buf, bh::count, "");
    auto staging = [&](int i) -> DevBuf& {
      buf[i].alloc(rows[i].bytes);
      return buf[i];
    };
    upload_twiddles(tw, make_twiddles(G));
    xf = {g, r, false, st, &tw, nullptr, &gR};
    if (gp) xf.lines.setup(g.lp, st, buf[bh::gtwr], buf[bh::gtwc]);

    // data: b and smoothinit = padarray(smooth_init, [r r 0 0], 'symmetric') (L23:19)
    HIPCHK(hipMemcpy(bdev.p, b, bdev.bytes, hipMemcpyHostToDevice));
    {
      DevBuf& stage = staging(bh::stage);
      HIPCHK(hipMemcpy(stage.p, smooth_init, stage.bytes, hipMemcpyHostToDevice));
      HIPCHK(launch_pad_symmetric<double>(stage.re(), smp.re(), sbx, sby, r, G.X,
                                          G.Y, (int64_t)W * n, st));
      HIPCHK(hipStreamSynchronize(st));
      stage.release();
    }
    // gammas (L23:35-38): gamma_heuristic = 60 lambda / max(b(:))
    HIPCHK(launch_max<double>(bdev.re(), (int64_t)((size_t)sbx * sby * W * n),
                              part.re(), pair.re(), st));
    double bmax = 0;
    HIPCHK(hipMemcpyAsync(&bmax, pair.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (dist) {   // max over the ranks through the sum collective: one slot per rank
      std::vector<double> mx((size_t)ctx->nranks, 0.0);
      mx[(size_t)ctx->rank] = bmax;
      DevBuf& rm = staging(bh::rm);
      HIPCHK(hipMemcpy(rm.p, mx.data(), rm.bytes, hipMemcpyHostToDevice));
      ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, rm.re(), mx.size());
      HIPCHK(hipMemcpyAsync(mx.data(), rm.p, rm.bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      rm.release();
      bmax = *std::max_element(mx.begin(), mx.end());
    }
    if (!(bmax > 0)) throw Err(CCSC_E_INVALID, "max(b(:)) must be positive (L23:36)");
    gamma_h = 60.0 * p.lambda_prior / bmax;
    const double gD1 = gamma_h / p.rho_d;                // gammas_D = [gh/5000, gh]  (L23:37)
    const double gZ1 = gamma_h * W / p.rho_z;            // gammas_Z = [gh/500, gh]   (L23:38)
    th_D1 = p.lambda_residual / gD1;                     // lambda(1)/gammas_D(1)     (L23:112)
    th_Z1 = p.lambda_residual / gZ1;                     // lambda(1)/gammas_Z(1)     (L23:175)
    th_Z2 = p.lambda_prior / gamma_h;                    // lambda(2)/gammas_Z(2)     (L23:176)

    // filters: d0 [s,s,K] replicated over W, embedded at circshift(-r) (L23:54-56)
    {
      DevBuf &d0dev = staging(bh::d0), &d0w = staging(bh::d0w);
      if (d0) HIPCHK(hipMemcpy(d0dev.p, d0, d0dev.bytes, hipMemcpyHostToDevice));
      else HIPCHK(launch_randn<double>(d0dev.re(), (int64_t)SS * K, p.seed ^ 0xd0d0d0d0ULL, 0, st));
      HIPCHK(launch_rep_filters<double>(d0dev.re(), d0w.re(), SS, W, K, st));
      HIPCHK(launch_embed_filters<double>(d0w.re(), D.re(), 1, KG, s, G, 1, st));
      HIPCHK(hipStreamSynchronize(st));
      d0w.release();     // (the order their scope ended in)
      d0dev.release();
    }
    HIPCHK(hipMemsetAsync(yD.p, 0, yD.bytes, st));
    HIPCHK(hipMemsetAsync(eD.p, 0, eD.bytes, st));
    HIPCHK(hipMemsetAsync(eZ.p, 0, eZ.bytes, st));
    HIPCHK(hipMemsetAsync(eZ2.p, 0, eZ2.bytes, st));
    // codes z = randn(size_z) (L23:69): this rank's images of the one global stream, so
    // the draw does not depend on the rank count
    if (z0) HIPCHK(hipMemcpy(z.p, z0, z.bytes, hipMemcpyHostToDevice));
    else
      HIPCHK(launch_randn<double>(z.re(), (int64_t)(z.bytes / 8), p.seed,
                                  (uint64_t)i0 * (uint64_t)K * (uint64_t)P, st));
    // d_hat = fft2(d) (L23:57); u_D{2} of the first d-iteration = Pi(d - 0) (L23:113)
    xf.fwd_embed(D.re(), G.X, G.Y, 1, 0, Dh.cx(), KG);
    HIPCHK(launch_gather_support<double>(D.re(), yD.re(), supp.re(), KG, r, G.X, G.Y, st));
    HIPCHK(launch_project<double>(supp.re(), Usup.re(), KG, SS, 1.0, st));
    obj = objective_fresh();                              // L23:72
    obj_filter = obj_z = obj;                             // L23:82-83
    lg.start(p, obj);
  }

  // ---- slice transforms: the fused LDS slice kernels, or on global-pass slices the line
  // passes of recon.hip around gslice.hip's elementwise halves (SliceXf for the ones the
  // consensus learners run too).  On global passes the inverse consumes its input spectrum
  // (the column pass runs in place): Xi and Zh are dead after their C2R here.
  // v = real(ifft2(Xi)), DZ (nullable), the objective's data parts (k_hs_c2r_v)
  void c2r_v(double* DZ) {
    const int64_t cnt = (int64_t)W * n;
    if (!gp) {
      HIPCHK(launch_hs_c2r_v<double>(Xi.cx(), v.re(), bdev.re(), smp.re(), DZ, part.re(), cnt,
                                     tw.cx(), G, r, sbx, sby, st));
      return;
    }
    xf.lines.c2r(Xi.cx(), gR.re(), cnt);
    HIPCHK(launch_gp_hs_epilog<double>(kHsV, gR.re(), v.re(), bdev.re(), smp.re(), DZ, part.re(),
                                       G.X, G.Y, r, sbx, sby, 1.0 / (double)P, cnt, st));
  }
  // masked-data split with dual e, into Xi (k_hs_data_r2c)
  void data_r2c(DevBuf& e, double theta) {
    const int64_t cnt = (int64_t)W * n;
    if (!gp) {
      HIPCHK(launch_hs_data_r2c<double>(v.re(), e.re(), bdev.re(), smp.re(), Xi.cx(), cnt, tw.cx(),
                                        G, r, sbx, sby, theta, st));
      return;
    }
    HIPCHK(launch_gp_hs_prolog<double>(kHsData, v.re(), e.re(), bdev.re(), smp.re(), gR.re(), G.X,
                                       G.Y, r, sbx, sby, theta, cnt, st));
    xf.lines.r2c(gR.re(), Xi.cx(), cnt);
  }
  // sparsity split of the Z-phase with dual eZ2, into Zh (k_hs_z_r2c)
  void z_r2c() {
    const int64_t cnt = (int64_t)K * n;
    if (!gp) {
      HIPCHK(launch_hs_z_r2c<double>(z.re(), eZ2.re(), Zh.cx(), cnt, tw.cx(), G, th_Z2, st));
      return;
    }
    HIPCHK(launch_gp_hs_prolog<double>(kHsSparse, z.re(), eZ2.re(), bdev.re(), smp.re(), gR.re(),
                                       G.X, G.Y, r, sbx, sby, th_Z2, cnt, st));
    xf.lines.r2c(gR.re(), Zh.cx(), cnt);
  }
  // z = real(ifft2(zhat)), sum |z| per slice (k_hs_c2r_z)
  void c2r_z() {
    const int64_t cnt = (int64_t)K * n;
    if (!gp) {
      HIPCHK(launch_hs_c2r_z<double>(Zh.cx(), z.re(), part.re(), cnt, tw.cx(), G, st));
      return;
    }
    xf.lines.c2r(Zh.cx(), gR.re(), cnt);
    HIPCHK(launch_gp_hs_epilog<double>(kHsZ, gR.re(), z.re(), bdev.re(), smp.re(), nullptr,
                                       part.re(), G.X, G.Y, r, sbx, sby, 1.0 / (double)P, cnt, st));
  }

  // v = real(ifft2(H zhat)) from Xi (= H zhat) and the objective of (z, d_hat)
  // (objectiveFunction, L23:326-343); pair[2] must hold sum |z|.
  double finish_objective() {
    c2r_v(nullptr);
    HIPCHK(launch_sum_pairs<double>(part.re(), W * n, pair.re(), st));
    // the data term and sum |z| over every rank's images, reduced in a copy: pair[2] (this
    // rank's sum |z|) serves every objective of a d-phase
    const double* ps = pair.re();
    if (dist) {
      HIPCHK(hipMemcpyAsync(pair.re() + 8, ps, 4 * sizeof(double), hipMemcpyDeviceToDevice, st));
      ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, pair.re() + 8, 4);
      ps = pair.re() + 8;
    }
    double h4[4];
    HIPCHK(hipMemcpyAsync(h4, ps, sizeof h4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return p.lambda_residual * 0.5 * h4[0] + p.lambda_prior * W * h4[2];   // g_z: z repeated W times (L23:332,338)
  }
  // zhat = fft2(z) (L23:100,158,234), sum |z|, v = H z and the objective
  double objective_now() override { return objective_fresh(); }
  double objective_fresh() {
    xf.fwd_embed(z.re(), G.X, G.Y, 1, 0, Zh.cx(), (int64_t)K * n);
    HIPCHK(launch_norms<double>(z.re(), nullptr, (int64_t)z.bytes / 8, part.re(),
                                pair.re() + 2, st));
    HIPCHK(launch_hs_synth<double>(Dh.cx(), Zh.cx(), Xi.cx(), F, W, K, n, st));
    return finish_objective();
  }
  // global: a and b are rank-local (z; D is the same on every rank)
  double rel_change(const DevBuf& a, const DevBuf& b, bool global = false) {
    HIPCHK(launch_norms<double>(a.re(), b.re(), (int64_t)a.bytes / 8,
                                part.re(), pair.re() + 4, st));
    if (global && dist) ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, pair.re() + 4, 2);
    double h2[2];
    HIPCHK(hipMemcpyAsync(h2, pair.re() + 4, sizeof h2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return std::sqrt(h2[0]) / std::sqrt(h2[1]);
  }

  // ---- one outer iteration (L23:86-226) ---------------------------------------
  void outer_iteration() override {
    const auto t0 = std::chrono::steady_clock::now();
    const double obj_min = std::min(obj_filter, obj_z);   // L23:94
    HIPCHK(hipMemcpyAsync(Dold.p, D.p, D.bytes, hipMemcpyDeviceToDevice, st));    // d_old (L23:95)
    HIPCHK(hipMemcpyAsync(Dhold.p, Dh.p, Dh.bytes, hipMemcpyDeviceToDevice, st)); // d_hat_old
    // z_hat = fft2(z) (L23:100) and v_D{1} = H z of the first d-iteration (L23:108)
    objective_fresh();
    // opt_f = (Z_f' Z_f + rho I)^-1 as a Cholesky factor per bin (L23:290)
    // on the matrix cores (gramchol.hip, K <= 192; no right-hand side here: NV = 0)
    if (rt.dfactor == DFactor::WBig) {
      HIPCHK(launch_wbig_gram(Zh.cx(), Zh.cx(), Xw.cx(), L.cx(), h.cx(), F, K, n, p.rho_d, 0, st));
    } else if (rt.dfactor == DFactor::Big) {
      // the Gram of this rank's images (rho I on rank 0 only), summed over the ranks, then
      // the same Cholesky on every rank
      HIPCHK(launch_gram_big(Zh.cx(), Zh.cx(), Xw.cx(), L.cx(), h.cx(), F, K, n,
                             ctx->rank == 0 ? p.rho_d : 0.0, 0, st, false));
      ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, L.re(), (size_t)2 * F * (K * (K + 1) / 2));
      HIPCHK(launch_chol_big(L.cx(), F, K, st));
    } else
      HIPCHK(launch_gram_chol_mf(Zh.cx(), Zh.cx(), L.cx(), h.cx(), F, K, n, p.rho_d, 0, st));
    // 64 < K <= 112: the tile d-solve over the W wavelengths (factor read once per solve)
    if (rt.dsolve == DSolve::Tile) HIPCHK(launch_invert_diag(L.cx(), F, K, st));
    for (int id = 0; id < p.max_it_d; ++id) {                                    // L23:102
      // c = 1: masked data split (L23:112, 117, 120-121)
      data_r2c(eD, th_D1);
      // c = 2: kernel constraint split, y = -d_D{2} (L23:113, 117, 120-121)
      xf.dual_r2c(D.re(), yD.re(), Usup.re(), Ch.cx(), KG, KG);
      // d_hat = opt (Z' xi1 + rho xi2) per (bin, wavelength)  (L23:125, 289-295)
      HIPCHK(launch_hs_corr<double>(Zh.cx(), Xi.cx(), h.cx(), F, W, K, n, st));
      if (dist) ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, h.re(), (size_t)2 * F * W * K);
      if (rt.dfactor == DFactor::WBig)
        HIPCHK(launch_wbig_solve(L.cx(), h.cx(), Ch.cx(), Dh.cx(), 1, F, K, n, p.rho_d, W, st));
      else if (rt.dsolve == DSolve::Tile)
        HIPCHK(launch_dsolve_tile(L.cx(), h.cx(), Ch.cx(), Dh.cx(), 1, F, K, p.rho_d, W, st));
      else
        HIPCHK(launch_dsolve<double>(L.cx(), h.cx(), Ch.cx(), Dh.cx(), 1, F, K, p.rho_d, W, st));
      // d = real(ifft2(d_hat)) (L23:126); support of d - d_D{2} -> u_D{2} of the next d-iteration
      xf.c2r_dout(Dh.cx(), Ch.cx(), D.re(), yD.re(), supp.re(), dnorm.re(), 0, KG);
      HIPCHK(launch_project<double>(supp.re(), Usup.re(), KG, SS, 1.0, st));
      // objective (L23:132); its H z is v_D{1} of the next d-iteration (z is fixed here)
      HIPCHK(launch_hs_synth<double>(Dh.cx(), Zh.cx(), Xi.cx(), F, W, K, n, st));
      obj = finish_objective();
      lg.tr_od[lg.d_slot(id)] = obj;
    }
    obj_filter = obj;                                                            // L23:139
    const double d_diff = rel_change(D, Dold);                                   // L23:142-146
    lg.tr_dd[lg.d_slot(0)] = d_diff;

    // ---- Z-phase (L23:149-200) ----
    // 1 / (rho + sum_{w,k} |d_hat|^2) per bin (L23:262-268, 317)
    HIPCHK(launch_sden<double>(Dh.cx(), sden.re(), F, KG, p.rho_z, 1.0, st));
    HIPCHK(hipMemcpyAsync(zold.p, z.p, z.bytes, hipMemcpyDeviceToDevice, st));  // z_old (L23:159)
    // v = H z is current: the last D objective used z_hat = fft2(z) (L23:158)
    for (int iz = 0; iz < p.max_it_z; ++iz) {                                    // L23:165
      data_r2c(eZ, th_Z1);                                                       // L23:175,180,183-184
      z_r2c();                                                                   // L23:176,180,183-184
      HIPCHK(launch_hs_analysis<double>(Dh.cx(), Xi.cx(),
                                        Zh.cx(), sden.re(), p.rho_z,
                                        Zh.cx(), F, W, K, n, st));  // L23:188, 302-324
      // objective (L23:195); H zhat is v_Z{1} of the next z-iteration (L23:171) -- formed
      // before the C2R of zhat, which consumes Zh on global-pass slices
      HIPCHK(launch_hs_synth<double>(Dh.cx(), Zh.cx(), Xi.cx(), F, W, K, n, st));
      c2r_z();                                                                   // L23:189
      HIPCHK(launch_sum_pairs<double>(part.re(), K * n, pair.re() + 2, st));
      obj = finish_objective();
      lg.tr_oz[lg.z_slot(iz)] = obj;
    }
    obj_z = obj;                                                                 // L23:202
    int flags = 0;
    if (obj_min <= obj_filter && obj_min <= obj_z) {                             // L23:204-213 (Q16)
      // roll back to the iterate before this outer iteration and stop
      HIPCHK(hipMemcpyAsync(z.p, zold.p, z.bytes, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(Dh.p, Dhold.p, Dh.bytes, hipMemcpyDeviceToDevice, st));
      xf.c2r_plain(Dh.cx(), Ch.cx(), D.re(), KG);   // D = real(ifft2(Dh)); Dh stays intact
      obj = objective_fresh();
      lg.finished = true;
      flags |= 1;
    } else {
      const double z_diff = rel_change(z, zold, true);                           // L23:216-220
      lg.tr_zd[lg.z_slot(0)] = z_diff;
      if (z_diff < p.tol && d_diff < p.tol) lg.finished = true;                     // L23:223
    }
    HIPCHK(hipStreamSynchronize(st));
    const double secs =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    lg.push(obj_filter, obj_z, secs, p.max_it_d, p.max_it_z, flags);
  }

  void results(ccsc_outputs* out) override {
    if (!out) return;
    if (out->d_res) {
      // d_res = circshift(d, [r r 0 0])(1:2r+1, 1:2r+1, :, :)  (L23:231-232)
      std::vector<double> Dh_((size_t)KG * P);
      HIPCHK(hipMemcpy(Dh_.data(), D.p, D.bytes, hipMemcpyDeviceToHost));
      crop_filters(Dh_, out->d_res, KG, s, r, G, 1, P);
    }
    if (out->z_res) HIPCHK(hipMemcpy(out->z_res, z.p, z.bytes, hipMemcpyDeviceToHost));
    if (out->DZ) {
      // Dz = real(ifft2(sum_k d_hat .* fft2(z))) + smoothinit  (L23:234-235)
      DevBuf dz;
      dz.alloc(v.bytes);
      xf.fwd_embed(z.re(), G.X, G.Y, 1, 0, Zh.cx(), (int64_t)K * n);
      HIPCHK(launch_hs_synth<double>(Dh.cx(), Zh.cx(), Xi.cx(), F, W, K, n, st));
      c2r_v(dz.re());
      HIPCHK(hipStreamSynchronize(st));   // st is non-blocking: hipMemcpy does not order after it
      HIPCHK(hipMemcpy(out->DZ, dz.p, dz.bytes, hipMemcpyDeviceToHost));
    }
    if (out->obj_val) *out->obj_val = obj;   // the last objective the learner evaluated
  }

  // The codes as results() copies them into z_res: one column of X Y K values per image.
  const double* codes_dense(int64_t* M, int64_t* nloc) override {
    HIPCHK(hipStreamSynchronize(st));
    *nloc = n;
    *M = (int64_t)K * P;
    return z.re();
  }
};

}  // namespace

std::unique_ptr<Session> make_session_hs(ccsc_ctx* ctx, const ccsc_problem& p, const double* b,
                                         const double* smooth_init, const double* d0,
                                         const double* z0) {
  return std::unique_ptr<Session>(new SessionHS(ctx, p, b, smooth_init, d0, z0));
}

}  // namespace ccsc
