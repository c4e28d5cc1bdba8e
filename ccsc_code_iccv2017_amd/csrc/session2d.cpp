// libccsc session of the consensus learners: the device buffers from the memory plan of
// plan.hpp and the outer ADMM schedule on the route it resolved.
//
// Schedule of one outer iteration (dP:89-190; dZ:90-194), per rank:
//   precompute  for each local block: R2C of its z slices -> Zh;
//               gram+cholesky -> L_f, h_f                       (dP:95-99)
//   d-loop      dual+R2C -> C ; dsolve -> Dhat ; C2R -> D, support(D+y)
//               -> local sum -> RCCL all-reduce -> projection u (dP:103-134)
//   z-prep      dhat = Dhat of global block 1 (RCCL broadcast), sden  (dP:143)
//   z-loop      fused z-iteration kernel over the local patches   (dP:147-168)
#include "recon.hpp"
#include "session.hpp"
#include "slice.hpp"

namespace ccsc {
namespace {

// Session of every consensus learner: dP, dZ, the 4D light-field learner (2D
// spatial convolution, NV = U*V views share the codes, L4:18-21) and the 3D
// learner (Tn > 1: plane transforms + t-direction FFT, L3).
struct Session2D final : Session {
  Geom g;
  Grid2D G;     // plane grid (g.G)
  Route rt;     // the kernels this problem runs on (plan.hpp)
  std::vector<BufRow> rows;   // the memory plan: buf[i] is allocated from rows[i]
  int r, s, K, ni, P, F, Kp;   // P, F: voxels / half-spectrum bins per slice (all dims)
  int SS;       // filter support size (2r+1)^ndim
  int Tn;       // 3D: t extent of the padded grid (1 otherwise)
  int NV, KG;   // views, filter slices per block (K * NV)
  bool is4, is3;
  // the diagonal-tile inversion of block j runs on st2 beside block j+1's precompute R2C
  hipStream_t st2 = nullptr;
  hipEvent_t ev_g = nullptr, ev_i = nullptr;
  // 110 grid: block j+1's precompute R2C (k_zhat_line, into the other of Zh / Zh2) runs on
  // st3 beside block j's Gram/Cholesky, filling that kernel's last partial round
  hipStream_t st3 = nullptr;
  hipEvent_t ev_s = nullptr, ev_z = nullptr, ev_gz[2] = {nullptr, nullptr};
  // 110 grid, tol = 0, >= 512 patches: a z-phase's launches split over two streams (patches [0, np/2) on st,
  // the rest on st3, idle during the z-phase), so each stream's next launch starts as soon as
  // its own half is done and fills the other's partial last round of workgroups (a C2 launch
  // is 39.06 rounds of one workgroup per CU); the halves couple only at the phase ends
  bool zsplit_open = false;
  hipEvent_t zsp_a = nullptr;
  int zsp_n = 0;
  int64_t N, nbl, b0, np;
  bool owner0;
  double theta;

  DevBuf buf[b2::count];
  DevBuf &tw = buf[b2::tw], &bdev = buf[b2::b], &Bhat = buf[b2::Bhat], &z = buf[b2::z],
         &yz = buf[b2::yz], &cbuf = buf[b2::cbuf], &D = buf[b2::D], &yD = buf[b2::yD],
         &Usup = buf[b2::Usup], &ssum = buf[b2::ssum], &supp = buf[b2::supp], &Ch = buf[b2::Ch],
         &Dh = buf[b2::Dh], &L = buf[b2::L], &h = buf[b2::h], &Zh = buf[b2::Zh],
         &Zh2 = buf[b2::Zh2], &Xbig = buf[b2::Xbig], &dhat = buf[b2::dhat],
         &dtmp = buf[b2::dtmp], &sden = buf[b2::sden], &dnorm = buf[b2::dnorm],
         &znorm = buf[b2::znorm], &part = buf[b2::part], &pair = buf[b2::pair], &E = buf[b2::E];
  // 2D z-phase state (zsplit.hip): zmode 0 = (z, y) materialised in `z`, `yz`;
  // zmode 1 = `z` holds the pre-threshold state a = z + y, W the last w and `dw`
  // the filter spectrum w was solved with (dhat, or dhatw after the next z-prep
  // replaced dhat); `yz` is then stale until materialize_z().
  DevBuf &W = buf[b2::W], &dhatw = buf[b2::dhatw];
  int zmode = 0;
  const cpx<double>* dw = nullptr;
  // zmode 2 = register-line z-step (zline.hip, the 110 grid with tol = 0): `z` holds a
  // in state order, W the last w in bin-slot order solved with dws (dhs or dhws);
  // Bhs / dhs / sdens: B^, the current filter spectrum and sden in bin-slot order.
  bool zl_on = false;   // rt.z == ZStep::Line
  DevBuf &Bhs = buf[b2::Bhs], &dhs = buf[b2::dhs], &dhws = buf[b2::dhws],
         &sdens = buf[b2::sdens];
  const cpx<double>* dws = nullptr;
  // What the shared buffer `yz` holds while the state is in zmode 2.  Other: y, the 3D / 4D /
  // global-pass state a, or stale contents.  tol > 0 (state order) -- ZPrev: the z of the
  // iterate before the current one (the next launch measures the current iterate against
  // it), ZCur: the current iterate's z (its test is done).  tol = 0 with rt.zemit -- Spectra:
  // the code spectra of the current state, [np][K][F] in bin-slot order as the phase's last
  // z-launch emitted them (twice fft2(u - y), without the term of w); the D-precompute reads
  // them.  One tag serves both because a session has one tol: ZPrev / ZCur arise only with
  // tol > 0, Spectra only with tol = 0.  Every z-launch and whatever writes `yz` sets it.
  enum class YzHolds { Other, ZPrev, ZCur, Spectra };
  YzHolds yzh = YzHolds::Other;
  // 3D: t-FFT twiddles, objective scratch (also the global path's)
  DevBuf &twt = buf[b2::twt], &oacc = buf[b2::oacc], &odz = buf[b2::odz];
  // 2D slices past one CU's LDS (Geom::gp): global line passes (xf.lines, recon.hip), and
  // the real scratch the elementwise stages (gslice.hip) read and write
  bool gp = false;
  DevBuf &gR = buf[b2::gR], &Cg = buf[b2::Cg];
  SliceXf xf;   // the slice transforms: fwd_embed, dual_r2c, c2r_dout
  // 3D with k_tsolve3 (rt.tsolve_tc, its t plan rt.gt2): the plan's twiddles; B^, the filter
  // spectrum and sden in its tile order
  DevBuf &twt2 = buf[b2::twt2];
  DevBuf &BhatT = buf[b2::BhatT], &dhatT = buf[b2::dhatT], &sdenT = buf[b2::sdenT];
  int tsolve_ppw = 16;          // patches per k_tsolve3 workgroup
  bool c_ready = false;         // 3D: the z-step spectrum C already holds the next forward

  double last_d = std::numeric_limits<double>::infinity();
  double last_z = std::numeric_limits<double>::infinity();
  double obj_filter = std::numeric_limits<double>::quiet_NaN();
  double obj_z = std::numeric_limits<double>::quiet_NaN();

  // profiling
  bool prof = false;
  struct Rec { int id; hipEvent_t a, b; int n = 1; int64_t blocks = 1; };   // n launches between a and b
  std::vector<Rec> recs;
  EventPool pool;
  int64_t k_launch[5] = {0, 0, 0, 0, 0};
  double k_ms[5] = {0, 0, 0, 0, 0};
  // blocks the launches of id 1 covered (one per block launch, nbl per grouped launch)
  int64_t k_blocks1 = 0;

  template <typename Fn>
  void timed(int id, Fn&& fn, int64_t blocks = 1) {
    if (!prof) {
      fn();
      return;
    }
    Rec rc{id, pool.get(), pool.get(), 1, blocks};
    HIPCHK(hipEventRecord(rc.a, st));
    fn();
    HIPCHK(hipEventRecord(rc.b, st));
    recs.push_back(rc);
  }
  void drain_records() {
    for (auto& rc : recs) {
      float ms = 0;
      HIPCHK(hipEventSynchronize(rc.b));
      HIPCHK(hipEventElapsedTime(&ms, rc.a, rc.b));
      k_launch[rc.id] += rc.n;
      if (rc.id == 1) k_blocks1 += rc.blocks;
      k_ms[rc.id] += ms;
      pool.put(rc.a);
      pool.put(rc.b);
    }
    recs.clear();
  }

  ~Session2D() {
    if (st) hipStreamSynchronize(st);
    if (st2) {
      hipStreamSynchronize(st2);
      hipStreamDestroy(st2);
    }
    if (ev_g) hipEventDestroy(ev_g);
    if (ev_i) hipEventDestroy(ev_i);
    if (st3) {
      hipStreamSynchronize(st3);
      hipStreamDestroy(st3);
    }
    for (hipEvent_t e : {ev_s, ev_z, ev_gz[0], ev_gz[1]})
      if (e) hipEventDestroy(e);
    for (auto& rc : recs) {
      hipEventDestroy(rc.a);
      hipEventDestroy(rc.b);
    }
  }

  // the objective is refreshed after every d- / z-iteration (the reference's verbose rules
  // are the same for both phases)
  bool verbose_refresh() const { return objective_refresh(p); }   // (plan.cpp: the route reads it too)

  Session2D(ccsc_ctx* c, const ccsc_problem& pin, const double* b, const double* d0,
            const double* z0)
      : Session(c, pin) {
    resolve_problem(p);
    check_supported(p, &g);
    G = g.G;
    rt = route2d(p, g, ctx->rank, ctx->nranks, ctx->rccl_self);
    rows = mem_plan2d(p, g, rt);
    r = p.psf / 2;
    s = p.psf;
    K = p.K;
    ni = p.ni;
    Tn = g.Tn;
    P = (int)g.P();
    F = (int)g.F();
    SS = s * s * (Tn > 1 ? s : 1);
    Kp = K * (K + 1) / 2;
    NV = p.views[0] * p.views[1];
    KG = K * NV;
    is4 = p.variant == CCSC_L4D;
    is3 = p.variant == CCSC_L3D;
    gp = g.gp;
    zl_on = rt.z == ZStep::Line;
    N = p.n / ni;
    nbl = rt.nb;
    b0 = rt.b0;
    np = nbl * ni;
    owner0 = (b0 == 0);
    theta = p.lambda_prior / p.theta_div;
    if (!b) throw Err(CCSC_E_INVALID, "b must not be NULL");
    if (rt.st2) {
      HIPCHK(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ev_g, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_i, hipEventDisableTiming));
    }

    const char* note = p.tol > 0 ? " (tol > 0 adds a z-sized buffer)" : "";
    alloc_plan(rows, buf, b2::count, note, [&](int i) {
      if (i == b2::Zh2 && rt.st3) {   // st3 keeps its place among the allocations
        HIPCHK(hipStreamCreateWithFlags(&st3, hipStreamNonBlocking));
        for (hipEvent_t* e : {&ev_s, &ev_z, &ev_gz[0], &ev_gz[1]})
          HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
      }
    });
    upload_twiddles(tw, make_twiddles(G));
    if (rt.z == ZStep::Planes3) upload_twiddles(twt, make_twiddles(g.Gt));
    if (rt.tsolve_tc) upload_twiddles(twt2, make_twiddles(rt.gt2));
    xf = {g, r, is3, st, &tw, &twt, &gR};
    if (gp) xf.lines.setup(g.lp, st, buf[b2::gtwr], buf[b2::gtwc], &buf[b2::gtwt]);

    // data: b (rank-local, [sbx, sby(, sbt), np] column-major) and its padded spectrum
    HIPCHK(hipMemcpy(bdev.p, b, bdev.bytes, hipMemcpyHostToDevice));
    xf.fwd_embed(bdev.re(), (int)p.sb[0], (int)p.sb[1], is3 ? (int)p.sb[2] : 1, r,
              Bhat.cx(), np * NV);
    if (zl_on)
      HIPCHK(launch_to_slots<double>(Bhat.cx(), Bhs.cx(), np, st));
    if (rt.tsolve_tc)
      HIPCHK(launch_to_ttiles<double>(Bhat.cx(), BhatT.cx(), Tn, G.Y, G.Xh, rt.tsolve_tc, np, st));
    // filters: init.d or device RNG (dP:38-39; 4D: [psf,psf,U,V,K], L4:39-40; 3D: psf^3, L3:39-40)
    DevBuf& d0dev = buf[b2::d0];
    d0dev.alloc(rows[b2::d0].bytes);
    const size_t nd0 = (size_t)SS * KG;
    if (d0) HIPCHK(hipMemcpy(d0dev.p, d0, nd0 * 8, hipMemcpyHostToDevice));
    else HIPCHK(launch_randn<double>(d0dev.re(), (int64_t)nd0, p.seed ^ 0xd0d0d0d0ULL, 0, st));
    HIPCHK(launch_embed_filters<double>(d0dev.re(), D.re(), (int)nbl, KG, s, G, Tn, st));
    HIPCHK(hipMemsetAsync(yD.p, 0, yD.bytes, st));
    HIPCHK(hipMemsetAsync(Usup.p, 0, Usup.bytes, st));  // u = Pi(0) = 0 (Q2)
    HIPCHK(hipMemsetAsync(yz.p, 0, yz.bytes, st));
    // codes: init.z or device RNG (dP:45; dZ:44-47 replicates one z0 per block)
    const size_t KP = (size_t)K * P;
    if (p.variant == CCSC_DZPAR) {
      const size_t nz0 = (size_t)ni * KP;
      if (z0) HIPCHK(hipMemcpy(z.p, z0, nz0 * 8, hipMemcpyHostToDevice));
      else HIPCHK(launch_randn<double>(z.re(), (int64_t)nz0, p.seed, 0, st));
      if (nbl > 1)
        HIPCHK(launch_replicate<double>(z.re(), z.re() + nz0, (int64_t)nz0, (int)nbl - 1, st));
    } else {
      if (z0) HIPCHK(hipMemcpy(z.p, z0, z.bytes, hipMemcpyHostToDevice));
      else
        HIPCHK(launch_randn<double>(z.re(), (int64_t)(np * KP), p.seed,
                                    (uint64_t)(b0 * ni) * KP, st));
    }
    // 3D / 4D / global-pass 2D: `yz` holds the z-step state a = z + y (kernels3d.hip,
    // zstep.hip, gslice.hip), y = 0
    if (is4 || is3 || gp) HIPCHK(hipMemcpyAsync(yz.p, z.p, z.bytes, hipMemcpyDeviceToDevice, st));
    // dhat = fft2(d) of the initial filters (all blocks share d0, dP:41-42)
    xf.fwd_embed(D.re(), G.X, G.Y, Tn, 0, dhat.cx(), KG);
    HIPCHK(hipStreamSynchronize(st));
    d0dev.release();

    if (p.verbose != CCSC_VERBOSE_NONE || p.trace_objective)
      obj_filter = obj_z = objective(dhat.cx(), nullptr);  // dP:56
    lg.start(p, obj_z);
  }

  // ---- collectives (ctx_collective) -------------------------------------------
  void allreduce(double* buf, size_t count) { ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, buf, count); }
  void bcast0(double* buf, size_t count) { ctx_collective(ctx, st, CCSC_COMM_BCAST0, buf, count); }
  // h2 = the sum over the ranks of `count` partial pairs (of `pair` as it stands when parts
  // is NULL), on the host
  void reduce_pair(const double* parts, int64_t count, double* h2) {
    if (parts) HIPCHK(launch_sum_pairs<double>(parts, (int)count, pair.re(), st));
    allreduce(pair.re(), 2);
    HIPCHK(hipMemcpyAsync(h2, pair.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  // what a z-step launch left for the tol test (register-line z-step, zline.hip):
  // `lagged` the test of the iterate it started from (zpart, one launch late: the
  // launch was speculative), `form` the test of the iterate it produced (fpart)
  struct ZTests {
    bool lagged = false, form = false;
  };
  double* zpart() { return znorm.re(); }
  double* fpart() { return znorm.re() + 2 * np; }
  // one z-iteration over the local patches (dP:147-157; 4D L4:163-167; 3D L3:164-178).
  // The other z-steps leave the test of the produced iterate in znorm when tol_on.
  bool zsplit_ok(bool tol_on) const {
    return rt.zsplit2 && zl_on && !tol_on && zmode == 2 && st3 && np >= 512;
  }
  // both halves of a split z-phase done before anything else reads the state on st
  void zsplit_join() {
    if (!zsplit_open) return;
    hipEvent_t e = pool.get(), b = pool.get();
    HIPCHK(hipEventRecord(e, st3));
    HIPCHK(hipStreamWaitEvent(st, e, 0));
    HIPCHK(hipEventRecord(b, st));
    pool.put(e);
    if (prof) {
      recs.push_back(Rec{0, zsp_a, b, zsp_n});
    } else {
      pool.put(zsp_a);
      pool.put(b);
    }
    zsplit_open = false;
  }

  // write_z: the 3D / 4D z-steps store z only for the iterations whose z is read (the last
  // of the phase -- the D-precompute's -- the objective's, the tol test's); `yz` holds
  // their state a = z + y (kernels3d.hip, zstep.hip)
  // more: another z-iteration follows directly (3D: its forward plane transform is fused
  // into this one's inverse, c_ready)
  // emit: the register-line z-step also stores the spectra of the state it writes into
  // `yz` (rt.zemit; the caller knows this is the phase's last iteration and nothing
  // materialises the state after it)
  ZTests zstep_iter(bool tol_on, bool write_z = true, bool more = false, bool emit = false) {
    const auto* twc = tw.cx();
    if (rt.z == ZStep::Diag4) {
      HIPCHK(launch_zstep_diag<double>(z.re(), yz.re(), E.cx(), sden.re(), np * K, twc, G, theta,
                                       p.rho_z, znorm.re(), tol_on, write_z || tol_on, st));
    } else if (rt.z == ZStep::Planes3) {
      cpx<double>* C = E.cx();
      const auto* twtc = twt.cx();
      // the state a = z + y lives in `yz` (modes 3, kernels3d.hip)
      if (!c_ready)
        HIPCHK(launch_plane_fwd<double>(3, z.re(), yz.re(), nullptr, 0, 0, 0, 0,
                                        theta, 1, r, C, np * K, Tn, twc, G, st, rt.tsolve_tc));
      if (rt.tsolve_tc) {
        HIPCHK(launch_tsolve3<double>(C, BhatT.cx(), dhatT.cx(), sdenT.re(), np, K, G.Y, G.Xh,
                                      rt.tsolve_tc, 1.0 / (double)P, twt2.cx(), rt.gt2, st,
                                      tsolve_ppw));
      } else {
        HIPCHK(launch_tfft<double>(C, C, np * K, G.Y, G.F, -1, twtc, g.Gt, st));
        HIPCHK(launch_zsolve3<double>(C, Bhat.cx(), dhat.cx(),
                                      sden.re(), F, np, K, 1.0 / (double)P, st));
        HIPCHK(launch_tfft<double>(C, C, np * K, G.Y, G.F, +1, twtc, g.Gt, st));
      }
      HIPCHK(launch_plane_inv<double>(3, C, z.re(), nullptr, nullptr, tol_on ? znorm.re() : nullptr,
                                      0, 1.0, r, np * K, Tn, twc, G, st, rt.tsolve_tc, yz.re(),
                                      theta, write_z || tol_on, more ? C : nullptr));
      c_ready = more;
    } else if (rt.z == ZStep::Global) {
      // global-pass 2D slices: c = a - 2 clamp(a) -> R2C -> closed-form solve per bin
      // (k_zsolve3, the 1/P folded in) -> C2R -> a' = z' + clamp(a), z' when it is read
      // (4D: the diagonal solve (E + rho c) sden against the view correlations, L4:327-347)
      cpx<double>* C = is4 ? Cg.cx() : E.cx();
      HIPCHK(launch_gp_prolog<double>(3, nullptr, yz.re(), nullptr, 0, 0, 0, theta, 1, r,
                                      gR.re(), G.X, G.Y, np * K, st, Tn));
      xf.lines.r2c(gR.re(), C, np * K);
      if (is4)
        HIPCHK(launch_gp_zdiag<double>(C, E.cx(), sden.re(), p.rho_z, (int)F, np * K, st));
      else
        HIPCHK(launch_zsolve3<double>(C, Bhat.cx(), dhat.cx(),
                                      sden.re(), F, np, K, 1.0 / (double)P, st));
      xf.lines.c2r(C, gR.re(), np * K);
      HIPCHK(launch_gp_epilog<double>(3, gR.re(), z.re(), nullptr, nullptr,
                                      tol_on ? znorm.re() : nullptr, 0, 1.0, r, G.X, G.Y,
                                      np * K, yz.re(), theta, write_z || tol_on, st, Tn));
    } else if (rt.z == ZStep::Line) {
      // register-line z-step (zline.hip): mode 0 reads (z, y) and leaves a in state order.
      // tol > 0: a launch whose starting w was solved with the current filters measures
      // the iterate it produces in place (Form); otherwise (the first z-iteration after a
      // d-phase, or a materialised state) it stores the z it starts from in `yz`, and the
      // next launch measures that iterate against it (Cmp, one launch late)
      const int mode = zmode == 2 ? 2 : 0;
      // (a mode-0 launch reads y from `yz`; with a tol test `yz` holds z_old)
      cpx<double>* Cz = (emit && rt.zemit && !tol_on && mode == 2) ? yz.cx() : nullptr;
      if (!tol_on) yzh = Cz ? YzHolds::Spectra : YzHolds::Other;
      if (zsplit_ok(tol_on)) {
        if (!zsplit_open) {
          zsp_a = pool.get();
          HIPCHK(hipEventRecord(zsp_a, st));
          HIPCHK(hipStreamWaitEvent(st3, zsp_a, 0));
          zsplit_open = true;
          zsp_n = 0;
        }
        const int64_t na = np / 2;
        const int64_t zo = na * K * (int64_t)P, wo = na * (int64_t)F;
        HIPCHK(launch_zline<double>(z.re(), z.re(), z.re(), yz.re(), W.cx(), Bhs.cx(), dws,
                                    dhs.cx(), sdens.re(), na, K, theta, p.rho_z, 2, st, 0, nullptr,
                                    nullptr, nullptr, Cz));
        HIPCHK(launch_zline<double>(z.re() + zo, z.re() + zo, z.re() + zo, yz.re() + zo,
                                    W.cx() + wo, Bhs.cx() + wo, dws, dhs.cx(), sdens.re(), np - na,
                                    K, theta, p.rho_z, 2, st3, 0, nullptr, nullptr, nullptr,
                                    Cz ? Cz + na * K * (int64_t)F : nullptr));
        ++zsp_n;
        dws = dhs.cx();
        return ZTests{};
      }
      const bool same = mode == 2 && dws == dhs.cx();
      int tolv = 0;
      if (tol_on) {
        if (!same) tolv = kZlTolStore;
        else if (yzh == YzHolds::ZPrev) tolv = kZlTolStore | kZlTolCmp | kZlTolForm;
        else tolv = kZlTolForm;
      }
      HIPCHK(launch_zline<double>(z.re(), z.re(), z.re(), yz.re(), W.cx(), Bhs.cx(),
                                  zmode == 2 ? dws : dhs.cx(), dhs.cx(), sdens.re(), np, K, theta,
                                  p.rho_z, mode, st, tolv, yz.re(), zpart(), fpart(), Cz));
      zmode = 2;
      dws = dhs.cx();
      // `yz` holds the z before the current iterate only after a lone Store launch; after a
      // Cmp launch it holds the iterate the test covered (kept for zl_rollback only)
      if (tol_on) yzh = (tolv == kZlTolStore) ? YzHolds::ZPrev : YzHolds::Other;
      ZTests r;
      r.lagged = (tolv & kZlTolCmp) != 0;
      r.form = (tolv & kZlTolForm) != 0;
      return r;
    } else if (!tol_on) {
      // one pass per patch over the pre-threshold state a (zsplit.hip): `z` holds a
      HIPCHK(launch_zsplit<double>(z.re(), z.re(), yz.re(), W.cx(), Bhat.cx(), dw, dhat.cx(),
                                   sden.re(), np, twc, G, K, theta, zmode, st));
      zmode = 1;
      dw = dhat.cx();
    } else {
      // tol test (dP:156-157): a into cbuf so z_old stays in z, then (z, y) from a
      // and ifft2(conj(d) w) with the per-slice change norms
      HIPCHK(launch_zsplit<double>(z.re(), cbuf.re(), yz.re(), W.cx(), Bhat.cx(), dw, dhat.cx(),
                                   sden.re(), np, twc, G, K, theta, zmode, st));
      HIPCHK(launch_zmat<double>(cbuf.re(), yz.re(), W.cx(), dhat.cx(), z.re(), z.re(), znorm.re(),
                                 np, twc, G, K, theta, st));
      zmode = 0;
    }
    return ZTests{};
  }
  // register-line state + tol: the test of the current iterate against the z before it
  // (in `yz`, ZPrev) without advancing (end of a z-phase)
  void zl_finalize() {
    HIPCHK(launch_zline<double>(z.re(), z.re(), z.re(), yz.re(), W.cx(), Bhs.cx(), dws, dhs.cx(),
                                sdens.re(), np, K, theta, p.rho_z, 3, st, kZlTolStore | kZlTolCmp,
                                yz.re(), zpart(), fpart()));
    yzh = YzHolds::ZCur;
  }
  // register-line state + tol: materialise (z, y) of the current iterate and measure it
  // against the z before it (`yz`, ZPrev): both slices to natural order in place, then
  // k_zmat with z_old = yz (read before it is overwritten by y)
  void zl_materialize_tol() {
    HIPCHK(launch_state_to_nat_inplace<double>(z.re(), np * K, st));
    HIPCHK(launch_state_to_nat_inplace<double>(yz.re(), np * K, st));
    HIPCHK(launch_zmat<double>(z.re(), yz.re(), W.cx(), dws, z.re(), yz.re(), znorm.re(), np,
                               tw.cx(), G, K, theta, st, true));
    zmode = 0;
    yzh = YzHolds::Other;
  }
  // register-line state + tol: the launch just made was one iteration past the break
  // (its test of the iterate it started from fired).  That iterate is intact: `yz` holds
  // its z and `z` its pre-threshold value a = z + y (the launch's state write); the
  // launch's w is dropped.  (z, y) natural <- (yz, z - yz).
  void zl_rollback() {
    HIPCHK(launch_state_to_nat_inplace<double>(z.re(), np * K, st));
    HIPCHK(launch_state_to_nat_inplace<double>(yz.re(), np * K, st));
    HIPCHK(launch_sub_inplace<double>(z.re(), yz.re(), np * K * (int64_t)P, st));
    std::swap(z.p, yz.p);   // z <- z, yz <- y
    zmode = 0;
    yzh = YzHolds::Other;
  }
  // state a -> (z, y) materialised in place (objective, outputs)
  void materialize_z() {
    if (zmode == 0) return;
    yzh = YzHolds::Other;   // `yz` receives y
    if (zmode == 2) {   // state order -> natural a in yz, then (z, y) from it
      HIPCHK(launch_state_to_nat<double>(z.re(), yz.re(), np * K, st));
      HIPCHK(launch_zmat<double>(yz.re(), yz.re(), W.cx(), dws, z.re(), nullptr, nullptr, np,
                                 tw.cx(), G, K, theta, st, true));
      zmode = 0;
      return;
    }
    HIPCHK(launch_zmat<double>(z.re(), yz.re(), W.cx(), dw, z.re(), nullptr, nullptr, np, tw.cx(),
                               G, K, theta, st));
    zmode = 0;
  }

  // 3D objective (L3:342-355), patch by patch through the z-step's spectrum buffer
  void objective3_parts(const cpx<double>* dsp, double* DZdev) {
    const auto* twc = tw.cx();
    const auto* twtc = twt.cx();
    cpx<double>* C = E.cx();
    const int sbx = (int)p.sb[0], sby = (int)p.sb[1], sbt = (int)p.sb[2];
    HIPCHK(hipMemsetAsync(pair.p, 0, 2 * sizeof(double), st));
    for (int64_t q = 0; q < np; ++q) {
      const double* zq = z.re() + (size_t)q * K * P;
      double* dzq = DZdev ? DZdev + (size_t)q * P : odz.re();
      HIPCHK(launch_plane_fwd<double>(0, zq, nullptr, nullptr, G.X, G.Y, Tn, 0, 0.0, 1, 0, C, K,
                                      Tn, twc, G, st));
      HIPCHK(launch_tfft<double>(C, C, K, G.Y, G.F, -1, twtc, g.Gt, st));
      HIPCHK(launch_corr_sum<double>(C, dsp, oacc.cx(), F, K, st));
      HIPCHK(launch_tfft<double>(oacc.cx(), oacc.cx(), 1, G.Y, G.F, +1, twtc, g.Gt, st));
      HIPCHK(launch_plane_inv<double>(0, oacc.cx(), dzq, nullptr, nullptr, nullptr, 0,
                                      1.0 / (double)P, r, 1, Tn, twc, G, st));
      HIPCHK(launch_crop_sq<double>(dzq, bdev.re() + (size_t)q * sbx * sby * sbt, sbx, sby,
                                    sbt, r, r, G.X, G.Y, zq, (int64_t)K * P, pair.re(), st));
    }
  }


  // objective with filter spectrum `dsp` (valid on every rank); DZ optional.
  // global-pass 2D objective (dP:305-324), patch by patch through the z-step's spectra
  // (4D, L4:349-369: every view of the patch from the same code spectra, DZ cropped per view)
  void objective_gp_parts(const cpx<double>* dsp, double* DZdev) {
    cpx<double>* C = is4 ? Cg.cx() : E.cx();
    const int sbx = (int)p.sb[0], sby = (int)p.sb[1];
    HIPCHK(hipMemsetAsync(pair.p, 0, 2 * sizeof(double), st));
    if (is4) {
      const size_t vb = (size_t)sbx * sby;
      for (int64_t q = 0; q < np; ++q) {
        const double* zq = z.re() + (size_t)q * K * P;
        xf.lines.r2c(zq, C, K);
        HIPCHK(launch_gp_views<double>(C, dsp, oacc.cx(), (int)F, K, NV, st));
        xf.lines.c2r(oacc.cx(), gR.re(), NV);
        HIPCHK(launch_gp_crop<double>(gR.re(), bdev.re() + (size_t)q * NV * vb,
                                      DZdev ? DZdev + (size_t)q * NV * vb : nullptr, sbx, sby, r,
                                      G.X, G.Y, 1.0 / (double)P, pair.re(), NV, st));
        // sum |z| of the patch (no crop term: sx = sy = 0)
        HIPCHK(launch_crop_sq<double>(gR.re(), bdev.re(), 0, 0, 1, r, 0, G.X, G.Y, zq,
                                      (int64_t)K * P, pair.re(), st));
      }
      return;
    }
    for (int64_t q = 0; q < np; ++q) {
      const double* zq = z.re() + (size_t)q * K * P;
      double* dzq = DZdev ? DZdev + (size_t)q * P : odz.re();
      xf.lines.r2c(zq, C, K);
      HIPCHK(launch_corr_sum<double>(C, dsp, oacc.cx(), F, K, st));
      xf.lines.c2r(oacc.cx(), gR.re(), 1);
      HIPCHK(launch_gp_epilog<double>(0, gR.re(), dzq, nullptr, nullptr, nullptr, 0,
                                      1.0 / (double)P, r, G.X, G.Y, 1, nullptr, 0.0, 0, st, Tn));
      // (3D: the crop of L3:351 in t as well)
      const int sbt = Tn > 1 ? (int)p.sb[2] : 1;
      HIPCHK(launch_crop_sq<double>(dzq, bdev.re() + (size_t)q * sbx * sby * sbt, sbx, sby, sbt, r,
                                    Tn > 1 ? r : 0, G.X, G.Y, zq, (int64_t)K * P, pair.re(), st));
    }
  }

  double objective(const cpx<double>* dsp, double* DZdev) {
    double h2[2];
    if (gp || is3) {   // the parts accumulate in `pair`
      if (gp) objective_gp_parts(dsp, DZdev);
      else objective3_parts(dsp, DZdev);
      reduce_pair(nullptr, 0, h2);
    } else {
      materialize_z();
      HIPCHK(launch_objective<double>(z.re(), dsp, bdev.re(), (int)p.sb[0], (int)p.sb[1], r, DZdev,
                                      part.re(), np, tw.cx(), G, K, NV, st));
      reduce_pair(part.re(), np * NV, h2);
    }
    return p.lambda_residual * 0.5 * h2[0] + p.lambda_prior * h2[1];
  }
  double objective_now() override { return objective(dhat.cx(), nullptr); }
  // current filter spectrum of global block 1 into dtmp on every rank
  const cpx<double>* current_dhat() {
    if (owner0)
      HIPCHK(hipMemcpyAsync(dtmp.p, Dh.p, (size_t)KG * F * 16, hipMemcpyDeviceToDevice, st));
    bcast0(dtmp.re(), (size_t)2 * KG * F);
    return dtmp.cx();
  }

  // ---- one outer iteration --------------------------------------------------
  void outer_iteration() override {
    const bool dtile = rt.dsolve == DSolve::Tile;
    hipEvent_t e0 = pool.get(), e1 = pool.get();
    double obj_ms = 0;
    auto objective_timed = [&](const cpx<double>* dsp) {
      hipEvent_t a = pool.get(), b = pool.get();
      HIPCHK(hipEventRecord(a, st));
      const double o = objective(dsp, nullptr);
      HIPCHK(hipEventRecord(b, st));
      HIPCHK(hipEventSynchronize(b));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, a, b));
      obj_ms += ms;
      pool.put(a);
      pool.put(b);
      return o;
    };
    HIPCHK(hipEventRecord(e0, st));

    // ---- D precompute (dP:95-99) ----
    // 110 grid: block j+1's R2C on st3 beside block j's Gram on st (same-box A/B at
    // 8ff8b2a: 949 vs 957.7 ms per C2 step in series, profiles/r03j/preov_ab.txt)
    // the spectra the last z-launch emitted (rt.zemit): no R2C pass and no st3 hand-off,
    // k_gram_chol_mf adds the term of w as it stages them
    const bool zem = yzh == YzHolds::Spectra && zmode == 2 && rt.zemit && rt.dfactor == DFactor::Mfma;
    const bool ovz = zmode == 2 && st3 && !zem;
    // k_gram_chol_mf leaves the inverted diagonal tiles itself (rt.dinv): no k_invert_diag
    const bool dinv = dtile && rt.dinv && rt.dfactor == DFactor::Mfma;
    const bool dgrp = zem && rt.dgroup;
    if (dgrp) {
      // every local block's spectra lie in `yz`: one launch over them (its partial last
      // round of workgroups paid once, not per block)
      timed(1, [&] {
        HIPCHK(launch_gram_chol_mf(yz.cx(), Bhs.cx(), L.cx(), h.cx(), F, K, ni, p.rho_d, NV, st,
                                   W.cx(), dws, (int)nbl, dinv));
        // (a block too large for the fused form's LDS: L is contiguous over the blocks)
        if (dtile && !dinv) HIPCHK(launch_invert_diag(L.cx(), (int)nbl * F, K, st));
      }, nbl);
    }
    if (ovz) {   // st3's R2C passes read the state the z-phase left on st
      HIPCHK(hipEventRecord(ev_s, st));
      HIPCHK(hipStreamWaitEvent(st3, ev_s, 0));
    }
    for (int64_t jl = 0; jl < (dgrp ? 0 : nbl); ++jl) {
      cpx<double>* Zc = (ovz && (jl & 1)) ? Zh2.cx() : Zh.cx();
      if (zem) {
        Zc = yz.cx() + (size_t)jl * ni * K * F;
      } else if (ovz) {   // the same on the lanes (zline.hip), on st3 (see st3)
        if (jl >= 2) HIPCHK(hipStreamWaitEvent(st3, ev_gz[jl & 1], 0));   // Gram(jl-2) read Zc
        HIPCHK(launch_zhat_line<double>(z.re() + (size_t)jl * ni * K * P,
                                        W.cx() + (size_t)jl * ni * F, dws, Zc, ni, K, theta, st3));
        HIPCHK(hipEventRecord(ev_z, st3));
        HIPCHK(hipStreamWaitEvent(st, ev_z, 0));
      } else if (zmode == 2)
        HIPCHK(launch_zhat_line<double>(z.re() + (size_t)jl * ni * K * P,
                                        W.cx() + (size_t)jl * ni * F, dws,
                                        Zh.cx(), ni, K, theta, st));
      else if (zmode)  // fft2(z) of the state a: fft2(u - y) + XY conj(dw) w, u = soft(a)
        HIPCHK(launch_zhat_split<double>(z.re() + (size_t)jl * ni * K * P,
                                         W.cx() + (size_t)jl * ni * F, zmode == 2 ? dws : dw,
                                         Zh.cx(), ni, tw.cx(), G, K, theta, st, zmode == 2));
      else
        xf.fwd_embed(z.re() + (size_t)jl * ni * K * P, G.X, G.Y, Tn, 0, Zh.cx(), (int64_t)ni * K);
      timed(1, [&] {
        const cpx<double>* Bj = Bhat.cx() + (size_t)jl * ni * NV * F;
        cpx<double>* Lj = L.cx() + (size_t)jl * F * Kp;
        cpx<double>* hj = h.cx() + (size_t)jl * F * NV * K;
        const int NVg = rt.h_sep ? 0 : NV;
        if (rt.h_sep)
          HIPCHK(launch_hs_corr<double>(Zc, Bj, hj, F, NV, K, ni, st));
        switch (rt.dfactor) {
          case DFactor::WBig:
            HIPCHK(launch_wbig_gram(Zc, Bj, Xbig.cx(), Lj, hj, F, K, ni, p.rho_d, NV, st));
            break;
          case DFactor::Wb:
            HIPCHK(launch_gram_wb<double>(Zc, Bj, Lj, hj, F, K, ni, p.rho_d, NV, rt.wb_stage, st));
            break;
          case DFactor::Big:
            HIPCHK(launch_gram_big(Zc, Bj, Xbig.cx(), Lj, hj, F, K, ni, p.rho_d, NVg, st));
            break;
          case DFactor::Mfma:
            HIPCHK(launch_gram_chol_mf(Zc, zem ? Bhs.cx() + (size_t)jl * ni * F : Bj,
                                       Lj, hj, F, K, ni, p.rho_d, NVg, st,
                                       zem ? W.cx() + (size_t)jl * ni * F : nullptr,
                                       zem ? dws : nullptr, 1, dinv));
            if (dtile && !dinv) {
              HIPCHK(hipEventRecord(ev_g, st));
              HIPCHK(hipStreamWaitEvent(st2, ev_g, 0));
              HIPCHK(launch_invert_diag(Lj, F, K, st2));
            }
            break;
          case DFactor::Valu:
            HIPCHK(launch_gram_chol<double>(Zc, Bj, Lj, hj, F, K, ni, p.rho_d, NVg, st));
            break;
        }
      });
      if (ovz) HIPCHK(hipEventRecord(ev_gz[jl & 1], st));
    }
    if (dtile && !dinv && !dgrp) {   // every block's inverted diagonal tiles before the first d-solve
      HIPCHK(hipEventRecord(ev_i, st2));
      HIPCHK(hipStreamWaitEvent(st, ev_i, 0));
    }
    // ---- D iterations (dP:103-134) ----
    const bool tol_on = p.tol > 0;
    const bool want_od = verbose_refresh() || p.trace_objective;
    int nd = 0;
    for (int id = 0; id < p.max_it_d; ++id) {
      // dual + R2C of (u - y) into Ch (dP:107-111)
      timed(3, [&] { xf.dual_r2c(D.re(), yD.re(), Usup.re(), Ch.cx(), nbl * KG, KG); });
      timed(2, [&] {
        if (rt.dfactor == DFactor::WBig)
          HIPCHK(launch_wbig_solve(L.cx(), h.cx(), Ch.cx(),
                                   Dh.cx(), (int)nbl, F, K, ni, p.rho_d, NV, st));
        else if (rt.dfactor == DFactor::Wb)
          HIPCHK(launch_dsolve_wb<double>(L.cx(), h.cx(), Ch.cx(), Dh.cx(), (int)nbl, F, K, ni,
                                          p.rho_d, NV, rt.wb_stage, st));
        else if (dtile)
          HIPCHK(launch_dsolve_tile(L.cx(), h.cx(), Ch.cx(), Dh.cx(), (int)nbl, F, K, p.rho_d, NV,
                                    st));
        else
          HIPCHK(launch_dsolve<double>(L.cx(), h.cx(), Ch.cx(), Dh.cx(), (int)nbl, F, K, p.rho_d,
                                       NV, st));
      });
      // C2R of Dh -> D, support of D + y, d-norms of block 1 (dP:112-121); Dh stays intact
      // (block 1's spectrum feeds the z-step)
      timed(4, [&] {
        xf.c2r_dout(Dh.cx(), Ch.cx(), D.re(), yD.re(), supp.re(), dnorm.re(), owner0 ? KG : 0,
                    nbl * KG);
      });
      HIPCHK(launch_supp_reduce<double>(supp.re(), ssum.re(), (int)nbl, KG * SS, st));
      allreduce(ssum.re(), (size_t)KG * SS);
      // Pi normalises per filter (2D, dP:212-213; 3D, L3:245-252) / per (u,v,k) slice
      // (4D, L4:224-225)
      HIPCHK(launch_project<double>(ssum.re(), Usup.re(), KG, SS, 1.0 / (double)N, st));
      ++nd;
      double dd = std::numeric_limits<double>::quiet_NaN();
      if (tol_on) {
        double h2[2];
        // (the plane kernels leave one pair per (slice, t); the global-pass epilogue per slice)
        if (!owner0) HIPCHK(hipMemsetAsync(pair.p, 0, 2 * sizeof(double), st));
        reduce_pair(owner0 ? dnorm.re() : nullptr, gp ? KG : KG * Tn, h2);
        dd = std::sqrt(h2[0]) / std::sqrt(h2[1]);
        last_d = dd;
        lg.tr_dd[lg.d_slot(id)] = dd;
      }
      if (want_od) {
        const double o = objective_timed(current_dhat());
        if (verbose_refresh()) obj_filter = o;
        if (p.trace_objective) lg.tr_od[lg.d_slot(id)] = o;
      }
      if (tol_on && dd < p.tol) break;  // dP:130-132
    }
    // ---- Z precompute (dP:143-144): d = Dhat of block 1 ----
    if (zmode == 1 && dw == dhat.cx()) {  // keep the spectrum w was solved with
      std::swap(dhat.p, dhatw.p);
      dw = dhatw.cx();
    }
    if (zmode == 2 && dws == dhs.cx()) {
      std::swap(dhs.p, dhws.p);
      dws = dhws.cx();
    }
    if (owner0) HIPCHK(hipMemcpyAsync(dhat.p, Dh.p, (size_t)KG * F * 16, hipMemcpyDeviceToDevice, st));
    bcast0(dhat.re(), (size_t)2 * KG * F);
    // s(f) = sum over filters (and views, L4:277,330) of |dhat|^2
    HIPCHK(launch_sden<double>(dhat.cx(), sden.re(), F, KG, p.rho_z, 1.0 / (double)P, st));
    if (zl_on) {
      HIPCHK(launch_to_slots<double>(dhat.cx(), dhs.cx(), K, st));
      HIPCHK(launch_to_slots_real<double>(sden.re(), sdens.re(), st));
    }
    if (rt.tsolve_tc) {
      HIPCHK(launch_to_ttiles<double>(dhat.cx(), dhatT.cx(), Tn, G.Y, G.Xh, rt.tsolve_tc, K, st));
      HIPCHK(launch_to_ttiles_real<double>(sden.re(), sdenT.re(), Tn, G.Y, G.Xh, rt.tsolve_tc, st));
    }
    if (is4)   // L4:327 first term, constant over the z-iterations
      HIPCHK(launch_view_corr<double>(dhat.cx(), Bhat.cx(), E.cx(), np, F, K, NV, st));
    // ---- Z iterations (dP:147-168) ----
    const bool want_oz = verbose_refresh() || p.trace_objective;
    int nz = 0;
    // z_diff of iteration iz (dP:156-157, dZ:163-164) from `count` partial pairs
    // (||z - z_old||^2, ||z||^2); the Parseval form of zline.hip may round a vanishing
    // difference to a tiny negative sum
    auto z_test = [&](int iz, const double* parts, int64_t count) {
      double h2[2];
      reduce_pair(parts, count, h2);
      const double zd = std::sqrt(std::max(h2[0], 0.0)) / std::sqrt(h2[1]);
      last_z = zd;
      lg.tr_zd[lg.z_slot(iz)] = zd;
      return zd;
    };
    // register-line z-step with tol (zline.hip): a launch measures the iterate it
    // produces (ZTests::form) once its starting w was solved with the current filters;
    // after a d-phase the first launch stores its starting z and the second measures
    // that iterate one launch late (ZTests::lagged; the second launch was speculative
    // when the test fires: zl_rollback); the objective's materialisation measures
    // without the lag (zl_materialize_tol)
    const bool zl_tol = zl_on && tol_on;
    bool zbreak = false;
    c_ready = false;
    for (int iz = 0; iz < p.max_it_z; ++iz) {
      ZTests zt_done;
      const bool wz = want_oz || iz + 1 == p.max_it_z;
      // the objective (want_oz) reuses the spectrum buffer between iterations
      const bool more = iz + 1 < p.max_it_z && !want_oz;
      // tol = 0: the phase's last iteration is known; an objective evaluation after it would
      // materialise the state over the spectra
      const bool emit = !tol_on && !want_oz && iz + 1 == p.max_it_z;
      if (zsplit_ok(tol_on))
        zt_done = zstep_iter(tol_on, wz, more, emit);   // timed as one phase record by zsplit_join
      else
        timed(0, [&] { zt_done = zstep_iter(tol_on, wz, more, emit); });
      ++nz;
      if (zt_done.lagged && z_test(iz - 1, zpart(), np) < p.tol) {   // dP:165-167 for iz - 1
        zl_rollback();
        --nz;
        zbreak = true;
        break;
      }
      double zd = std::numeric_limits<double>::quiet_NaN();
      if (zl_tol && want_oz) {
        zl_materialize_tol();
        zd = z_test(iz, znorm.re(), np * K);
      } else if (zt_done.form) {
        zd = z_test(iz, fpart(), np);
      } else if (tol_on && !zl_tol) {
        zd = z_test(iz, znorm.re(), gp ? np * K : np * K * Tn);
      }
      if (want_oz) {
        zsplit_join();
        const double o = objective_timed(dhat.cx());
        if (verbose_refresh()) obj_z = o;
        if (p.trace_objective) lg.tr_oz[lg.z_slot(iz)] = o;
      }
      if (tol_on && zd < p.tol) {  // dP:165-167
        zbreak = true;
        break;
      }
    }
    zsplit_join();
    if (zl_tol && !zbreak && yzh == YzHolds::ZPrev) {   // the last iteration's test
      zl_finalize();
      z_test(nz - 1, zpart(), np);
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    pool.put(e0);
    pool.put(e1);
    drain_records();
    const double secs = (ms - obj_ms) * 1e-3;
    lg.push(obj_filter, obj_z, secs, nd, nz, 0);  // dP:174-176
    if (tol_on && last_z < p.tol && last_d < p.tol) lg.finished = true;  // dP:186-188
  }

  void results(ccsc_outputs* out) override {
    if (!out) return;
    if (out->d_res) {
      // D1 lives on rank 0 (block 1); broadcast so every rank returns it.
      std::vector<double> D1((size_t)KG * P);
      DevBuf tmp;
      tmp.alloc((size_t)KG * P * 8);
      if (owner0) HIPCHK(hipMemcpyAsync(tmp.p, D.p, tmp.bytes, hipMemcpyDeviceToDevice, st));
      bcast0(tmp.re(), (size_t)KG * P);
      HIPCHK(hipMemcpyAsync(D1.data(), tmp.p, tmp.bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      crop_filters(D1, out->d_res, KG, s, r, G, Tn, P);
    }
    if (out->z_res) {
      materialize_z();
      HIPCHK(hipStreamSynchronize(st));   // st is non-blocking: hipMemcpy does not order after it
      HIPCHK(hipMemcpy(out->z_res, z.p, z.bytes, hipMemcpyDeviceToHost));
    }
    if (out->DZ) {
      // DZ = real(ifft2(sum_k zhat .* dup{1}))  (dP:193), uncropped [X,Y,1,n]
      DevBuf dz;
      dz.alloc(is4 ? (size_t)np * NV * p.sb[0] * p.sb[1] * 8 : (size_t)np * P * 8);
      objective(dhat.cx(), dz.re());
      HIPCHK(hipMemcpy(out->DZ, dz.p, dz.bytes, hipMemcpyDeviceToHost));
    }
    if (out->obj_val) *out->obj_val = objective(dhat.cx(), nullptr);
  }

  // The codes as results() would copy them into z_res: the natural-order `z`, one column
  // of M = X Y (T) K values per local patch.  Leaves the session as that copy leaves it.
  const double* codes_dense(int64_t* M, int64_t* n) override {
    materialize_z();
    HIPCHK(hipStreamSynchronize(st));
    *n = np;
    *M = (int64_t)(z.bytes / sizeof(double)) / np;
    return z.re();
  }

  double alg_bytes(int id) const {
    const double Pd = P, Fd = F, Kd = K;
    switch (id) {
      case 0:  // z-iteration, SURVEY.md §8(d): n K (4 s P + 4 c F) + n c F V  (s = 8, c = 16):
               // prox+dual+R2C, solve, C2R stages each reading/writing their operands once
        return (double)np * Kd * (4.0 * 8.0 * Pd + 4.0 * 16.0 * Fd) + (double)np * NV * 16.0 * Fd;
      case 1:  // gram+chol per block: read A (ni x K x F) + b, write L, h; a launch covers
               // one block or, grouped (rt.dgroup), the rank's: the mean over the launches timed
        return ((double)ni * Kd * Fd * 16.0 + ni * Fd * 16.0 + Fd * Kp * 16.0 + Fd * Kd * 16.0) *
               (k_launch[1] ? (double)k_blocks1 / (double)k_launch[1] : 1.0);
      case 2:  // dsolve over local blocks: read L, h, C; write Dhat
        return (double)nbl * Fd * (Kp + 3.0 * Kd) * 16.0;
      case 3:  // dual+R2C: read D, y; write y, C
        return (double)nbl * Kd * (3.0 * 8.0 * Pd + 16.0 * Fd);
      case 4:  // C2R + support: read Dhat, write D
        return (double)nbl * Kd * (16.0 * Fd + 8.0 * Pd);
    }
    return 0;
  }
  void set_profiling(bool on) override { prof = on; }
  void kernel_stats(int id, int64_t* launches, double* total_ms, double* bytes) const override {
    *launches = k_launch[id];
    *total_ms = k_ms[id];
    *bytes = alg_bytes(id);
  }
};

}  // namespace

std::unique_ptr<Session> make_session2d(ccsc_ctx* ctx, const ccsc_problem& p, const double* b,
                                        const double* d0, const double* z0) {
  return std::unique_ptr<Session>(new Session2D(ctx, p, b, d0, z0));
}

}  // namespace ccsc
