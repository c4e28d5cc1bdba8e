// libccsc host engine: the sessions (device buffers from the memory plan of plan.hpp, the
// outer ADMM schedule on the route it resolved), RCCL consensus, and the C-ABI.
//
// Schedule of one outer iteration (dP:89-190; dZ:90-194), per rank:
//   precompute  for each local block: R2C of its z slices -> Zh;
//               gram+cholesky -> L_f, h_f                       (dP:95-99)
//   d-loop      dual+R2C -> C ; dsolve -> Dhat ; C2R -> D, support(D+y)
//               -> local sum -> RCCL all-reduce -> projection u (dP:103-134)
//   z-prep      dhat = Dhat of global block 1 (RCCL broadcast), sden  (dP:143)
//   z-loop      fused z-iteration kernel over the local patches   (dP:147-168)
#include "../../include/ccsc.h"
#include "host.hpp"
#include "recon.hpp"
#include "slice.hpp"

#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <string>
#include <vector>

using namespace ccsc;

namespace ccsc {

// Host iteration log of a session (ccsc_iterlog).  Per outer iteration: the objectives after
// the d- and z-phase, cumulative seconds, inner iteration counts, flags; entry 0 of the
// first three is the initial state.  Per inner iteration: the objective and relative-change
// traces, NaN where they were not evaluated.
struct HostLog {
  int max_it_d = 0, max_it_z = 0;
  int outer_done = 0;
  bool finished = false;
  std::vector<double> v_obj_d, v_obj_z, v_tim, tr_od, tr_oz, tr_dd, tr_zd;
  std::vector<int32_t> v_nd, v_nz, v_flags;

  void start(const ccsc_problem& p, double obj0) {
    max_it_d = p.max_it_d;
    max_it_z = p.max_it_z;
    v_obj_d.push_back(obj0);
    v_obj_z.push_back(obj0);
    v_tim.push_back(0.0);
  }
  void ensure_trace_capacity(int total_outer) {
    const size_t nd = (size_t)total_outer * max_it_d, nz = (size_t)total_outer * max_it_z;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (tr_od.size() < nd) tr_od.resize(nd, nan);
    if (tr_dd.size() < nd) tr_dd.resize(nd, nan);
    if (tr_oz.size() < nz) tr_oz.resize(nz, nan);
    if (tr_zd.size() < nz) tr_zd.resize(nz, nan);
  }
  // slot of inner iteration t of the current outer iteration in a d- / z-trace
  size_t d_slot(int t) const { return (size_t)outer_done * max_it_d + t; }
  size_t z_slot(int t) const { return (size_t)outer_done * max_it_z + t; }
  void push(double obj_d, double obj_z, double secs, int nd, int nz, int flags) {
    v_obj_d.push_back(obj_d);
    v_obj_z.push_back(obj_z);
    v_tim.push_back(v_tim.back() + secs);
    v_nd.push_back(nd);
    v_nz.push_back(nz);
    v_flags.push_back(flags);
    ++outer_done;
  }
  void write(ccsc_iterlog* lg) const {
    if (!lg) return;
    const int cnt = std::min<int>(lg->capacity, (int)v_tim.size());
    lg->count = cnt;
    for (int i = 0; i < cnt; ++i) {
      if (lg->obj_vals_d) lg->obj_vals_d[i] = v_obj_d[i];
      if (lg->obj_vals_z) lg->obj_vals_z[i] = v_obj_z[i];
      if (lg->tim_vals) lg->tim_vals[i] = v_tim[i];
    }
    const int no = std::min<int>(lg->capacity, outer_done);
    for (int i = 0; i < no; ++i) {
      if (lg->n_d) lg->n_d[i] = v_nd[i];
      if (lg->n_z) lg->n_z[i] = v_nz[i];
      if (lg->flags) lg->flags[i] = v_flags[i];
      for (int t = 0; t < max_it_d; ++t) {
        const size_t q = (size_t)i * max_it_d + t;
        if (lg->trace_obj_d) lg->trace_obj_d[q] = q < tr_od.size() ? tr_od[q] : NAN;
        if (lg->trace_d_diff) lg->trace_d_diff[q] = q < tr_dd.size() ? tr_dd[q] : NAN;
      }
      for (int t = 0; t < max_it_z; ++t) {
        const size_t q = (size_t)i * max_it_z + t;
        if (lg->trace_obj_z) lg->trace_obj_z[q] = q < tr_oz.size() ? tr_oz[q] : NAN;
        if (lg->trace_z_diff) lg->trace_z_diff[q] = q < tr_zd.size() ? tr_zd[q] : NAN;
      }
    }
  }
};

// up to n_outer outer iterations of a session: `pre` (the outer index) before each, `cb` after
template <typename S>
static void run_outer(S& s, int n_outer, ccsc_cb cb, void* user,
                      const std::function<void(int)>& pre = nullptr) {
  HostLog& lg = s.lg;
  lg.ensure_trace_capacity(lg.outer_done + n_outer);
  for (int i = 0; i < n_outer && !lg.finished; ++i) {
    if (pre) pre(lg.outer_done);
    s.outer_iteration();
    if (cb) cb(user, lg.outer_done, lg.v_obj_d.back(), lg.v_obj_z.back(), lg.v_tim.back());
  }
}

static const char* kKernelNames[5] = {"zstep", "gram_chol", "dsolve", "dual_r2c", "c2r_dout"};

// Wait for a non-blocking communicator's pending call (ncclInProgress); with `abort`,
// give up as soon as the group aborted (the enqueue may be waiting on a failed rank).
static void wait_comm(ncclComm_t c, const std::atomic<bool>* abort) {
  ncclResult_t st = ncclInProgress;
  for (;;) {
    NCCLCHK(ncclCommGetAsyncError(c, &st));
    if (st != ncclInProgress) break;
    if (abort && abort->load())
      throw Err(CCSC_E_RCCL, "host communicator aborted: another rank of this context failed");
    std::this_thread::yield();
  }
  if (st != ncclSuccess)
    throw Err(CCSC_E_RCCL, std::string("RCCL communicator error: ") + ncclGetErrorString(st));
}

// The communicators of a device-list context (rank i on devices[i]), created
// non-blocking so that no collective call can stall inside RCCL: abort_group relies on
// it to abort them only while no rank is inside a call.
static void init_group_comms(std::vector<ncclComm_t>& comms, const int32_t* devices, int nd) {
  // NCCL_COMM_BLOCKING=1 overrides cfg.blocking = 0 per communicator: a surviving rank could
  // then block inside a collective waiting on a failed one and abort_group would wait on it
  // forever -- refuse it instead of deadlocking later
  if (const char* b = std::getenv("NCCL_COMM_BLOCKING"))
    if (std::atoi(b) != 0)
      throw Err(CCSC_E_INVALID,
                "NCCL_COMM_BLOCKING=1 is not supported for multi-device contexts: their RCCL "
                "communicators must be non-blocking so a failed rank can be aborted");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
  cfg.blocking = 0;
  auto ok = [](ncclResult_t r) { return r == ncclSuccess || r == ncclInProgress; };
  if (!ok(ncclGroupStart())) throw Err(CCSC_E_RCCL, "ncclGroupStart failed");
  for (int i = 0; i < nd; ++i) {
    HIPCHK(hipSetDevice(devices[i]));
    const ncclResult_t r = ncclCommInitRankConfig(&comms[i], nd, id, i, &cfg);
    if (!ok(r)) {
      ncclGroupEnd();
      throw Err(CCSC_E_RCCL, std::string("ncclCommInitRankConfig failed: ") + ncclGetErrorString(r));
    }
  }
  const ncclResult_t r = ncclGroupEnd();
  if (!ok(r)) throw Err(CCSC_E_RCCL, std::string("ncclGroupEnd failed: ") + ncclGetErrorString(r));
  for (int i = 0; i < nd; ++i) wait_comm(comms[i], nullptr);
}

// ---------------------------------------------------------------------------
// Session: 2D consensus learners (dP / dZ)
// ---------------------------------------------------------------------------
// ---- collectives of a rank context ------------------------------------------
// The transport is chosen by what the context was created with (a host callback or
// an RCCL communicator), never by a communicator pointer an abort may have cleared;
// in a multi-device group every collective first checks that no rank has failed.
static void host_exchange(ccsc_ctx* ctx, hipStream_t st, int op, double* buf, size_t count) {
  ctx->stage.resize(count);
  HIPCHK(hipMemcpyAsync(ctx->stage.data(), buf, count * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ctx->hostfn(ctx->hostuser, op, ctx->stage.data(), (int64_t)count) != 0)
    throw Err(CCSC_E_RCCL, "host communicator callback failed");
  HIPCHK(hipMemcpyAsync(buf, ctx->stage.data(), count * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
}
static void ctx_collective(ccsc_ctx* ctx, hipStream_t st, int op, double* buf, size_t count) {
  if (ctx->nranks <= 1 && !ctx->rccl_self) return;
  if (ctx->hostfn) {   // the exchange itself returns an error once the group aborted
    host_exchange(ctx, st, op, buf, count);
    return;
  }
  CommGroup* g = ctx->grp.get();
  if (g) g->inflight.fetch_add(1);
  struct Leave {
    CommGroup* g;
    ~Leave() {
      if (g) g->inflight.fetch_sub(1);
    }
  } leave{g};
  if (g && g->aborted.load())
    throw Err(CCSC_E_RCCL, "host communicator aborted: another rank of this context failed");
  if (!ctx->comm) throw Err(CCSC_E_STATE, "multi-rank context without a communicator");
  const ncclResult_t r = op == CCSC_COMM_ALLREDUCE_SUM
                             ? ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, ctx->comm, st)
                             : ncclBroadcast(buf, buf, count, ncclDouble, 0, ctx->comm, st);
  // a device-list group's communicators are non-blocking (init_group_comms): the enqueue
  // may still be connecting; wait for it here, giving up once the group aborted, so no
  // rank stays inside RCCL on a communicator abort_group is about to abort
  if (r == ncclInProgress) wait_comm(ctx->comm, g ? &g->aborted : nullptr);
  else if (r != ncclSuccess)
    throw Err(CCSC_E_RCCL, std::string("RCCL collective failed: ") + ncclGetErrorString(r));
}

// Session of every consensus learner: dP, dZ, the 4D light-field learner (2D
// spatial convolution, NV = U*V views share the codes, L4:18-21) and the 3D
// learner (Tn > 1: plane transforms + t-direction FFT, L3).
struct Session2D {
  ccsc_ctx* ctx;
  ccsc_problem p;
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
  hipStream_t st;

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
  // tol > 0 with the register-line z-step: what `yz` holds (state order) while the
  // state is in zmode 2 -- ZT_PREV: the z of the iterate before the current one
  // (the next launch measures the current iterate against it), ZT_CUR: the
  // current iterate's z (its test is done), ZT_NONE: nothing (y, or stale).
  enum { ZT_NONE, ZT_PREV, ZT_CUR };
  int zt = ZT_NONE;
  // rt.zemit (tol = 0): `yz` holds the code spectra of the current state, [np][K][F] in
  // bin-slot order as the phase's last z-launch emitted them (twice fft2(u - y), without
  // the term of w).  Set by that launch alone; cleared by every other z-launch and by
  // whatever writes `yz` (materialize_z).  The D-precompute reads them when it is set.
  bool cz_valid = false;
  // 3D: t-FFT twiddles, objective scratch (also the global path's)
  DevBuf &twt = buf[b2::twt], &oacc = buf[b2::oacc], &odz = buf[b2::odz];
  // 2D slices past one CU's LDS (Geom::gp): global line passes (recon.hip), and the real
  // scratch the elementwise stages (gslice.hip) read and write
  bool gp = false;
  LinePass lines;
  DevBuf &gR = buf[b2::gR], &Cg = buf[b2::Cg];
  // 3D with k_tsolve3 (rt.tsolve_tc, its t plan rt.gt2): the plan's twiddles; B^, the filter
  // spectrum and sden in its tile order
  DevBuf &twt2 = buf[b2::twt2];
  DevBuf &BhatT = buf[b2::BhatT], &dhatT = buf[b2::dhatT], &sdenT = buf[b2::sdenT];
  int tsolve_ppw = 16;          // patches per k_tsolve3 workgroup
  bool c_ready = false;         // 3D: the z-step spectrum C already holds the next forward

  HostLog lg;
  double last_d = std::numeric_limits<double>::infinity();
  double last_z = std::numeric_limits<double>::infinity();
  double obj_filter = std::numeric_limits<double>::quiet_NaN();
  double obj_z = std::numeric_limits<double>::quiet_NaN();

  // profiling
  bool prof = false;
  struct Rec { int id; hipEvent_t a, b; int n = 1; int64_t blocks = 1; };   // n launches between a and b
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  int64_t k_launch[5] = {0, 0, 0, 0, 0};
  double k_ms[5] = {0, 0, 0, 0, 0};
  // blocks the launches of id 1 covered (one per block launch, nbl per grouped launch)
  int64_t k_blocks1 = 0;

  hipEvent_t get_event() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    return e;
  }
  template <typename Fn>
  void timed(int id, Fn&& fn, int64_t blocks = 1) {
    if (!prof) {
      fn();
      return;
    }
    Rec rc{id, get_event(), get_event(), 1, blocks};
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
      pool.push_back(rc.a);
      pool.push_back(rc.b);
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
    for (auto e : pool) hipEventDestroy(e);
  }

  // the objective is refreshed after every d- / z-iteration (the reference's verbose rules
  // are the same for both phases)
  bool verbose_refresh() const { return objective_refresh(p); }   // (plan.cpp: the route reads it too)

  Session2D(ccsc_ctx* c, const ccsc_problem& pin, const double* b, const double* d0,
            const double* z0)
      : ctx(c), p(pin), st(c->stream) {
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

    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    if (plan_total(rows) > freeb)
      throw Err(CCSC_E_NOMEM, "device plan needs " + std::to_string(plan_total(rows) >> 20) +
                                  " MiB, " + std::to_string(freeb >> 20) + " MiB free" +
                                  (p.tol > 0 ? " (tol > 0 adds a z-sized buffer)" : ""));
    for (int i = 0; i < b2::count; ++i) {
      if (rows[i].scope == 0) buf[i].alloc(rows[i].bytes);
      if (i == b2::Zh2 && rt.st3) {   // st3 keeps its place among the allocations
        HIPCHK(hipStreamCreateWithFlags(&st3, hipStreamNonBlocking));
        for (hipEvent_t* e : {&ev_s, &ev_z, &ev_gz[0], &ev_gz[1]})
          HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
      }
    }
    upload_twiddles(tw, make_twiddles(G));
    if (rt.z == ZStep::Planes3) upload_twiddles(twt, make_twiddles(g.Gt));
    if (rt.tsolve_tc) upload_twiddles(twt2, make_twiddles(rt.gt2));
    if (gp) lines.setup(g.lp, st, buf[b2::gtwr], buf[b2::gtwc], &buf[b2::gtwt]);

    // data: b (rank-local, [sbx, sby(, sbt), np] column-major) and its padded spectrum
    HIPCHK(hipMemcpy(bdev.p, b, bdev.bytes, hipMemcpyHostToDevice));
    fwd_embed(bdev.as<double>(), (int)p.sb[0], (int)p.sb[1], is3 ? (int)p.sb[2] : 1, r,
              Bhat.as<cpx<double>>(), np * NV);
    if (zl_on)
      HIPCHK(launch_to_slots<double>(Bhat.as<cpx<double>>(), Bhs.as<cpx<double>>(), np, st));
    if (rt.tsolve_tc)
      HIPCHK(launch_to_ttiles<double>(Bhat.as<cpx<double>>(), BhatT.as<cpx<double>>(), Tn, G.Y,
                                      G.Xh, rt.tsolve_tc, np, st));
    // filters: init.d or device RNG (dP:38-39; 4D: [psf,psf,U,V,K], L4:39-40; 3D: psf^3, L3:39-40)
    DevBuf& d0dev = buf[b2::d0];
    d0dev.alloc(rows[b2::d0].bytes);
    const size_t nd0 = (size_t)SS * KG;
    if (d0) HIPCHK(hipMemcpy(d0dev.p, d0, nd0 * 8, hipMemcpyHostToDevice));
    else HIPCHK(launch_randn<double>(d0dev.as<double>(), (int64_t)nd0, p.seed ^ 0xd0d0d0d0ULL, 0, st));
    HIPCHK(launch_embed_filters<double>(d0dev.as<double>(), D.as<double>(), (int)nbl, KG, s, G, Tn,
                                        st));
    HIPCHK(hipMemsetAsync(yD.p, 0, yD.bytes, st));
    HIPCHK(hipMemsetAsync(Usup.p, 0, Usup.bytes, st));  // u = Pi(0) = 0 (Q2)
    HIPCHK(hipMemsetAsync(yz.p, 0, yz.bytes, st));
    // codes: init.z or device RNG (dP:45; dZ:44-47 replicates one z0 per block)
    const size_t KP = (size_t)K * P;
    if (p.variant == CCSC_DZPAR) {
      const size_t nz0 = (size_t)ni * KP;
      if (z0) HIPCHK(hipMemcpy(z.p, z0, nz0 * 8, hipMemcpyHostToDevice));
      else HIPCHK(launch_randn<double>(z.as<double>(), (int64_t)nz0, p.seed, 0, st));
      if (nbl > 1)
        HIPCHK(launch_replicate<double>(z.as<double>(), z.as<double>() + nz0, (int64_t)nz0,
                                        (int)nbl - 1, st));
    } else {
      if (z0) HIPCHK(hipMemcpy(z.p, z0, z.bytes, hipMemcpyHostToDevice));
      else
        HIPCHK(launch_randn<double>(z.as<double>(), (int64_t)(np * KP), p.seed,
                                    (uint64_t)(b0 * ni) * KP, st));
    }
    // 3D / 4D / global-pass 2D: `yz` holds the z-step state a = z + y (kernels3d.hip,
    // zstep.hip, gslice.hip), y = 0
    if (is4 || is3 || gp) HIPCHK(hipMemcpyAsync(yz.p, z.p, z.bytes, hipMemcpyDeviceToDevice, st));
    // dhat = fft2(d) of the initial filters (all blocks share d0, dP:41-42)
    fwd_embed(D.as<double>(), G.X, G.Y, Tn, 0, dhat.as<cpx<double>>(), KG);
    HIPCHK(hipStreamSynchronize(st));
    d0dev.release();

    if (p.verbose != CCSC_VERBOSE_NONE || p.trace_objective)
      obj_filter = obj_z = objective(dhat.as<cpx<double>>(), nullptr);  // dP:56
    lg.start(p, obj_z);
  }

  // ---- collectives (ctx_collective) -------------------------------------------
  void allreduce(double* buf, size_t count) { ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, buf, count); }
  void bcast0(double* buf, size_t count) { ctx_collective(ctx, st, CCSC_COMM_BCAST0, buf, count); }
  void pair_to_host(double* out2) {
    HIPCHK(hipMemcpyAsync(out2, pair.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  // ---- transforms ------------------------------------------------------------
  // dst[count][F] = R2C of the zero-padded [sx, sy, st] sub-volumes of src placed at
  // offset o in every dimension (o = r: padarray of b, dP:23 / L3:23; o = 0: full grid)
  void fwd_embed(const double* src, int sx, int sy, int stt, int o, cpx<double>* dst,
                 int64_t count) {
    const auto* twc = tw.as<cpx<double>>();
    if (gp) {
      if (sx == G.X && sy == G.Y && stt == Tn && o == 0) {
        lines.r2c(src, dst, count);
        return;
      }
      HIPCHK(launch_gp_prolog<double>(0, src, nullptr, nullptr, sx, sy, o, 0.0, 1, r,
                                      gR.as<double>(), G.X, G.Y, count, st, Tn, stt,
                                      Tn > 1 ? o : 0));
      lines.r2c(gR.as<double>(), dst, count);
      return;
    }
    if (!is3) {
      HIPCHK(launch_r2c_embed<double>(src, (int64_t)sx * sy, sx, sy, o, o, dst, F, count, twc, G,
                                      st));
      return;
    }
    HIPCHK(launch_plane_fwd<double>(0, src, nullptr, nullptr, sx, sy, stt, o, 0.0, 1, 0, dst,
                                    count, Tn, twc, G, st));
    HIPCHK(launch_tfft<double>(dst, dst, count, G.Y, G.F, -1, twt.as<cpx<double>>(), g.Gt, st));
  }
  // D-step dual + R2C of (u - y) into Ch (dP:107-111)
  void dual_fwd() {
    const auto* twc = tw.as<cpx<double>>();
    if (gp) {
      HIPCHK(launch_gp_prolog<double>(2, D.as<double>(), yD.as<double>(), Usup.as<double>(), 0, 0,
                                      0, 0.0, KG, r, gR.as<double>(), G.X, G.Y, nbl * KG, st, Tn));
      lines.r2c(gR.as<double>(), Ch.as<cpx<double>>(), nbl * KG);
      return;
    }
    if (!is3) {
      HIPCHK(launch_dual_r2c<double>(D.as<double>(), yD.as<double>(), Usup.as<double>(),
                                     Ch.as<cpx<double>>(), nbl * KG, twc, G, KG, r, st));
      return;
    }
    HIPCHK(launch_plane_fwd<double>(2, D.as<double>(), yD.as<double>(), Usup.as<double>(), 0, 0, 0,
                                    0, 0.0, KG, r, Ch.as<cpx<double>>(), nbl * KG, Tn, twc, G, st));
    HIPCHK(launch_tfft<double>(Ch.as<cpx<double>>(), Ch.as<cpx<double>>(), nbl * KG, G.Y, G.F, -1,
                               twt.as<cpx<double>>(), g.Gt, st));
  }
  // C2R of Dh -> D, support of D + y, d-norms of block 1 (dP:112-121)
  void inv_dout() {
    const auto* twc = tw.as<cpx<double>>();
    if (gp) {   // Dh stays intact (block 1's spectrum feeds the z-step): the inverse runs on Ch
      HIPCHK(hipMemcpyAsync(Ch.p, Dh.p, (size_t)nbl * KG * F * 16, hipMemcpyDeviceToDevice, st));
      lines.c2r(Ch.as<cpx<double>>(), gR.as<double>(), nbl * KG);
      HIPCHK(launch_gp_epilog<double>(2, gR.as<double>(), D.as<double>(), yD.as<double>(),
                                      supp.as<double>(), dnorm.as<double>(), owner0 ? KG : 0,
                                      1.0 / (double)P, r, G.X, G.Y, nbl * KG, nullptr, 0.0, 0, st, Tn));
      return;
    }
    if (!is3) {
      HIPCHK(launch_c2r_dout<double>(Dh.as<cpx<double>>(), D.as<double>(), yD.as<double>(),
                                     supp.as<double>(), dnorm.as<double>(), owner0 ? KG : 0,
                                     nbl * KG, twc, G, r, st));
      return;
    }
    // Dh stays intact (block 1's spectrum feeds the z-step): t-inverse into Ch
    HIPCHK(launch_tfft<double>(Dh.as<cpx<double>>(), Ch.as<cpx<double>>(), nbl * KG, G.Y, G.F, +1,
                               twt.as<cpx<double>>(), g.Gt, st));
    HIPCHK(launch_plane_inv<double>(2, Ch.as<cpx<double>>(), D.as<double>(), yD.as<double>(),
                                    supp.as<double>(), dnorm.as<double>(), owner0 ? KG : 0,
                                    1.0 / (double)P, r, nbl * KG, Tn, twc, G, st));
  }
  // what a z-step launch left for the tol test (register-line z-step, zline.hip):
  // `lagged` the test of the iterate it started from (zpart, one launch late: the
  // launch was speculative), `form` the test of the iterate it produced (fpart)
  struct ZTests {
    bool lagged = false, form = false;
  };
  double* zpart() { return znorm.as<double>(); }
  double* fpart() { return znorm.as<double>() + 2 * np; }
  // one z-iteration over the local patches (dP:147-157; 4D L4:163-167; 3D L3:164-178).
  // The other z-steps leave the test of the produced iterate in znorm when tol_on.
  bool zsplit_ok(bool tol_on) const {
    return rt.zsplit2 && zl_on && !tol_on && zmode == 2 && st3 && np >= 512;
  }
  // both halves of a split z-phase done before anything else reads the state on st
  void zsplit_join() {
    if (!zsplit_open) return;
    hipEvent_t e = get_event(), b = get_event();
    HIPCHK(hipEventRecord(e, st3));
    HIPCHK(hipStreamWaitEvent(st, e, 0));
    HIPCHK(hipEventRecord(b, st));
    pool.push_back(e);
    if (prof) {
      recs.push_back(Rec{0, zsp_a, b, zsp_n});
    } else {
      pool.push_back(zsp_a);
      pool.push_back(b);
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
    const auto* twc = tw.as<cpx<double>>();
    if (rt.z == ZStep::Diag4) {
      HIPCHK(launch_zstep_diag<double>(z.as<double>(), yz.as<double>(), E.as<cpx<double>>(),
                                       sden.as<double>(), np * K, twc, G, theta, p.rho_z,
                                       znorm.as<double>(), tol_on, write_z || tol_on, st));
    } else if (rt.z == ZStep::Planes3) {
      cpx<double>* C = E.as<cpx<double>>();
      const auto* twtc = twt.as<cpx<double>>();
      // the state a = z + y lives in `yz` (modes 3, kernels3d.hip)
      if (!c_ready)
        HIPCHK(launch_plane_fwd<double>(3, z.as<double>(), yz.as<double>(), nullptr, 0, 0, 0, 0,
                                        theta, 1, r, C, np * K, Tn, twc, G, st, rt.tsolve_tc));
      if (rt.tsolve_tc) {
        HIPCHK(launch_tsolve3<double>(C, BhatT.as<cpx<double>>(), dhatT.as<cpx<double>>(),
                                      sdenT.as<double>(), np, K, G.Y, G.Xh, rt.tsolve_tc,
                                      1.0 / (double)P, twt2.as<cpx<double>>(), rt.gt2, st,
                                      tsolve_ppw));
      } else {
        HIPCHK(launch_tfft<double>(C, C, np * K, G.Y, G.F, -1, twtc, g.Gt, st));
        HIPCHK(launch_zsolve3<double>(C, Bhat.as<cpx<double>>(), dhat.as<cpx<double>>(),
                                      sden.as<double>(), F, np, K, 1.0 / (double)P, st));
        HIPCHK(launch_tfft<double>(C, C, np * K, G.Y, G.F, +1, twtc, g.Gt, st));
      }
      HIPCHK(launch_plane_inv<double>(3, C, z.as<double>(), nullptr, nullptr,
                                      tol_on ? znorm.as<double>() : nullptr, 0, 1.0, r, np * K,
                                      Tn, twc, G, st, rt.tsolve_tc, yz.as<double>(), theta,
                                      write_z || tol_on, more ? C : nullptr));
      c_ready = more;
    } else if (rt.z == ZStep::Global) {
      // global-pass 2D slices: c = a - 2 clamp(a) -> R2C -> closed-form solve per bin
      // (k_zsolve3, the 1/P folded in) -> C2R -> a' = z' + clamp(a), z' when it is read
      // (4D: the diagonal solve (E + rho c) sden against the view correlations, L4:327-347)
      cpx<double>* C = is4 ? Cg.as<cpx<double>>() : E.as<cpx<double>>();
      HIPCHK(launch_gp_prolog<double>(3, nullptr, yz.as<double>(), nullptr, 0, 0, 0, theta, 1, r,
                                      gR.as<double>(), G.X, G.Y, np * K, st, Tn));
      lines.r2c(gR.as<double>(), C, np * K);
      if (is4)
        HIPCHK(launch_gp_zdiag<double>(C, E.as<cpx<double>>(), sden.as<double>(), p.rho_z, (int)F,
                                       np * K, st));
      else
        HIPCHK(launch_zsolve3<double>(C, Bhat.as<cpx<double>>(), dhat.as<cpx<double>>(),
                                      sden.as<double>(), F, np, K, 1.0 / (double)P, st));
      lines.c2r(C, gR.as<double>(), np * K);
      HIPCHK(launch_gp_epilog<double>(3, gR.as<double>(), z.as<double>(), nullptr, nullptr,
                                      tol_on ? znorm.as<double>() : nullptr, 0, 1.0, r, G.X, G.Y,
                                      np * K, yz.as<double>(), theta, write_z || tol_on, st, Tn));
    } else if (rt.z == ZStep::Line) {
      // register-line z-step (zline.hip): mode 0 reads (z, y) and leaves a in state order.
      // tol > 0: a launch whose starting w was solved with the current filters measures
      // the iterate it produces in place (Form); otherwise (the first z-iteration after a
      // d-phase, or a materialised state) it stores the z it starts from in `yz`, and the
      // next launch measures that iterate against it (Cmp, one launch late)
      const int mode = zmode == 2 ? 2 : 0;
      // (a mode-0 launch reads y from `yz`; with a tol test `yz` holds z_old)
      cpx<double>* Cz = (emit && rt.zemit && !tol_on && mode == 2) ? yz.as<cpx<double>>() : nullptr;
      cz_valid = Cz != nullptr;
      if (zsplit_ok(tol_on)) {
        if (!zsplit_open) {
          zsp_a = get_event();
          HIPCHK(hipEventRecord(zsp_a, st));
          HIPCHK(hipStreamWaitEvent(st3, zsp_a, 0));
          zsplit_open = true;
          zsp_n = 0;
        }
        const int64_t na = np / 2;
        const int64_t zo = na * K * (int64_t)P, wo = na * (int64_t)F;
        HIPCHK(launch_zline<double>(z.as<double>(), z.as<double>(), z.as<double>(), yz.as<double>(),
                                    W.as<cpx<double>>(), Bhs.as<cpx<double>>(), dws,
                                    dhs.as<cpx<double>>(), sdens.as<double>(), na, K, theta,
                                    p.rho_z, 2, st, 0, nullptr, nullptr, nullptr, Cz));
        HIPCHK(launch_zline<double>(z.as<double>() + zo, z.as<double>() + zo, z.as<double>() + zo,
                                    yz.as<double>() + zo, W.as<cpx<double>>() + wo,
                                    Bhs.as<cpx<double>>() + wo, dws, dhs.as<cpx<double>>(),
                                    sdens.as<double>(), np - na, K, theta, p.rho_z, 2, st3, 0,
                                    nullptr, nullptr, nullptr, Cz ? Cz + na * K * (int64_t)F : nullptr));
        ++zsp_n;
        dws = dhs.as<cpx<double>>();
        return ZTests{};
      }
      const bool same = mode == 2 && dws == dhs.as<cpx<double>>();
      int tolv = 0;
      if (tol_on) {
        if (!same) tolv = kZlTolStore;
        else if (zt == ZT_PREV) tolv = kZlTolStore | kZlTolCmp | kZlTolForm;
        else tolv = kZlTolForm;
      }
      HIPCHK(launch_zline<double>(z.as<double>(), z.as<double>(), z.as<double>(), yz.as<double>(),
                                  W.as<cpx<double>>(), Bhs.as<cpx<double>>(),
                                  zmode == 2 ? dws : dhs.as<cpx<double>>(), dhs.as<cpx<double>>(),
                                  sdens.as<double>(), np, K, theta, p.rho_z, mode, st, tolv,
                                  yz.as<double>(), zpart(), fpart(), Cz));
      zmode = 2;
      dws = dhs.as<cpx<double>>();
      // `yz` holds the z before the current iterate only after a lone Store launch; after a
      // Cmp launch it holds the iterate the test covered (kept for zl_rollback only)
      if (tol_on) zt = (tolv == kZlTolStore) ? ZT_PREV : ZT_NONE;
      ZTests r;
      r.lagged = (tolv & kZlTolCmp) != 0;
      r.form = (tolv & kZlTolForm) != 0;
      return r;
    } else if (!tol_on) {
      // one pass per patch over the pre-threshold state a (zsplit.hip): `z` holds a
      HIPCHK(launch_zsplit<double>(z.as<double>(), z.as<double>(), yz.as<double>(),
                                   W.as<cpx<double>>(), Bhat.as<cpx<double>>(), dw,
                                   dhat.as<cpx<double>>(), sden.as<double>(), np, twc, G, K,
                                   theta, zmode, st));
      zmode = 1;
      dw = dhat.as<cpx<double>>();
    } else {
      // tol test (dP:156-157): a into cbuf so z_old stays in z, then (z, y) from a
      // and ifft2(conj(d) w) with the per-slice change norms
      HIPCHK(launch_zsplit<double>(z.as<double>(), cbuf.as<double>(), yz.as<double>(),
                                   W.as<cpx<double>>(), Bhat.as<cpx<double>>(), dw,
                                   dhat.as<cpx<double>>(), sden.as<double>(), np, twc, G, K,
                                   theta, zmode, st));
      HIPCHK(launch_zmat<double>(cbuf.as<double>(), yz.as<double>(), W.as<cpx<double>>(),
                                 dhat.as<cpx<double>>(), z.as<double>(), z.as<double>(),
                                 znorm.as<double>(), np, twc, G, K, theta, st));
      zmode = 0;
    }
    return ZTests{};
  }
  // register-line state + tol: the test of the current iterate against the z before it
  // (in `yz`, ZT_PREV) without advancing (end of a z-phase)
  void zl_finalize() {
    HIPCHK(launch_zline<double>(z.as<double>(), z.as<double>(), z.as<double>(), yz.as<double>(),
                                W.as<cpx<double>>(), Bhs.as<cpx<double>>(), dws,
                                dhs.as<cpx<double>>(), sdens.as<double>(), np, K, theta, p.rho_z,
                                3, st, kZlTolStore | kZlTolCmp, yz.as<double>(), zpart(),
                                fpart()));
    zt = ZT_CUR;
  }
  // register-line state + tol: materialise (z, y) of the current iterate and measure it
  // against the z before it (`yz`, ZT_PREV): both slices to natural order in place, then
  // k_zmat with z_old = yz (read before it is overwritten by y)
  void zl_materialize_tol() {
    cz_valid = false;
    HIPCHK(launch_state_to_nat_inplace<double>(z.as<double>(), np * K, st));
    HIPCHK(launch_state_to_nat_inplace<double>(yz.as<double>(), np * K, st));
    HIPCHK(launch_zmat<double>(z.as<double>(), yz.as<double>(), W.as<cpx<double>>(), dws,
                               z.as<double>(), yz.as<double>(), znorm.as<double>(), np,
                               tw.as<cpx<double>>(), G, K, theta, st, true));
    zmode = 0;
    zt = ZT_NONE;
  }
  // register-line state + tol: the launch just made was one iteration past the break
  // (its test of the iterate it started from fired).  That iterate is intact: `yz` holds
  // its z and `z` its pre-threshold value a = z + y (the launch's state write); the
  // launch's w is dropped.  (z, y) natural <- (yz, z - yz).
  void zl_rollback() {
    cz_valid = false;
    HIPCHK(launch_state_to_nat_inplace<double>(z.as<double>(), np * K, st));
    HIPCHK(launch_state_to_nat_inplace<double>(yz.as<double>(), np * K, st));
    HIPCHK(launch_sub_inplace<double>(z.as<double>(), yz.as<double>(), np * K * (int64_t)P, st));
    std::swap(z.p, yz.p);   // z <- z, yz <- y
    zmode = 0;
    zt = ZT_NONE;
  }
  // state a -> (z, y) materialised in place (objective, outputs)
  void materialize_z() {
    if (zmode == 0) return;
    zt = ZT_NONE;   // `yz` receives y
    cz_valid = false;
    if (zmode == 2) {   // state order -> natural a in yz, then (z, y) from it
      HIPCHK(launch_state_to_nat<double>(z.as<double>(), yz.as<double>(), np * K, st));
      HIPCHK(launch_zmat<double>(yz.as<double>(), yz.as<double>(), W.as<cpx<double>>(), dws,
                                 z.as<double>(), nullptr, nullptr, np, tw.as<cpx<double>>(), G, K,
                                 theta, st, true));
      zmode = 0;
      return;
    }
    HIPCHK(launch_zmat<double>(z.as<double>(), yz.as<double>(), W.as<cpx<double>>(), dw,
                               z.as<double>(), nullptr, nullptr, np, tw.as<cpx<double>>(), G, K,
                               theta, st));
    zmode = 0;
  }

  // 3D objective (L3:342-355), patch by patch through the z-step's spectrum buffer
  void objective3_parts(const cpx<double>* dsp, double* DZdev) {
    const auto* twc = tw.as<cpx<double>>();
    const auto* twtc = twt.as<cpx<double>>();
    cpx<double>* C = E.as<cpx<double>>();
    const int sbx = (int)p.sb[0], sby = (int)p.sb[1], sbt = (int)p.sb[2];
    HIPCHK(hipMemsetAsync(pair.p, 0, 2 * sizeof(double), st));
    for (int64_t q = 0; q < np; ++q) {
      const double* zq = z.as<double>() + (size_t)q * K * P;
      double* dzq = DZdev ? DZdev + (size_t)q * P : odz.as<double>();
      HIPCHK(launch_plane_fwd<double>(0, zq, nullptr, nullptr, G.X, G.Y, Tn, 0, 0.0, 1, 0, C, K,
                                      Tn, twc, G, st));
      HIPCHK(launch_tfft<double>(C, C, K, G.Y, G.F, -1, twtc, g.Gt, st));
      HIPCHK(launch_corr_sum<double>(C, dsp, oacc.as<cpx<double>>(), F, K, st));
      HIPCHK(launch_tfft<double>(oacc.as<cpx<double>>(), oacc.as<cpx<double>>(), 1, G.Y, G.F, +1,
                                 twtc, g.Gt, st));
      HIPCHK(launch_plane_inv<double>(0, oacc.as<cpx<double>>(), dzq, nullptr, nullptr, nullptr, 0,
                                      1.0 / (double)P, r, 1, Tn, twc, G, st));
      HIPCHK(launch_crop_sq<double>(dzq, bdev.as<double>() + (size_t)q * sbx * sby * sbt, sbx, sby,
                                    sbt, r, r, G.X, G.Y, zq, (int64_t)K * P, pair.as<double>(), st));
    }
  }


  // objective with filter spectrum `dsp` (valid on every rank); DZ optional.
  // global-pass 2D objective (dP:305-324), patch by patch through the z-step's spectra
  // (4D, L4:349-369: every view of the patch from the same code spectra, DZ cropped per view)
  void objective_gp_parts(const cpx<double>* dsp, double* DZdev) {
    cpx<double>* C = is4 ? Cg.as<cpx<double>>() : E.as<cpx<double>>();
    const int sbx = (int)p.sb[0], sby = (int)p.sb[1];
    HIPCHK(hipMemsetAsync(pair.p, 0, 2 * sizeof(double), st));
    if (is4) {
      const size_t vb = (size_t)sbx * sby;
      for (int64_t q = 0; q < np; ++q) {
        const double* zq = z.as<double>() + (size_t)q * K * P;
        lines.r2c(zq, C, K);
        HIPCHK(launch_gp_views<double>(C, dsp, oacc.as<cpx<double>>(), (int)F, K, NV, st));
        lines.c2r(oacc.as<cpx<double>>(), gR.as<double>(), NV);
        HIPCHK(launch_gp_crop<double>(gR.as<double>(), bdev.as<double>() + (size_t)q * NV * vb,
                                      DZdev ? DZdev + (size_t)q * NV * vb : nullptr, sbx, sby, r,
                                      G.X, G.Y, 1.0 / (double)P, pair.as<double>(), NV, st));
        // sum |z| of the patch (no crop term: sx = sy = 0)
        HIPCHK(launch_crop_sq<double>(gR.as<double>(), bdev.as<double>(), 0, 0, 1, r, 0, G.X, G.Y, zq,
                                      (int64_t)K * P, pair.as<double>(), st));
      }
      return;
    }
    for (int64_t q = 0; q < np; ++q) {
      const double* zq = z.as<double>() + (size_t)q * K * P;
      double* dzq = DZdev ? DZdev + (size_t)q * P : odz.as<double>();
      lines.r2c(zq, C, K);
      HIPCHK(launch_corr_sum<double>(C, dsp, oacc.as<cpx<double>>(), F, K, st));
      lines.c2r(oacc.as<cpx<double>>(), gR.as<double>(), 1);
      HIPCHK(launch_gp_epilog<double>(0, gR.as<double>(), dzq, nullptr, nullptr, nullptr, 0,
                                      1.0 / (double)P, r, G.X, G.Y, 1, nullptr, 0.0, 0, st, Tn));
      // (3D: the crop of L3:351 in t as well)
      const int sbt = Tn > 1 ? (int)p.sb[2] : 1;
      HIPCHK(launch_crop_sq<double>(dzq, bdev.as<double>() + (size_t)q * sbx * sby * sbt, sbx, sby,
                                    sbt, r, Tn > 1 ? r : 0, G.X, G.Y, zq, (int64_t)K * P,
                                    pair.as<double>(), st));
    }
  }

  double objective(const cpx<double>* dsp, double* DZdev) {
    if (is3 || gp) {
      if (gp) objective_gp_parts(dsp, DZdev);
      else objective3_parts(dsp, DZdev);
      allreduce(pair.as<double>(), 2);
      double h2[2];
      pair_to_host(h2);
      return p.lambda_residual * 0.5 * h2[0] + p.lambda_prior * h2[1];
    }
    materialize_z();
    HIPCHK(launch_objective<double>(z.as<double>(), dsp, bdev.as<double>(), (int)p.sb[0],
                                    (int)p.sb[1], r, DZdev, part.as<double>(), np,
                                    tw.as<cpx<double>>(), G, K, NV, st));
    HIPCHK(launch_sum_pairs<double>(part.as<double>(), (int)(np * NV), pair.as<double>(), st));
    allreduce(pair.as<double>(), 2);
    double h2[2];
    pair_to_host(h2);
    return p.lambda_residual * 0.5 * h2[0] + p.lambda_prior * h2[1];
  }
  // current filter spectrum of global block 1 into dtmp on every rank
  const cpx<double>* current_dhat() {
    if (owner0)
      HIPCHK(hipMemcpyAsync(dtmp.p, Dh.p, (size_t)KG * F * 16, hipMemcpyDeviceToDevice, st));
    bcast0(dtmp.as<double>(), (size_t)2 * KG * F);
    return dtmp.as<cpx<double>>();
  }

  // ---- one outer iteration --------------------------------------------------
  void outer_iteration() {
    const bool dtile = rt.dsolve == DSolve::Tile;
    hipEvent_t e0 = get_event(), e1 = get_event();
    double obj_ms = 0;
    auto objective_timed = [&](const cpx<double>* dsp) {
      hipEvent_t a = get_event(), b = get_event();
      HIPCHK(hipEventRecord(a, st));
      const double o = objective(dsp, nullptr);
      HIPCHK(hipEventRecord(b, st));
      HIPCHK(hipEventSynchronize(b));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, a, b));
      obj_ms += ms;
      pool.push_back(a);
      pool.push_back(b);
      return o;
    };
    HIPCHK(hipEventRecord(e0, st));

    // ---- D precompute (dP:95-99) ----
    // 110 grid: block j+1's R2C on st3 beside block j's Gram on st (same-box A/B at
    // 8ff8b2a: 949 vs 957.7 ms per C2 step in series, profiles/r03j/preov_ab.txt)
    // the spectra the last z-launch emitted (rt.zemit): no R2C pass and no st3 hand-off,
    // k_gram_chol_mf adds the term of w as it stages them
    const bool zem = cz_valid && zmode == 2 && rt.zemit && rt.dfactor == DFactor::Mfma;
    const bool ovz = zmode == 2 && st3 && !zem;
    // k_gram_chol_mf leaves the inverted diagonal tiles itself (rt.dinv): no k_invert_diag
    const bool dinv = dtile && rt.dinv && rt.dfactor == DFactor::Mfma;
    const bool dgrp = zem && rt.dgroup;
    if (dgrp) {
      // every local block's spectra lie in `yz`: one launch over them (its partial last
      // round of workgroups paid once, not per block)
      timed(1, [&] {
        HIPCHK(launch_gram_chol_mf(yz.as<cpx<double>>(), Bhs.as<cpx<double>>(),
                                   L.as<cpx<double>>(), h.as<cpx<double>>(), F, K, ni, p.rho_d,
                                   NV, st, W.as<cpx<double>>(), dws, (int)nbl, dinv));
        // (a block too large for the fused form's LDS: L is contiguous over the blocks)
        if (dtile && !dinv) HIPCHK(launch_invert_diag(L.as<cpx<double>>(), (int)nbl * F, K, st));
      }, nbl);
    }
    if (ovz) {   // st3's R2C passes read the state the z-phase left on st
      HIPCHK(hipEventRecord(ev_s, st));
      HIPCHK(hipStreamWaitEvent(st3, ev_s, 0));
    }
    for (int64_t jl = 0; jl < (dgrp ? 0 : nbl); ++jl) {
      cpx<double>* Zc = (ovz && (jl & 1)) ? Zh2.as<cpx<double>>() : Zh.as<cpx<double>>();
      if (zem) {
        Zc = yz.as<cpx<double>>() + (size_t)jl * ni * K * F;
      } else if (ovz) {   // the same on the lanes (zline.hip), on st3 (see st3)
        if (jl >= 2) HIPCHK(hipStreamWaitEvent(st3, ev_gz[jl & 1], 0));   // Gram(jl-2) read Zc
        HIPCHK(launch_zhat_line<double>(z.as<double>() + (size_t)jl * ni * K * P,
                                        W.as<cpx<double>>() + (size_t)jl * ni * F, dws, Zc, ni,
                                        K, theta, st3));
        HIPCHK(hipEventRecord(ev_z, st3));
        HIPCHK(hipStreamWaitEvent(st, ev_z, 0));
      } else if (zmode == 2)
        HIPCHK(launch_zhat_line<double>(z.as<double>() + (size_t)jl * ni * K * P,
                                        W.as<cpx<double>>() + (size_t)jl * ni * F, dws,
                                        Zh.as<cpx<double>>(), ni, K, theta, st));
      else if (zmode)  // fft2(z) of the state a: fft2(u - y) + XY conj(dw) w, u = soft(a)
        HIPCHK(launch_zhat_split<double>(z.as<double>() + (size_t)jl * ni * K * P,
                                         W.as<cpx<double>>() + (size_t)jl * ni * F,
                                         zmode == 2 ? dws : dw, Zh.as<cpx<double>>(), ni,
                                         tw.as<cpx<double>>(), G, K, theta, st, zmode == 2));
      else
        fwd_embed(z.as<double>() + (size_t)jl * ni * K * P, G.X, G.Y, Tn, 0,
                  Zh.as<cpx<double>>(), (int64_t)ni * K);
      timed(1, [&] {
        const cpx<double>* Bj = Bhat.as<cpx<double>>() + (size_t)jl * ni * NV * F;
        cpx<double>* Lj = L.as<cpx<double>>() + (size_t)jl * F * Kp;
        cpx<double>* hj = h.as<cpx<double>>() + (size_t)jl * F * NV * K;
        const int NVg = rt.h_sep ? 0 : NV;
        if (rt.h_sep)
          HIPCHK(launch_hs_corr<double>(Zc, Bj, hj, F, NV, K, ni, st));
        switch (rt.dfactor) {
          case DFactor::WBig:
            HIPCHK(launch_wbig_gram(Zc, Bj, Xbig.as<cpx<double>>(), Lj, hj, F, K, ni, p.rho_d, NV, st));
            break;
          case DFactor::Wb:
            HIPCHK(launch_gram_wb<double>(Zc, Bj, Lj, hj, F, K, ni, p.rho_d, NV, rt.wb_stage, st));
            break;
          case DFactor::Big:
            HIPCHK(launch_gram_big(Zc, Bj, Xbig.as<cpx<double>>(), Lj, hj, F, K, ni, p.rho_d, NVg, st));
            break;
          case DFactor::Mfma:
            HIPCHK(launch_gram_chol_mf(Zc, zem ? Bhs.as<cpx<double>>() + (size_t)jl * ni * F : Bj,
                                       Lj, hj, F, K, ni, p.rho_d, NVg, st,
                                       zem ? W.as<cpx<double>>() + (size_t)jl * ni * F : nullptr,
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
      timed(3, [&] { dual_fwd(); });
      timed(2, [&] {
        if (rt.dfactor == DFactor::WBig)
          HIPCHK(launch_wbig_solve(L.as<cpx<double>>(), h.as<cpx<double>>(), Ch.as<cpx<double>>(),
                                   Dh.as<cpx<double>>(), (int)nbl, F, K, ni, p.rho_d, NV, st));
        else if (rt.dfactor == DFactor::Wb)
          HIPCHK(launch_dsolve_wb<double>(L.as<cpx<double>>(), h.as<cpx<double>>(),
                                          Ch.as<cpx<double>>(), Dh.as<cpx<double>>(), (int)nbl, F,
                                          K, ni, p.rho_d, NV, rt.wb_stage, st));
        else if (dtile)
          HIPCHK(launch_dsolve_tile(L.as<cpx<double>>(), h.as<cpx<double>>(),
                                    Ch.as<cpx<double>>(), Dh.as<cpx<double>>(), (int)nbl, F, K,
                                    p.rho_d, NV, st));
        else
          HIPCHK(launch_dsolve<double>(L.as<cpx<double>>(), h.as<cpx<double>>(),
                                       Ch.as<cpx<double>>(), Dh.as<cpx<double>>(), (int)nbl, F, K,
                                       p.rho_d, NV, st));
      });
      timed(4, [&] { inv_dout(); });
      HIPCHK(launch_supp_reduce<double>(supp.as<double>(), ssum.as<double>(), (int)nbl, KG * SS,
                                        st));
      allreduce(ssum.as<double>(), (size_t)KG * SS);
      // Pi normalises per filter (2D, dP:212-213; 3D, L3:245-252) / per (u,v,k) slice
      // (4D, L4:224-225)
      HIPCHK(launch_project<double>(ssum.as<double>(), Usup.as<double>(), KG, SS,
                                    1.0 / (double)N, st));
      ++nd;
      double dd = std::numeric_limits<double>::quiet_NaN();
      if (tol_on) {
        if (owner0)
          // (the plane kernels leave one pair per (slice, t); the global-pass epilogue per slice)
          HIPCHK(launch_sum_pairs<double>(dnorm.as<double>(), gp ? KG : KG * Tn, pair.as<double>(), st));
        else HIPCHK(hipMemsetAsync(pair.p, 0, 2 * sizeof(double), st));
        allreduce(pair.as<double>(), 2);
        double h2[2];
        pair_to_host(h2);
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
    if (zmode == 1 && dw == dhat.as<cpx<double>>()) {  // keep the spectrum w was solved with
      std::swap(dhat.p, dhatw.p);
      dw = dhatw.as<cpx<double>>();
    }
    if (zmode == 2 && dws == dhs.as<cpx<double>>()) {
      std::swap(dhs.p, dhws.p);
      dws = dhws.as<cpx<double>>();
    }
    if (owner0) HIPCHK(hipMemcpyAsync(dhat.p, Dh.p, (size_t)KG * F * 16, hipMemcpyDeviceToDevice, st));
    bcast0(dhat.as<double>(), (size_t)2 * KG * F);
    // s(f) = sum over filters (and views, L4:277,330) of |dhat|^2
    HIPCHK(launch_sden<double>(dhat.as<cpx<double>>(), sden.as<double>(), F, KG, p.rho_z,
                               1.0 / (double)P, st));
    if (zl_on) {
      HIPCHK(launch_to_slots<double>(dhat.as<cpx<double>>(), dhs.as<cpx<double>>(), K, st));
      HIPCHK(launch_to_slots_real<double>(sden.as<double>(), sdens.as<double>(), st));
    }
    if (rt.tsolve_tc) {
      HIPCHK(launch_to_ttiles<double>(dhat.as<cpx<double>>(), dhatT.as<cpx<double>>(), Tn, G.Y,
                                      G.Xh, rt.tsolve_tc, K, st));
      HIPCHK(launch_to_ttiles_real<double>(sden.as<double>(), sdenT.as<double>(), Tn, G.Y, G.Xh,
                                           rt.tsolve_tc, st));
    }
    if (is4)   // L4:327 first term, constant over the z-iterations
      HIPCHK(launch_view_corr<double>(dhat.as<cpx<double>>(), Bhat.as<cpx<double>>(),
                                      E.as<cpx<double>>(), np, F, K, NV, st));
    // ---- Z iterations (dP:147-168) ----
    const bool want_oz = verbose_refresh() || p.trace_objective;
    int nz = 0;
    // z_diff of iteration iz (dP:156-157, dZ:163-164) from `count` partial pairs
    // (||z - z_old||^2, ||z||^2); the Parseval form of zline.hip may round a vanishing
    // difference to a tiny negative sum
    auto z_test = [&](int iz, const double* parts, int64_t count) {
      HIPCHK(launch_sum_pairs<double>(parts, (int)count, pair.as<double>(), st));
      allreduce(pair.as<double>(), 2);
      double h2[2];
      pair_to_host(h2);
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
        zd = z_test(iz, znorm.as<double>(), np * K);
      } else if (zt_done.form) {
        zd = z_test(iz, fpart(), np);
      } else if (tol_on && !zl_tol) {
        zd = z_test(iz, znorm.as<double>(), gp ? np * K : np * K * Tn);
      }
      if (want_oz) {
        zsplit_join();
        const double o = objective_timed(dhat.as<cpx<double>>());
        if (verbose_refresh()) obj_z = o;
        if (p.trace_objective) lg.tr_oz[lg.z_slot(iz)] = o;
      }
      if (tol_on && zd < p.tol) {  // dP:165-167
        zbreak = true;
        break;
      }
    }
    zsplit_join();
    if (zl_tol && !zbreak && zt == ZT_PREV) {   // the last iteration's test
      zl_finalize();
      z_test(nz - 1, zpart(), np);
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    pool.push_back(e0);
    pool.push_back(e1);
    drain_records();
    const double secs = (ms - obj_ms) * 1e-3;
    lg.push(obj_filter, obj_z, secs, nd, nz, 0);  // dP:174-176
    if (tol_on && last_z < p.tol && last_d < p.tol) lg.finished = true;  // dP:186-188
  }

  void results(ccsc_outputs* out) {
    if (!out) return;
    if (out->d_res) {
      // D1 lives on rank 0 (block 1); broadcast so every rank returns it.
      std::vector<double> D1((size_t)KG * P);
      DevBuf tmp;
      tmp.alloc((size_t)KG * P * 8);
      if (owner0) HIPCHK(hipMemcpyAsync(tmp.p, D.p, tmp.bytes, hipMemcpyDeviceToDevice, st));
      bcast0(tmp.as<double>(), (size_t)KG * P);
      HIPCHK(hipMemcpyAsync(D1.data(), tmp.p, tmp.bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      // d_res = circshift(D1, +r)(1:psf, 1:psf(, 1:psf), :)  (dP:195-196; 4D L4:208-209:
      // per view; 3D L3:226-227)
      const int st3 = Tn > 1 ? s : 1;
      for (int k = 0; k < KG; ++k)
        for (int l = 0; l < st3; ++l)
          for (int j = 0; j < s; ++j)
            for (int i = 0; i < s; ++i) {
              const int x = (i - r + G.X) % G.X, y = (j - r + G.Y) % G.Y;
              const int t = Tn > 1 ? (l - r + Tn) % Tn : 0;
              out->d_res[i + (size_t)s * (j + (size_t)s * (l + (size_t)st3 * k))] =
                  D1[(size_t)k * P + ((size_t)t * G.Y + y) * G.X + x];
            }
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
      objective(dhat.as<cpx<double>>(), dz.as<double>());
      HIPCHK(hipMemcpy(out->DZ, dz.p, dz.bytes, hipMemcpyDeviceToHost));
    }
    if (out->obj_val) *out->obj_val = objective(dhat.as<cpx<double>>(), nullptr);
  }

  // The codes as results() would copy them into z_res: the natural-order `z`, one column
  // of M = X Y (T) K values per local patch.  Leaves the session as that copy leaves it.
  const double* codes_dense(int64_t* M, int64_t* n) {
    materialize_z();
    HIPCHK(hipStreamSynchronize(st));
    *n = np;
    *M = (int64_t)(z.bytes / sizeof(double)) / np;
    return z.as<double>();
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
};

// ---------------------------------------------------------------------------
// Session: 2-3D hyperspectral learner (L23 = 2-3D/DictionaryLearning/admm_learn.m)
// ---------------------------------------------------------------------------
// One non-consensus ADMM over all n images (one block).  Its d-solve sums over every image
// per frequency.  Several ranks (one process per GPU, images sharded in contiguous runs,
// shard()): each rank forms the Gram of its images (gramchol_big.hip, rho on rank 0 only) and
// the right-hand sides Z^H xi1 of its images, both are summed over the ranks (allreduce), and
// every rank factors and solves the same system; the objective's sums, the z change norms
// and max(b) (L23:36) are reduced too.  (Device state: mem_plan_hs, plan.cpp.)
struct SessionHS {
  ccsc_ctx* ctx;
  ccsc_problem p;
  Geom g;
  Grid2D G;
  Route rt;
  std::vector<BufRow> rows;   // the memory plan: buf[i] is allocated from rows[i]
  int r, s, SS, K, W, KG, P, F, sbx, sby;
  int n;
  hipStream_t st;
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
  LinePass lines;
  DevBuf& gR = buf[bh::gR];

  bool dist = false;   // rt.dist
  int64_t i0 = 0;      // first image of this rank
  double obj = std::numeric_limits<double>::quiet_NaN();
  double obj_filter = obj, obj_z = obj;
  HostLog lg;

  SessionHS(ccsc_ctx* c, const ccsc_problem& pin, const double* b, const double* smooth_init,
            const double* d0, const double* z0)
      : ctx(c), p(pin), st(c->stream) {
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

    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    if (plan_total(rows) > freeb)
      throw Err(CCSC_E_NOMEM, "device plan needs " + std::to_string(plan_total(rows) >> 20) +
                                  " MiB, " + std::to_string(freeb >> 20) + " MiB free");
    for (int i = 0; i < bh::count; ++i)
      if (rows[i].scope == 0) buf[i].alloc(rows[i].bytes);
    auto staging = [&](int i) -> DevBuf& {
      buf[i].alloc(rows[i].bytes);
      return buf[i];
    };
    upload_twiddles(tw, make_twiddles(G));
    if (gp) lines.setup(g.lp, st, buf[bh::gtwr], buf[bh::gtwc]);

    // data: b and smoothinit = padarray(smooth_init, [r r 0 0], 'symmetric') (L23:19)
    HIPCHK(hipMemcpy(bdev.p, b, bdev.bytes, hipMemcpyHostToDevice));
    {
      DevBuf& stage = staging(bh::stage);
      HIPCHK(hipMemcpy(stage.p, smooth_init, stage.bytes, hipMemcpyHostToDevice));
      HIPCHK(launch_pad_symmetric<double>(stage.as<double>(), smp.as<double>(), sbx, sby, r, G.X,
                                          G.Y, (int64_t)W * n, st));
      HIPCHK(hipStreamSynchronize(st));
      stage.release();
    }
    // gammas (L23:35-38): gamma_heuristic = 60 lambda / max(b(:))
    HIPCHK(launch_max<double>(bdev.as<double>(), (int64_t)((size_t)sbx * sby * W * n),
                              part.as<double>(), pair.as<double>(), st));
    double bmax = 0;
    HIPCHK(hipMemcpyAsync(&bmax, pair.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (dist) {   // max over the ranks through the sum collective: one slot per rank
      std::vector<double> mx((size_t)ctx->nranks, 0.0);
      mx[(size_t)ctx->rank] = bmax;
      DevBuf& rm = staging(bh::rm);
      HIPCHK(hipMemcpy(rm.p, mx.data(), rm.bytes, hipMemcpyHostToDevice));
      ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, rm.as<double>(), mx.size());
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
      else HIPCHK(launch_randn<double>(d0dev.as<double>(), (int64_t)SS * K, p.seed ^ 0xd0d0d0d0ULL, 0, st));
      HIPCHK(launch_rep_filters<double>(d0dev.as<double>(), d0w.as<double>(), SS, W, K, st));
      HIPCHK(launch_embed_filters<double>(d0w.as<double>(), D.as<double>(), 1, KG, s, G, 1, st));
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
      HIPCHK(launch_randn<double>(z.as<double>(), (int64_t)(z.bytes / 8), p.seed,
                                  (uint64_t)i0 * (uint64_t)K * (uint64_t)P, st));
    // d_hat = fft2(d) (L23:57); u_D{2} of the first d-iteration = Pi(d - 0) (L23:113)
    r2c_full(D.as<double>(), Dh.as<cpx<double>>(), KG);
    HIPCHK(launch_gather_support<double>(D.as<double>(), yD.as<double>(), supp.as<double>(), KG, r,
                                         G.X, G.Y, st));
    HIPCHK(launch_project<double>(supp.as<double>(), Usup.as<double>(), KG, SS, 1.0, st));
    obj = objective_fresh();                              // L23:72
    obj_filter = obj_z = obj;                             // L23:82-83
    lg.start(p, obj);
  }

  // ---- slice transforms: the fused LDS slice kernels, or on global-pass slices the line
  // passes of recon.hip around gslice.hip's elementwise halves.  On global passes the
  // inverse consumes its input spectrum (the column pass runs in place): Xi and Zh are dead
  // after their C2R here; Dh is copied to Ch (free between its d-solve and the next dual).
  // fft2 of whole real slices (L23:57,100,158,234)
  void r2c_full(const double* src, cpx<double>* dst, int64_t count) {
    if (gp) lines.r2c(src, dst, count);
    else
      HIPCHK(launch_r2c_embed<double>(src, P, G.X, G.Y, 0, 0, dst, F, count, tw.as<cpx<double>>(),
                                      G, st));
  }
  // v = real(ifft2(Xi)), DZ (nullable), the objective's data parts (k_hs_c2r_v)
  void c2r_v(double* DZ) {
    const int64_t cnt = (int64_t)W * n;
    if (!gp) {
      HIPCHK(launch_hs_c2r_v<double>(Xi.as<cpx<double>>(), v.as<double>(), bdev.as<double>(),
                                     smp.as<double>(), DZ, part.as<double>(), cnt,
                                     tw.as<cpx<double>>(), G, r, sbx, sby, st));
      return;
    }
    lines.c2r(Xi.as<cpx<double>>(), gR.as<double>(), cnt);
    HIPCHK(launch_gp_hs_epilog<double>(kHsV, gR.as<double>(), v.as<double>(), bdev.as<double>(),
                                       smp.as<double>(), DZ, part.as<double>(), G.X, G.Y, r, sbx,
                                       sby, 1.0 / (double)P, cnt, st));
  }
  // masked-data split with dual e, into Xi (k_hs_data_r2c)
  void data_r2c(DevBuf& e, double theta) {
    const int64_t cnt = (int64_t)W * n;
    if (!gp) {
      HIPCHK(launch_hs_data_r2c<double>(v.as<double>(), e.as<double>(), bdev.as<double>(),
                                        smp.as<double>(), Xi.as<cpx<double>>(), cnt,
                                        tw.as<cpx<double>>(), G, r, sbx, sby, theta, st));
      return;
    }
    HIPCHK(launch_gp_hs_prolog<double>(kHsData, v.as<double>(), e.as<double>(), bdev.as<double>(),
                                       smp.as<double>(), gR.as<double>(), G.X, G.Y, r, sbx, sby,
                                       theta, cnt, st));
    lines.r2c(gR.as<double>(), Xi.as<cpx<double>>(), cnt);
  }
  // kernel-constraint split of the D-phase, into Ch (k_dual_r2c)
  void dual_r2c() {
    if (!gp) {
      HIPCHK(launch_dual_r2c<double>(D.as<double>(), yD.as<double>(), Usup.as<double>(),
                                     Ch.as<cpx<double>>(), KG, tw.as<cpx<double>>(), G, KG, r, st));
      return;
    }
    HIPCHK(launch_gp_prolog<double>(2, D.as<double>(), yD.as<double>(), Usup.as<double>(), 0, 0, 0,
                                    0.0, KG, r, gR.as<double>(), G.X, G.Y, KG, st));
    lines.r2c(gR.as<double>(), Ch.as<cpx<double>>(), KG);
  }
  // d = real(ifft2(d_hat)), the support of d + y (k_c2r_dout); Dh stays intact
  void c2r_dout() {
    if (!gp) {
      HIPCHK(launch_c2r_dout<double>(Dh.as<cpx<double>>(), D.as<double>(), yD.as<double>(),
                                     supp.as<double>(), dnorm.as<double>(), 0, KG,
                                     tw.as<cpx<double>>(), G, r, st));
      return;
    }
    HIPCHK(hipMemcpyAsync(Ch.p, Dh.p, Dh.bytes, hipMemcpyDeviceToDevice, st));
    lines.c2r(Ch.as<cpx<double>>(), gR.as<double>(), KG);
    HIPCHK(launch_gp_epilog<double>(2, gR.as<double>(), D.as<double>(), yD.as<double>(),
                                    supp.as<double>(), dnorm.as<double>(), 0, 1.0 / (double)P, r,
                                    G.X, G.Y, KG, nullptr, 0.0, 0, st));
  }
  // sparsity split of the Z-phase with dual eZ2, into Zh (k_hs_z_r2c)
  void z_r2c() {
    const int64_t cnt = (int64_t)K * n;
    if (!gp) {
      HIPCHK(launch_hs_z_r2c<double>(z.as<double>(), eZ2.as<double>(), Zh.as<cpx<double>>(), cnt,
                                     tw.as<cpx<double>>(), G, th_Z2, st));
      return;
    }
    HIPCHK(launch_gp_hs_prolog<double>(kHsSparse, z.as<double>(), eZ2.as<double>(),
                                       bdev.as<double>(), smp.as<double>(), gR.as<double>(), G.X,
                                       G.Y, r, sbx, sby, th_Z2, cnt, st));
    lines.r2c(gR.as<double>(), Zh.as<cpx<double>>(), cnt);
  }
  // z = real(ifft2(zhat)), sum |z| per slice (k_hs_c2r_z)
  void c2r_z() {
    const int64_t cnt = (int64_t)K * n;
    if (!gp) {
      HIPCHK(launch_hs_c2r_z<double>(Zh.as<cpx<double>>(), z.as<double>(), part.as<double>(), cnt,
                                     tw.as<cpx<double>>(), G, st));
      return;
    }
    lines.c2r(Zh.as<cpx<double>>(), gR.as<double>(), cnt);
    HIPCHK(launch_gp_hs_epilog<double>(kHsZ, gR.as<double>(), z.as<double>(), bdev.as<double>(),
                                       smp.as<double>(), nullptr, part.as<double>(), G.X, G.Y, r,
                                       sbx, sby, 1.0 / (double)P, cnt, st));
  }
  // D = real(ifft2(Dh)) (the rollback); Dh stays intact
  void c2r_plain_D() {
    if (!gp) {
      HIPCHK(launch_c2r_plain<double>(Dh.as<cpx<double>>(), F, D.as<double>(), P, KG,
                                      tw.as<cpx<double>>(), G, 1.0 / (double)P, st));
      return;
    }
    HIPCHK(hipMemcpyAsync(Ch.p, Dh.p, Dh.bytes, hipMemcpyDeviceToDevice, st));
    lines.c2r(Ch.as<cpx<double>>(), gR.as<double>(), KG);
    HIPCHK(launch_gp_epilog<double>(0, gR.as<double>(), D.as<double>(), nullptr, nullptr, nullptr,
                                    0, 1.0 / (double)P, r, G.X, G.Y, KG, nullptr, 0.0, 0, st));
  }

  // v = real(ifft2(H zhat)) from Xi (= H zhat) and the objective of (z, d_hat)
  // (objectiveFunction, L23:326-343); pair[2] must hold sum |z|.
  double finish_objective() {
    c2r_v(nullptr);
    HIPCHK(launch_sum_pairs<double>(part.as<double>(), W * n, pair.as<double>(), st));
    // the data term and sum |z| over every rank's images, reduced in a copy: pair[2] (this
    // rank's sum |z|) serves every objective of a d-phase
    const double* ps = pair.as<double>();
    if (dist) {
      HIPCHK(hipMemcpyAsync(pair.as<double>() + 8, ps, 4 * sizeof(double), hipMemcpyDeviceToDevice, st));
      ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, pair.as<double>() + 8, 4);
      ps = pair.as<double>() + 8;
    }
    double h4[4];
    HIPCHK(hipMemcpyAsync(h4, ps, sizeof h4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return p.lambda_residual * 0.5 * h4[0] + p.lambda_prior * W * h4[2];   // g_z: z repeated W times (L23:332,338)
  }
  // zhat = fft2(z) (L23:100,158,234), sum |z|, v = H z and the objective
  double objective_fresh() {
    r2c_full(z.as<double>(), Zh.as<cpx<double>>(), (int64_t)K * n);
    HIPCHK(launch_norms<double>(z.as<double>(), nullptr, (int64_t)z.bytes / 8, part.as<double>(),
                                pair.as<double>() + 2, st));
    HIPCHK(launch_hs_synth<double>(Dh.as<cpx<double>>(), Zh.as<cpx<double>>(),
                                   Xi.as<cpx<double>>(), F, W, K, n, st));
    return finish_objective();
  }
  // global: a and b are rank-local (z; D is the same on every rank)
  double rel_change(const DevBuf& a, const DevBuf& b, bool global = false) {
    HIPCHK(launch_norms<double>(a.as<double>(), b.as<double>(), (int64_t)a.bytes / 8,
                                part.as<double>(), pair.as<double>() + 4, st));
    if (global && dist) ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, pair.as<double>() + 4, 2);
    double h2[2];
    HIPCHK(hipMemcpyAsync(h2, pair.as<double>() + 4, sizeof h2, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return std::sqrt(h2[0]) / std::sqrt(h2[1]);
  }

  // ---- one outer iteration (L23:86-226) ---------------------------------------
  void outer_iteration() {
    const auto t0 = std::chrono::steady_clock::now();
    const double obj_min = std::min(obj_filter, obj_z);   // L23:94
    HIPCHK(hipMemcpyAsync(Dold.p, D.p, D.bytes, hipMemcpyDeviceToDevice, st));    // d_old (L23:95)
    HIPCHK(hipMemcpyAsync(Dhold.p, Dh.p, Dh.bytes, hipMemcpyDeviceToDevice, st)); // d_hat_old
    // z_hat = fft2(z) (L23:100) and v_D{1} = H z of the first d-iteration (L23:108)
    objective_fresh();
    // opt_f = (Z_f' Z_f + rho I)^-1 as a Cholesky factor per bin (L23:290)
    // on the matrix cores (gramchol.hip, K <= 192; no right-hand side here: NV = 0)
    if (rt.dfactor == DFactor::WBig) {
      HIPCHK(launch_wbig_gram(Zh.as<cpx<double>>(), Zh.as<cpx<double>>(), Xw.as<cpx<double>>(),
                              L.as<cpx<double>>(), h.as<cpx<double>>(), F, K, n, p.rho_d, 0, st));
    } else if (rt.dfactor == DFactor::Big) {
      // the Gram of this rank's images (rho I on rank 0 only), summed over the ranks, then
      // the same Cholesky on every rank
      HIPCHK(launch_gram_big(Zh.as<cpx<double>>(), Zh.as<cpx<double>>(), Xw.as<cpx<double>>(),
                             L.as<cpx<double>>(), h.as<cpx<double>>(), F, K, n,
                             ctx->rank == 0 ? p.rho_d : 0.0, 0, st, false));
      ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, L.as<double>(),
                     (size_t)2 * F * (K * (K + 1) / 2));
      HIPCHK(launch_chol_big(L.as<cpx<double>>(), F, K, st));
    } else
      HIPCHK(launch_gram_chol_mf(Zh.as<cpx<double>>(), Zh.as<cpx<double>>(), L.as<cpx<double>>(),
                                 h.as<cpx<double>>(), F, K, n, p.rho_d, 0, st));
    // 64 < K <= 112: the tile d-solve over the W wavelengths (factor read once per solve)
    if (rt.dsolve == DSolve::Tile) HIPCHK(launch_invert_diag(L.as<cpx<double>>(), F, K, st));
    for (int id = 0; id < p.max_it_d; ++id) {                                    // L23:102
      // c = 1: masked data split (L23:112, 117, 120-121)
      data_r2c(eD, th_D1);
      // c = 2: kernel constraint split, y = -d_D{2} (L23:113, 117, 120-121)
      dual_r2c();
      // d_hat = opt (Z' xi1 + rho xi2) per (bin, wavelength)  (L23:125, 289-295)
      HIPCHK(launch_hs_corr<double>(Zh.as<cpx<double>>(), Xi.as<cpx<double>>(),
                                    h.as<cpx<double>>(), F, W, K, n, st));
      if (dist) ctx_collective(ctx, st, CCSC_COMM_ALLREDUCE_SUM, h.as<double>(), (size_t)2 * F * W * K);
      if (rt.dfactor == DFactor::WBig)
        HIPCHK(launch_wbig_solve(L.as<cpx<double>>(), h.as<cpx<double>>(), Ch.as<cpx<double>>(),
                                 Dh.as<cpx<double>>(), 1, F, K, n, p.rho_d, W, st));
      else if (rt.dsolve == DSolve::Tile)
        HIPCHK(launch_dsolve_tile(L.as<cpx<double>>(), h.as<cpx<double>>(), Ch.as<cpx<double>>(),
                                  Dh.as<cpx<double>>(), 1, F, K, p.rho_d, W, st));
      else
        HIPCHK(launch_dsolve<double>(L.as<cpx<double>>(), h.as<cpx<double>>(), Ch.as<cpx<double>>(),
                                     Dh.as<cpx<double>>(), 1, F, K, p.rho_d, W, st));
      // d = real(ifft2(d_hat)) (L23:126); support of d - d_D{2} -> u_D{2} of the next d-iteration
      c2r_dout();
      HIPCHK(launch_project<double>(supp.as<double>(), Usup.as<double>(), KG, SS, 1.0, st));
      // objective (L23:132); its H z is v_D{1} of the next d-iteration (z is fixed here)
      HIPCHK(launch_hs_synth<double>(Dh.as<cpx<double>>(), Zh.as<cpx<double>>(),
                                     Xi.as<cpx<double>>(), F, W, K, n, st));
      obj = finish_objective();
      lg.tr_od[lg.d_slot(id)] = obj;
    }
    obj_filter = obj;                                                            // L23:139
    const double d_diff = rel_change(D, Dold);                                   // L23:142-146
    lg.tr_dd[lg.d_slot(0)] = d_diff;

    // ---- Z-phase (L23:149-200) ----
    // 1 / (rho + sum_{w,k} |d_hat|^2) per bin (L23:262-268, 317)
    HIPCHK(launch_sden<double>(Dh.as<cpx<double>>(), sden.as<double>(), F, KG, p.rho_z, 1.0, st));
    HIPCHK(hipMemcpyAsync(zold.p, z.p, z.bytes, hipMemcpyDeviceToDevice, st));  // z_old (L23:159)
    // v = H z is current: the last D objective used z_hat = fft2(z) (L23:158)
    for (int iz = 0; iz < p.max_it_z; ++iz) {                                    // L23:165
      data_r2c(eZ, th_Z1);                                                       // L23:175,180,183-184
      z_r2c();                                                                   // L23:176,180,183-184
      HIPCHK(launch_hs_analysis<double>(Dh.as<cpx<double>>(), Xi.as<cpx<double>>(),
                                        Zh.as<cpx<double>>(), sden.as<double>(), p.rho_z,
                                        Zh.as<cpx<double>>(), F, W, K, n, st));  // L23:188, 302-324
      // objective (L23:195); H zhat is v_Z{1} of the next z-iteration (L23:171) -- formed
      // before the C2R of zhat, which consumes Zh on global-pass slices
      HIPCHK(launch_hs_synth<double>(Dh.as<cpx<double>>(), Zh.as<cpx<double>>(),
                                     Xi.as<cpx<double>>(), F, W, K, n, st));
      c2r_z();                                                                   // L23:189
      HIPCHK(launch_sum_pairs<double>(part.as<double>(), K * n, pair.as<double>() + 2, st));
      obj = finish_objective();
      lg.tr_oz[lg.z_slot(iz)] = obj;
    }
    obj_z = obj;                                                                 // L23:202
    int flags = 0;
    if (obj_min <= obj_filter && obj_min <= obj_z) {                             // L23:204-213 (Q16)
      // roll back to the iterate before this outer iteration and stop
      HIPCHK(hipMemcpyAsync(z.p, zold.p, z.bytes, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(Dh.p, Dhold.p, Dh.bytes, hipMemcpyDeviceToDevice, st));
      c2r_plain_D();
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

  void results(ccsc_outputs* out) {
    if (!out) return;
    if (out->d_res) {
      // d_res = circshift(d, [r r 0 0])(1:2r+1, 1:2r+1, :, :)  (L23:231-232)
      std::vector<double> Dh_((size_t)KG * P);
      HIPCHK(hipMemcpy(Dh_.data(), D.p, D.bytes, hipMemcpyDeviceToHost));
      for (int gI = 0; gI < KG; ++gI)
        for (int j = 0; j < s; ++j)
          for (int i = 0; i < s; ++i) {
            const int x = (i - r + G.X) % G.X, y = (j - r + G.Y) % G.Y;
            out->d_res[i + (size_t)s * (j + (size_t)s * gI)] = Dh_[(size_t)gI * P + (size_t)y * G.X + x];
          }
    }
    if (out->z_res) HIPCHK(hipMemcpy(out->z_res, z.p, z.bytes, hipMemcpyDeviceToHost));
    if (out->DZ) {
      // Dz = real(ifft2(sum_k d_hat .* fft2(z))) + smoothinit  (L23:234-235)
      DevBuf dz;
      dz.alloc(v.bytes);
      r2c_full(z.as<double>(), Zh.as<cpx<double>>(), (int64_t)K * n);
      HIPCHK(launch_hs_synth<double>(Dh.as<cpx<double>>(), Zh.as<cpx<double>>(),
                                     Xi.as<cpx<double>>(), F, W, K, n, st));
      c2r_v(dz.as<double>());
      HIPCHK(hipStreamSynchronize(st));   // st is non-blocking: hipMemcpy does not order after it
      HIPCHK(hipMemcpy(out->DZ, dz.p, dz.bytes, hipMemcpyDeviceToHost));
    }
    if (out->obj_val) *out->obj_val = obj;   // the last objective the learner evaluated
  }

  // The codes as results() copies them into z_res: one column of X Y K values per image.
  const double* codes_dense(int64_t* M, int64_t* nloc) {
    HIPCHK(hipStreamSynchronize(st));
    *nloc = n;
    *M = (int64_t)K * P;
    return z.as<double>();
  }
};

}  // namespace ccsc

struct ccsc_session {
  std::unique_ptr<ccsc::Session2D> s2;
  std::unique_ptr<ccsc::SessionHS> hs;
  ccsc_ctx* ctx() const { return s2 ? s2->ctx : hs->ctx; }
};

namespace ccsc {
// One rank of a multi-device context failed: mark the group aborted (once, whichever
// threads fail), wake the in-process exchange, wait until no rank is inside a collective
// call, then abort every RCCL communicator so the other ranks' kernels waiting on the
// failed rank return (see CommGroup).  The wait has no time limit and needs none: the
// group's communicators are non-blocking (init_group_comms), so an enqueue returns at
// once and collective()'s poll loop leaves as soon as `aborted` is set -- a communicator
// is never aborted (freed) while another thread is inside RCCL with it, and a rank that
// enters collective() later sees `aborted` (set before the wait) before it reads `comm`.
static void abort_group(ccsc_ctx* ctx) {
  CommGroup* g = ctx->grp.get();
  std::lock_guard<std::mutex> lk(g->mu);
  if (g->aborted.exchange(true)) return;
  if (ctx->hg) ctx->hg->abort();
  while (g->inflight.load() > 0) std::this_thread::sleep_for(std::chrono::microseconds(50));
  for (ccsc_ctx* u : ctx->subs)
    if (u->comm) {
      ncclCommAbort(u->comm);
      u->comm = nullptr;
    }
}

// Before a learn on a multi-device context whose previous learn failed: fresh
// communicators (RCCL: ncclCommInitAll over the device list; repeated devices: a new
// in-process exchange), so a failure does not leave the (MEX-cached) context unusable.
static void reset_group(ccsc_ctx* ctx) {
  CommGroup* g = ctx->grp.get();
  if (!g || !g->aborted.load()) return;
  std::lock_guard<std::mutex> lk(g->mu);
  const int nd = (int)ctx->subs.size();
  if (ctx->hg) {
    ctx->hg.reset(new HostGroup(nd));
    for (int i = 0; i < nd; ++i) ctx->hg_ranks[i] = HostGroupRank{ctx->hg.get(), i};
  } else {
    std::vector<ncclComm_t> comms(nd, nullptr);
    init_group_comms(comms, ctx->devices.data(), nd);
    for (int i = 0; i < nd; ++i) ctx->subs[i]->comm = comms[i];
    HIPCHK(hipSetDevice(ctx->device));
  }
  g->aborted.store(false);
}

// Test-only fault injection (failure detection): CCSC_TEST_FAIL_RANK =
// "rank:outer" makes that rank of a multi-device learn throw before outer iteration
// `outer`, while the other ranks run into their next collective.
static bool injected_fault(int rank, int outer) {
  const char* ev = std::getenv("CCSC_TEST_FAIL_RANK");
  int r = -1, o = -1;
  return ev && std::sscanf(ev, "%d:%d", &r, &o) == 2 && r == rank && o == outer;
}

// ccsc_learn on a multi-device context: the caller's whole problem (b, z0, outputs
// over all n patches) is split at the block boundaries of ccsc_shard; rank i runs
// on sub-context i in its own host thread, the calling thread drives rank 0 and is
// the only one that calls back (include/ccsc.h threading rule).  Collectives
// inside the sessions (RCCL, or the in-process exchange) keep the ranks in step.
static void learn_group(ccsc_ctx* ctx, const ccsc_problem& pin, const double* b, const double* d0,
                        const double* z0, ccsc_outputs* out, ccsc_iterlog* log, ccsc_cb cb,
                        void* user) {
  reset_group(ctx);
  ccsc_problem q = pin;
  resolve_problem(q);
  Geom g;
  check_supported(q, &g);
  const int nd = (int)ctx->subs.size();
  const bool is4 = q.variant == CCSC_L4D, is3 = q.variant == CCSC_L3D;
  const int64_t NV = (int64_t)q.views[0] * q.views[1];
  const int64_t bpatch = q.sb[0] * q.sb[1] * (is3 ? q.sb[2] : 1) * NV;   // b [sb.., (U,V), n]
  const int64_t zpatch = (int64_t)q.K * (int64_t)g.P();                  // z [X,Y,(T),K, n]
  const int64_t xpatch = is4 ? NV * q.sb[0] * q.sb[1] : (int64_t)g.P();  // DZ per patch
  const int64_t KG = (int64_t)q.K * NV;
  const int64_t SS = (int64_t)q.psf * q.psf * (is3 ? q.psf : 1);
  std::vector<std::vector<double>> dscr(nd), oscr(nd);
  std::vector<std::string> errs(nd);
  std::vector<int> codes(nd, CCSC_OK);
  auto run = [&](int i) {
    // the session outlives the catch: a failed rank aborts the group BEFORE its stream is
    // drained, so no rank waits on a collective whose peer has stopped
    std::unique_ptr<Session2D> Sp;
    try {
      ccsc_ctx* u = ctx->subs[i];
      HIPCHK(hipSetDevice(u->device));
      int64_t b0 = 0, nb = 0;
      shard(q, i, nd, b0, nb);
      const int64_t p0 = b0 * q.ni;
      const double* zi = z0 ? (q.variant == CCSC_DZPAR ? z0 : z0 + p0 * zpatch) : nullptr;
      Sp.reset(new Session2D(u, q, b + p0 * bpatch, d0, zi));
      Session2D& S = *Sp;
      run_outer(S, S.p.max_it, i == 0 ? cb : nullptr, user, [&](int it) {
        if (injected_fault(i, it))
          throw Err(CCSC_E_INVALID, "injected fault (CCSC_TEST_FAIL_RANK) before outer iteration " +
                                        std::to_string(it));
      });
      ccsc_outputs o{};
      if (out) {
        // d_res and obj_val are collectives: every rank asks when the caller does
        if (out->d_res) {
          dscr[i].resize(i == 0 ? 0 : (size_t)(KG * SS));
          o.d_res = i == 0 ? out->d_res : dscr[i].data();
        }
        if (out->obj_val) {
          oscr[i].resize(1);
          o.obj_val = i == 0 ? out->obj_val : oscr[i].data();
        }
        if (out->z_res) o.z_res = out->z_res + p0 * zpatch;
        if (out->DZ) o.DZ = out->DZ + p0 * xpatch;
      }
      S.results(out ? &o : nullptr);
      if (i == 0) S.lg.write(log);
    } catch (const Err& e) {
      errs[i] = e.what();
      codes[i] = e.code;
      abort_group(ctx);
    } catch (const std::exception& e) {
      errs[i] = e.what();
      codes[i] = CCSC_E_INVALID;
      abort_group(ctx);
    }
    try {
      Sp.reset();
    } catch (...) {
    }
  };
  std::vector<std::thread> th;
  for (int i = 1; i < nd; ++i) th.emplace_back(run, i);
  run(0);
  for (auto& t : th) t.join();
  HIPCHK(hipSetDevice(ctx->device));
  for (int i = 0; i < nd; ++i)   // the first failure (others are its consequences)
    if (codes[i] != CCSC_OK && !errs[i].empty() && errs[i].find("host communicator") == std::string::npos)
      throw Err(codes[i], "device " + std::to_string(ctx->subs[i]->device) + " (rank " +
                              std::to_string(i) + "): " + errs[i]);
  for (int i = 0; i < nd; ++i)
    if (codes[i] != CCSC_OK) throw Err(codes[i], "rank " + std::to_string(i) + ": " + errs[i]);
}
}  // namespace ccsc

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

int32_t ccsc_abi_version(void) { return CCSC_ABI_VERSION; }

int32_t ccsc_resolve(ccsc_problem* p, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!p) throw Err(CCSC_E_INVALID, "problem is NULL");
    resolve_problem(*p);
  });
}

int32_t ccsc_supported(const ccsc_problem* p, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!p) throw Err(CCSC_E_INVALID, "problem is NULL");
    ccsc_problem q = *p;
    resolve_problem(q);
    check_supported(q, nullptr);
  });
}

int32_t ccsc_shard(const ccsc_problem* p, int32_t rank, int32_t nranks, int64_t* block_begin,
                   int64_t* block_count, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!p || !block_begin || !block_count) throw Err(CCSC_E_INVALID, "NULL argument");
    ccsc_problem q = *p;
    resolve_problem(q);
    shard(q, rank, nranks, *block_begin, *block_count);
  });
}

int32_t ccsc_plan_bytes(const ccsc_problem* p, int32_t rank, int32_t nranks, uint64_t* bytes,
                        char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!p || !bytes) throw Err(CCSC_E_INVALID, "NULL argument");
    ccsc_problem q = *p;
    resolve_problem(q);
    Geom g;
    check_supported(q, &g);
    // the route and rows of the session that (rank, nranks) would create
    *bytes = q.variant == CCSC_HS23
                 ? plan_total(mem_plan_hs(q, g, route_hs(q, g, rank, nranks, false)))
                 : plan_total(mem_plan2d(q, g, route2d(q, g, rank, nranks, false)));
  });
}

int32_t ccsc_device_count(int32_t* count, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    int c = 0;
    HIPCHK(hipGetDeviceCount(&c));
    *count = c;
  });
}

int32_t ccsc_get_unique_id(uint8_t* uid128, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    std::memcpy(uid128, &id, 128);
  });
}

ccsc_ctx* ccsc_create(int32_t device, int32_t rank, int32_t nranks, const uint8_t* uid128,
                      char* err, size_t errlen) {
  ccsc_ctx* ctx = nullptr;
  const int rc = guarded(err, errlen, [&] {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw Err(CCSC_E_INVALID, "bad rank/nranks");
    std::unique_ptr<ccsc_ctx> c(new ccsc_ctx());
    c->device = device;
    c->rank = rank;
    c->nranks = nranks;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (nranks > 1) {
      if (!uid128) throw Err(CCSC_E_INVALID, "multi-rank context needs the RCCL unique id");
      ncclUniqueId id;
      std::memcpy(&id, uid128, 128);
      NCCLCHK(ncclCommInitRank(&c->comm, nranks, id, rank));
    }
    ctx = c.release();
  });
  return rc == CCSC_OK ? ctx : nullptr;
}

ccsc_ctx* ccsc_create_hostcomm(int32_t device, int32_t rank, int32_t nranks, ccsc_comm_fn fn,
                               void* user, char* err, size_t errlen) {
  ccsc_ctx* ctx = nullptr;
  const int rc = guarded(err, errlen, [&] {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw Err(CCSC_E_INVALID, "bad rank/nranks");
    if (nranks > 1 && !fn) throw Err(CCSC_E_INVALID, "host communicator needs a callback");
    std::unique_ptr<ccsc_ctx> c(new ccsc_ctx());
    c->device = device;
    c->rank = rank;
    c->nranks = nranks;
    c->hostfn = fn;
    c->hostuser = user;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    ctx = c.release();
  });
  return rc == CCSC_OK ? ctx : nullptr;
}

ccsc_ctx* ccsc_create_multi(const int32_t* devices, int32_t ndev, char* err, size_t errlen) {
  ccsc_ctx* ctx = nullptr;
  const int rc = guarded(err, errlen, [&] {
    if (!devices || ndev < 1) throw Err(CCSC_E_INVALID, "empty device list");
    int count = 0;
    HIPCHK(hipGetDeviceCount(&count));
    for (int i = 0; i < ndev; ++i)
      if (devices[i] < 0 || devices[i] >= count)
        throw Err(CCSC_E_INVALID, "device " + std::to_string(devices[i]) + " out of range (" +
                                      std::to_string(count) + " visible)");
    // every object is owned by `c` (subs, their streams and communicators) the moment it
    // exists, so an error at any step releases all of it through ccsc_destroy
    struct Guard {
      ccsc_ctx* c;
      ~Guard() {
        if (c) ccsc_destroy(c);
      }
    } guard{new ccsc_ctx()};
    ccsc_ctx* c = guard.c;
    c->device = devices[0];
    c->nranks = ndev;
    c->devices.assign(devices, devices + ndev);
    HIPCHK(hipSetDevice(devices[0]));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const char* self_ev = std::getenv("CCSC_TEST_RCCL_SELF");
    const bool rccl_self = ndev == 1 && self_ev && std::atoi(self_ev) != 0;
    if (ndev > 1 || rccl_self) {
      bool distinct = true;
      for (int i = 0; i < ndev; ++i)
        for (int j = 0; j < i; ++j) distinct = distinct && devices[i] != devices[j];
      c->grp = std::make_shared<CommGroup>();
      if (!distinct) {
        c->hg.reset(new HostGroup(ndev));
        c->hg_ranks.resize(ndev);
      }
      for (int i = 0; i < ndev; ++i) {
        c->subs.push_back(new ccsc_ctx());
        ccsc_ctx* u = c->subs.back();
        u->device = devices[i];
        u->rank = i;
        u->nranks = ndev;
        u->rccl_self = rccl_self;
        u->grp = c->grp;
        if (c->hg) {
          c->hg_ranks[i] = HostGroupRank{c->hg.get(), i};
          u->hostfn = host_group_fn;
          u->hostuser = &c->hg_ranks[i];
        }
      }
      if (distinct) {
        std::vector<ncclComm_t> comms(ndev, nullptr);
        init_group_comms(comms, devices, ndev);
        for (int i = 0; i < ndev; ++i) c->subs[i]->comm = comms[i];
      }
      for (int i = 0; i < ndev; ++i) {
        HIPCHK(hipSetDevice(devices[i]));
        HIPCHK(hipStreamCreateWithFlags(&c->subs[i]->stream, hipStreamNonBlocking));
      }
      HIPCHK(hipSetDevice(devices[0]));
    }
    ctx = c;
    guard.c = nullptr;
  });
  return rc == CCSC_OK ? ctx : nullptr;
}

int32_t ccsc_comm_ranks(ccsc_ctx* ctx, int32_t* ranks, int32_t* transport, char* err,
                        size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !ranks) throw Err(CCSC_E_INVALID, "NULL argument");
    // a multi-device context reports the communicator of its rank 0
    const ccsc_ctx* u = ctx->subs.empty() ? ctx : ctx->subs[0];
    int32_t t = CCSC_TRANSPORT_NONE, n = 1;
    if (u->nranks > 1 && u->hostfn) {
      t = CCSC_TRANSPORT_HOST;
      n = u->nranks;
    } else if (u->nranks > 1 || u->rccl_self) {
      if (!u->comm) throw Err(CCSC_E_STATE, "the communicator was aborted (a rank failed)");
      int c = 0;
      NCCLCHK(ncclCommCount(u->comm, &c));
      t = CCSC_TRANSPORT_RCCL;
      n = c;
    }
    *ranks = n;
    if (transport) *transport = t;
  });
}

void ccsc_destroy(ccsc_ctx* ctx) {
  if (!ctx) return;
  for (ccsc_ctx* u : ctx->subs) ccsc_destroy(u);
  ctx->subs.clear();
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (ctx->comm) ncclCommDestroy(ctx->comm);
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}

ccsc_session* ccsc_session_create(ccsc_ctx* ctx, const ccsc_problem* p, const double* b,
                                  const double* d0, const double* z0, char* err, size_t errlen) {
  ccsc_session* out = nullptr;
  guarded(err, errlen, [&] {
    if (!ctx || !p) throw Err(CCSC_E_INVALID, "NULL ctx/problem");
    if (p->variant == CCSC_HS23)
      throw Err(CCSC_E_INVALID, "the 2-3D learner takes smooth_init: use ccsc_session_create_hs23");
    if (!ctx->subs.empty())
      throw Err(CCSC_E_UNSUPPORTED, "sessions run on a one-device context (one per rank); a "
                                    "multi-device context serves ccsc_learn");
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<ccsc_session> s(new ccsc_session());
    s->s2.reset(new Session2D(ctx, *p, b, d0, z0));
    out = s.release();
  });
  return out;
}

ccsc_session* ccsc_session_create_hs23(ccsc_ctx* ctx, const ccsc_problem* p, const double* b,
                                       const double* smooth_init, const double* d0,
                                       const double* z0, char* err, size_t errlen) {
  ccsc_session* out = nullptr;
  guarded(err, errlen, [&] {
    if (!ctx || !p) throw Err(CCSC_E_INVALID, "NULL ctx/problem");
    if (!ctx->subs.empty())
      throw Err(CCSC_E_UNSUPPORTED, "the 2-3D learner runs one process per GPU (a rank context of "
                                    "ccsc_create / ccsc_create_hostcomm), not on a device list");
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<ccsc_session> s(new ccsc_session());
    s->hs.reset(new SessionHS(ctx, *p, b, smooth_init, d0, z0));
    out = s.release();
  });
  return out;
}

static void need_session(const ccsc_session* s) {
  if (!s || (!s->s2 && !s->hs)) throw Err(CCSC_E_STATE, "no session");
}

int32_t ccsc_session_step(ccsc_session* s, int32_t n_outer, int32_t* done, char* err,
                          size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    HIPCHK(hipSetDevice(s->ctx()->device));
    if (s->hs) run_outer(*s->hs, n_outer, nullptr, nullptr);
    else run_outer(*s->s2, n_outer, nullptr, nullptr);
    if (done) *done = (s->hs ? s->hs->lg : s->s2->lg).finished ? 1 : 0;
  });
}

int32_t ccsc_session_objective(ccsc_session* s, double* obj, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    if (!obj) throw Err(CCSC_E_INVALID, "NULL obj");
    HIPCHK(hipSetDevice(s->ctx()->device));
    if (s->hs) *obj = s->hs->objective_fresh();
    else *obj = s->s2->objective(s->s2->dhat.as<cpx<double>>(), nullptr);
  });
}

int32_t ccsc_session_results(ccsc_session* s, ccsc_outputs* out, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    HIPCHK(hipSetDevice(s->ctx()->device));
    if (s->hs) s->hs->results(out);
    else s->s2->results(out);
  });
}

int32_t ccsc_session_codes_count(ccsc_session* s, double eps, int64_t* jc, int64_t* rows,
                                 int64_t* cols, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_eps(eps);
    if (!jc) throw Err(CCSC_E_INVALID, "NULL jc");
    need_session(s);
    HIPCHK(hipSetDevice(s->ctx()->device));
    int64_t M = 0, n = 0;
    const double* z = s->hs ? s->hs->codes_dense(&M, &n) : s->s2->codes_dense(&M, &n);
    codes_check_shape(M, n);
    jc[0] = 0;
    codes_count_dev(s->ctx(), z, M, n, eps, jc);
    if (rows) *rows = M;
    if (cols) *cols = n;
  });
}

int32_t ccsc_session_codes_fill(ccsc_session* s, double eps, int64_t* ir, double* pr,
                                int64_t capacity, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_fill_args(eps, ir, pr, capacity);
    need_session(s);
    HIPCHK(hipSetDevice(s->ctx()->device));
    int64_t M = 0, n = 0;
    const double* z = s->hs ? s->hs->codes_dense(&M, &n) : s->s2->codes_dense(&M, &n);
    codes_check_shape(M, n);
    std::vector<int64_t> jc((size_t)n + 1, 0);
    codes_count_dev(s->ctx(), z, M, n, eps, jc.data());
    codes_check_capacity(capacity, jc[(size_t)n]);
    codes_fill_dev(s->ctx(), z, M, n, eps, jc.data(), ir, pr, false);
  });
}

int32_t ccsc_session_iterlog(ccsc_session* s, ccsc_iterlog* log, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    (s->hs ? s->hs->lg : s->s2->lg).write(log);
  });
}

int32_t ccsc_session_set_profiling(ccsc_session* s, int32_t on) {
  if (!s || !s->s2) return s && s->hs ? CCSC_OK : CCSC_E_STATE;  // 2-3D: no per-kernel timers
  s->s2->prof = on != 0;
  return CCSC_OK;
}

int32_t ccsc_session_kernel_stats(ccsc_session* s, int32_t id, int64_t* launches,
                                  double* total_ms, double* alg_bytes_per_launch, char* err,
                                  size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    if (id < 0 || id > 4) throw Err(CCSC_E_INVALID, "kernel id out of range");
    const bool t = (bool)s->s2;
    if (launches) *launches = t ? s->s2->k_launch[id] : 0;
    if (total_ms) *total_ms = t ? s->s2->k_ms[id] : 0.0;
    if (alg_bytes_per_launch) *alg_bytes_per_launch = t ? s->s2->alg_bytes(id) : 0.0;
    (void)kKernelNames;
  });
}

void ccsc_session_destroy(ccsc_session* s) {
  if (!s) return;
  if (s->s2 || s->hs) hipSetDevice(s->ctx()->device);
  delete s;
}

int32_t ccsc_learn_hs23(ccsc_ctx* ctx, const ccsc_problem* p, const double* b,
                        const double* smooth_init, const double* d0, const double* z0,
                        ccsc_outputs* out, ccsc_iterlog* log, ccsc_cb cb, void* user, char* err,
                        size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !p) throw Err(CCSC_E_INVALID, "NULL ctx/problem");
    if (!ctx->subs.empty())
      throw Err(CCSC_E_UNSUPPORTED, "the 2-3D learner runs one process per GPU (a rank context of "
                                    "ccsc_create / ccsc_create_hostcomm), not on a device list");
    HIPCHK(hipSetDevice(ctx->device));
    SessionHS S(ctx, *p, b, smooth_init, d0, z0);
    run_outer(S, S.p.max_it, cb, user);
    S.results(out);
    S.lg.write(log);
  });
}

int32_t ccsc_learn(ccsc_ctx* ctx, const ccsc_problem* p, const double* b, const double* d0,
                   const double* z0, ccsc_outputs* out, ccsc_iterlog* log, ccsc_cb cb,
                   void* user, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    if (!ctx || !p) throw Err(CCSC_E_INVALID, "NULL ctx/problem");
    if (p->variant == CCSC_HS23)
      throw Err(CCSC_E_INVALID, "the 2-3D learner takes smooth_init: use ccsc_learn_hs23");
    if (!ctx->subs.empty()) {
      learn_group(ctx, *p, b, d0, z0, out, log, cb, user);
      return;
    }
    HIPCHK(hipSetDevice(ctx->device));
    Session2D S(ctx, *p, b, d0, z0);
    run_outer(S, S.p.max_it, cb, user);
    S.results(out);
    S.lg.write(log);
  });
}

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
    HIPCHK(launch_r2c_embed<double>(a.as<double>(), P, X, Y, 0, 0, hs.as<cpx<double>>(), G.F,
                                    count, tw.as<cpx<double>>(), G, st));
    HIPCHK(launch_c2r_plain<double>(hs.as<cpx<double>>(), G.F, rt.as<double>(), P, count,
                                    tw.as<cpx<double>>(), G, 1.0 / (double)P, st));
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
    cpx<double>* Sp = S.as<cpx<double>>();
    lines.r2c(a.as<double>(), Sp, count);
    HIPCHK(hipStreamSynchronize(st));
    if (out_halfspec) HIPCHK(hipMemcpy(out_halfspec, S.p, S.bytes, hipMemcpyDeviceToHost));
    if (!roundtrip) return;
    rt.alloc((size_t)(P * count) * 8);
    lines.inv_cols(Sp, count);
    RowArgs<double> rr{};   // no smoothinit, no clamp, zero crop offsets, the full extent
    rr.S = Sp;
    rr.res = rt.as<double>();
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
    HIPCHK(launch_tfft<double>(a.as<cpx<double>>(), b.as<cpx<double>>(), count, Yn, F2, -1,
                               tw.as<cpx<double>>(), Gt, st));
    if (roundtrip)
      HIPCHK(launch_tfft<double>(b.as<cpx<double>>(), a.as<cpx<double>>(), count, Yn, F2, +1,
                                 tw.as<cpx<double>>(), Gt, st));
    HIPCHK(hipStreamSynchronize(st));
    if (out) HIPCHK(hipMemcpy(out, b.p, b.bytes, hipMemcpyDeviceToHost));
    if (roundtrip) HIPCHK(hipMemcpy(roundtrip, a.p, a.bytes, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
