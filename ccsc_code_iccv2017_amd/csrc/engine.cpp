// libccsc C-ABI (include/ccsc.h): contexts, the plan queries, sessions and the learners.  The
// sessions are in session2d.cpp / session_hs.cpp behind session.hpp, the transport in
// comm.cpp, the FFT test hooks in fft_hooks.cpp.
#include "session.hpp"

#include <cstdlib>
#include <cstring>
#include <thread>

using namespace ccsc;

namespace ccsc {

// up to n_outer outer iterations of a session: `pre` (the outer index) before each, `cb` after
static void run_outer(Session& s, int n_outer, ccsc_cb cb, void* user,
                      const std::function<void(int)>& pre = nullptr) {
  HostLog& lg = s.lg;
  lg.ensure_trace_capacity(lg.outer_done + n_outer);
  for (int i = 0; i < n_outer && !lg.finished; ++i) {
    if (pre) pre(lg.outer_done);
    s.outer_iteration();
    if (cb) cb(user, lg.outer_done, lg.v_obj_d.back(), lg.v_obj_z.back(), lg.v_tim.back());
  }
}
}  // namespace ccsc

struct ccsc_session {
  std::unique_ptr<ccsc::Session> s;
};

namespace ccsc {
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
    std::unique_ptr<Session> Sp;
    try {
      ccsc_ctx* u = ctx->subs[i];
      HIPCHK(hipSetDevice(u->device));
      int64_t b0 = 0, nb = 0;
      shard(q, i, nd, b0, nb);
      const int64_t p0 = b0 * q.ni;
      const double* zi = z0 ? (q.variant == CCSC_DZPAR ? z0 : z0 + p0 * zpatch) : nullptr;
      Sp = make_session2d(u, q, b + p0 * bpatch, d0, zi);
      Session& S = *Sp;
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
    s->s = make_session2d(ctx, *p, b, d0, z0);
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
    s->s = make_session_hs(ctx, *p, b, smooth_init, d0, z0);
    out = s.release();
  });
  return out;
}

static void need_session(const ccsc_session* s) {
  if (!s || !s->s) throw Err(CCSC_E_STATE, "no session");
}

int32_t ccsc_session_step(ccsc_session* s, int32_t n_outer, int32_t* done, char* err,
                          size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    HIPCHK(hipSetDevice(s->s->ctx->device));
    run_outer(*s->s, n_outer, nullptr, nullptr);
    if (done) *done = s->s->lg.finished ? 1 : 0;
  });
}

int32_t ccsc_session_objective(ccsc_session* s, double* obj, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    if (!obj) throw Err(CCSC_E_INVALID, "NULL obj");
    HIPCHK(hipSetDevice(s->s->ctx->device));
    *obj = s->s->objective_now();
  });
}

int32_t ccsc_session_results(ccsc_session* s, ccsc_outputs* out, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    HIPCHK(hipSetDevice(s->s->ctx->device));
    s->s->results(out);
  });
}

int32_t ccsc_session_codes_count(ccsc_session* s, double eps, int64_t* jc, int64_t* rows,
                                 int64_t* cols, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_eps(eps);
    if (!jc) throw Err(CCSC_E_INVALID, "NULL jc");
    need_session(s);
    HIPCHK(hipSetDevice(s->s->ctx->device));
    int64_t M = 0, n = 0;
    const double* z = s->s->codes_dense(&M, &n);
    codes_check_shape(M, n);
    jc[0] = 0;
    codes_count_dev(s->s->ctx, z, M, n, eps, jc);
    if (rows) *rows = M;
    if (cols) *cols = n;
  });
}

int32_t ccsc_session_codes_fill(ccsc_session* s, double eps, int64_t* ir, double* pr,
                                int64_t capacity, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    codes_check_fill_args(eps, ir, pr, capacity);
    need_session(s);
    HIPCHK(hipSetDevice(s->s->ctx->device));
    int64_t M = 0, n = 0;
    const double* z = s->s->codes_dense(&M, &n);
    codes_check_shape(M, n);
    std::vector<int64_t> jc((size_t)n + 1, 0);
    codes_count_dev(s->s->ctx, z, M, n, eps, jc.data());
    codes_check_capacity(capacity, jc[(size_t)n]);
    codes_fill_dev(s->s->ctx, z, M, n, eps, jc.data(), ir, pr, false);
  });
}

int32_t ccsc_session_iterlog(ccsc_session* s, ccsc_iterlog* log, char* err, size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    s->s->lg.write(log);
  });
}

int32_t ccsc_session_set_profiling(ccsc_session* s, int32_t on) {
  if (!s || !s->s) return CCSC_E_STATE;
  s->s->set_profiling(on != 0);   // (2-3D: no per-kernel timers)
  return CCSC_OK;
}

int32_t ccsc_session_kernel_stats(ccsc_session* s, int32_t id, int64_t* launches,
                                  double* total_ms, double* alg_bytes_per_launch, char* err,
                                  size_t errlen) {
  return guarded(err, errlen, [&] {
    need_session(s);
    if (id < 0 || id > 4) throw Err(CCSC_E_INVALID, "kernel id out of range");
    int64_t n = 0;
    double ms = 0, bytes = 0;   // (the 2-3D learner has no per-kernel timers)
    s->s->kernel_stats(id, &n, &ms, &bytes);
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    if (alg_bytes_per_launch) *alg_bytes_per_launch = bytes;
  });
}

void ccsc_session_destroy(ccsc_session* s) {
  if (!s) return;
  if (s->s) hipSetDevice(s->s->ctx->device);
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
    const std::unique_ptr<Session> S = make_session_hs(ctx, *p, b, smooth_init, d0, z0);
    run_outer(*S, S->p.max_it, cb, user);
    S->results(out);
    S->lg.write(log);
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
    const std::unique_ptr<Session> S = make_session2d(ctx, *p, b, d0, z0);
    run_outer(*S, S->p.max_it, cb, user);
    S->results(out);
    S->lg.write(log);
  });
}

}  // extern "C"
