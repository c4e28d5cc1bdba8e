// libccsc transport: the collectives of a rank context (RCCL over xGMI, or a host-staged
// callback), the communicators of a device-list context and its abort / re-init protocol.
#include "host.hpp"

#include <chrono>
#include <cstdlib>
#include <thread>

namespace ccsc {

int32_t host_group_fn(void* user, int32_t op, double* buf, int64_t count) {
  auto* u = static_cast<HostGroupRank*>(user);
  return u->g->exchange(u->rank, op, buf, count);
}

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
void init_group_comms(std::vector<ncclComm_t>& comms, const int32_t* devices, int nd) {
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
void ctx_collective(ccsc_ctx* ctx, hipStream_t st, int op, double* buf, size_t count) {
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

// One rank of a multi-device context failed: mark the group aborted (once, whichever
// threads fail), wake the in-process exchange, wait until no rank is inside a collective
// call, then abort every RCCL communicator so the other ranks' kernels waiting on the
// failed rank return (see CommGroup).  The wait has no time limit and needs none: the
// group's communicators are non-blocking (init_group_comms), so an enqueue returns at
// once and collective()'s poll loop leaves as soon as `aborted` is set -- a communicator
// is never aborted (freed) while another thread is inside RCCL with it, and a rank that
// enters collective() later sees `aborted` (set before the wait) before it reads `comm`.
void abort_group(ccsc_ctx* ctx) {
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
void reset_group(ccsc_ctx* ctx) {
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

}  // namespace ccsc
