// Transport of a rank context (comm.cpp): the collectives of the sessions over RCCL or a
// host callback, the in-process exchange of a device list that repeats a device, and the
// abort / re-init protocol of a device-list context.
#pragma once

#include "../../include/ccsc.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <vector>

struct ccsc_ctx;

namespace ccsc {
// In-process exchange between the device threads of a multi-device context whose
// device list repeats a device (RCCL needs distinct GPUs): every rank deposits its
// buffer, the last to arrive combines them in rank order (deterministic sums) and
// releases the others.  abort() wakes every waiter when one device thread failed.
struct HostGroup {
  int n;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  bool aborted = false;
  std::vector<std::vector<double>> slot;
  std::vector<double> res;
  explicit HostGroup(int n_) : n(n_), slot(n_) {}
  int exchange(int rank, int op, double* buf, int64_t count) {
    std::unique_lock<std::mutex> lk(mu);
    if (aborted) return -1;
    const uint64_t g = gen;
    slot[rank].assign(buf, buf + count);
    if (++arrived == n) {
      if (op == CCSC_COMM_BCAST0) {
        res = slot[0];
      } else {
        res = slot[0];
        for (int r = 1; r < n; ++r)
          for (int64_t i = 0; i < count; ++i) res[i] += slot[r][i];
      }
      arrived = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g || aborted; });
      if (aborted) return -1;
    }
    // the next exchange cannot complete (and replace res) before every rank has
    // arrived at it, i.e. has copied this result
    std::copy(res.begin(), res.begin() + count, buf);
    return 0;
  }
  void abort() {
    std::lock_guard<std::mutex> lk(mu);
    aborted = true;
    cv.notify_all();
  }
};
struct HostGroupRank {
  HostGroup* g;
  int rank;
};
// the ccsc_comm_fn of a HostGroup rank (user: its HostGroupRank)
int32_t host_group_fn(void* user, int32_t op, double* buf, int64_t count);

// Failure state shared by the ranks of a multi-device context.  When one rank's
// thread fails, abort_group() marks the group aborted ONCE, wakes the
// in-process exchange and aborts every RCCL communicator, so the other ranks' blocked
// collectives return; every later collective of the group throws instead of touching
// a communicator.  `inflight` counts collectives between that check and their
// enqueue, so the abort does not free a communicator under them.  The next
// ccsc_learn on the context re-creates the communicators (reset_group).
struct CommGroup {
  std::mutex mu;
  std::atomic<bool> aborted{false};
  std::atomic<int> inflight{0};
};

// the communicators of a device-list context, rank i on devices[i], created non-blocking
void init_group_comms(std::vector<ncclComm_t>& comms, const int32_t* devices, int nd);
// one collective (CCSC_COMM_ALLREDUCE_SUM / CCSC_COMM_BCAST0) of ctx's transport over
// buf[count] on the device, enqueued on st; nothing on a one-rank context
void ctx_collective(ccsc_ctx* ctx, hipStream_t st, int op, double* buf, size_t count);
void abort_group(ccsc_ctx* ctx);
void reset_group(ccsc_ctx* ctx);
}  // namespace ccsc
