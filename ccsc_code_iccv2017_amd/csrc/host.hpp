// Host-side helpers shared by the libccsc translation units: error type and guards of the
// C-ABI, HIP/RCCL checks, device buffers, the global line passes, the context.
#pragma once

#include "../../include/ccsc.h"
#include "comm.hpp"
#include "kernels.hpp"
#include "plan.hpp"

#include <rccl/rccl.h>

#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace ccsc {

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      throw Err(CCSC_E_HIP, std::string(#x) + " failed: " + hipGetErrorString(e_));       \
  } while (0)
#define NCCLCHK(x)                                                                        \
  do {                                                                                    \
    ncclResult_t r_ = (x);                                                                \
    if (r_ != ncclSuccess)                                                                \
      throw Err(CCSC_E_RCCL, std::string(#x) + " failed: " + ncclGetErrorString(r_));     \
  } while (0)

inline void set_err(char* err, size_t errlen, const std::string& m) {
  if (err && errlen) {
    std::snprintf(err, errlen, "%s", m.c_str());
  }
}

template <typename F>
static int32_t guarded(char* err, size_t errlen, F&& f) {
  try {
    f();
    return CCSC_OK;
  } catch (const Err& e) {
    set_err(err, errlen, e.what());
    return e.code;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, "host allocation failed");
    return CCSC_E_NOMEM;
  } catch (const std::exception& e) {
    set_err(err, errlen, e.what());
    return CCSC_E_INVALID;
  }
}

// ---------------------------------------------------------------------------
// device memory helpers
// ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void alloc(size_t b) {
    release();
    if (b == 0) return;
    HIPCHK(hipMalloc(&p, b));
    bytes = b;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename X> X* as() const { return reinterpret_cast<X*>(p); }
  double* re() const { return as<double>(); }             // the engine is fp64 only
  cpx<double>* cx() const { return as<cpx<double>>(); }
};

// a twiddle table onto the device (into b, allocated here unless a memory plan already did)
inline const cpx<double>* upload_twiddles(DevBuf& b, const std::vector<cpx<double>>& t) {
  if (!b.p) b.alloc(t.size() * sizeof(cpx<double>));
  HIPCHK(hipMemcpy(b.p, t.data(), t.size() * sizeof(cpx<double>), hipMemcpyHostToDevice));
  return b.cx();
}

// The global line passes of one grid (recon.hip) on a stream: their twiddle tables on the
// device and the unnormalised transforms of whole slices, real [count][t][y][x] <-> half
// spectra [count][t][y][x'] (rows, y-lines per plane, t-lines over the Y rows of a slice).
struct LinePass {
  LinePlan lp;
  hipStream_t st = nullptr;
  const cpx<double>*twr = nullptr, *twy = nullptr, *twt = nullptr;

  // uploads the tables into r, y (and *t, for a plan with t-lines)
  void setup(const LinePlan& plan, hipStream_t stream, DevBuf& r, DevBuf& y,
             DevBuf* t = nullptr) {
    lp = plan;
    st = stream;
    twr = upload_twiddles(r, make_twiddles(lp.rg.ntw, {&lp.rg.G.px}));
    twy = upload_twiddles(y, make_twiddles(lp.cy.ntw, {&lp.cy.p}));
    if (lp.with_t) twt = upload_twiddles(*t, make_twiddles(lp.ct.ntw, {&lp.ct.p}));
  }
  void r2c(const double* src, cpx<double>* dst, int64_t count) const {
    RowArgs<double> a{};
    a.S = dst;
    a.src = src;
    a.per_img = 1;
    HIPCHK(launch_rows<double>(kRowFwd, a, count, lp.rg, twr, st));
    HIPCHK(launch_cols<double>(dst, -1, count * lp.Tn, lp.cy, twy, st));
    if (lp.with_t) HIPCHK(launch_cols<double>(dst, -1, count * lp.Y, lp.ct, twt, st));
  }
  // the inverse column passes alone, in place (c2r's first half; ccsc_test_gfft's inverse)
  void inv_cols(cpx<double>* src, int64_t count) const {
    if (lp.with_t) HIPCHK(launch_cols<double>(src, +1, count * lp.Y, lp.ct, twt, st));
    HIPCHK(launch_cols<double>(src, +1, count * lp.Tn, lp.cy, twy, st));
  }
  // src is overwritten by the inverse column passes
  void c2r(cpx<double>* src, double* dst, int64_t count) const {
    inv_cols(src, count);
    RowArgs<double> a{};
    a.S = src;
    a.Z = dst;
    a.per_img = 1;
    HIPCHK(launch_rows<double>(kRowFinalZ, a, count, lp.rg, twr, st));
  }
};

}  // namespace ccsc

struct ccsc_ctx {
  int device = 0;
  int rank = 0;
  int nranks = 1;
  hipStream_t stream = nullptr;
  ncclComm_t comm = nullptr;       // RCCL over xGMI (production)
  ccsc_comm_fn hostfn = nullptr;   // host-staged transport (tests)
  void* hostuser = nullptr;
  std::vector<double> stage;
  // single-process multi-device context (ccsc_create_multi): one sub-context per
  // device, rank i of ndev, driven by one host thread each inside ccsc_learn
  std::vector<ccsc_ctx*> subs;
  std::unique_ptr<ccsc::HostGroup> hg;           // repeated devices: in-process exchange
  std::vector<ccsc::HostGroupRank> hg_ranks;
  std::vector<int32_t> devices;                  // the device list (ranks 0..ndev-1)
  std::shared_ptr<ccsc::CommGroup> grp;          // parent and subs of a multi-device context
  // test-only (CCSC_TEST_RCCL_SELF=1 on a one-device ccsc_create_multi): a 1-rank RCCL
  // communicator that every collective goes through, so the RCCL path (non-blocking init,
  // enqueue + wait_comm, abort / re-init) executes on a one-GPU box
  bool rccl_self = false;
};

namespace ccsc {
// codes.cpp: the dense -> compressed-sparse-column path over a device matrix a, column-major
// [M, n], on ctx's stream; both return with the stream idle.
int64_t codes_budget();   // bytes of workspace per chunk of columns: 256 MiB or CCSC_CODES_WS_MB
void codes_check_eps(double eps);                  // CCSC_E_INVALID unless eps >= 0
void codes_check_shape(int64_t M, int64_t n);      // CCSC_E_UNSUPPORTED from 2^31 rows
void codes_check_fill_args(double eps, const int64_t* ir, const double* pr, int64_t capacity);
void codes_check_capacity(int64_t capacity, int64_t nnz);
// jc[0] is the offset of the first column on entry; fills jc[1 .. n] (host)
void codes_count_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                     int64_t* jc);
// column c's kept entries go to ir / pr [jc[c], jc[c + 1]) (host arrays, or device arrays
// with out_dev); jc as codes_count_dev left it for the same matrix
void codes_fill_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                    const int64_t* jc, int64_t* ir, double* pr, bool out_dev);
}  // namespace ccsc
