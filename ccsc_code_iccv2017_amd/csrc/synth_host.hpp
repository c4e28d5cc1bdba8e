// Host-side checks the entry points over a compressed sparse column matrix share
// (synth_codes.cpp defines them; sweep_codes.cpp uses them too).
#pragma once

#include "synth_codes.hpp"
#include "host.hpp"

namespace ccsc {

extern const char* const kCscMalformed;   // the message of a raised device flag

// geometry, filters and the triple, validated in this order before any device call; out is
// required when n > 0
SynthGeom synth_check(const double* d, const int32_t* ks, int32_t C, int32_t K, const int32_t* g,
                      const int64_t* jc, const int64_t* ir, const double* pr, int64_t n,
                      int64_t nnz, const double* out);
// NULL ctx: CCSC_E_INVALID; a device-list context: CCSC_E_UNSUPPORTED, "<what> runs on a
// one-device context"
void check_ctx(const ccsc_ctx* ctx, const char* what);
// the host forms' check of the column offsets, before any launch
void check_jc_host(const int64_t* jc, int64_t n, int64_t nnz);

// the 4-byte device flag the kernels raise on a malformed column or row
struct CscFlag {
  DevBuf b;
  void reset(hipStream_t st) {
    b.alloc(sizeof(int32_t));
    HIPCHK(hipMemsetAsync(b.p, 0, sizeof(int32_t), st));
  }
  // synchronises the stream; CCSC_E_INVALID when a kernel raised the flag
  void finish(hipStream_t st) {
    int32_t h = 0;
    HIPCHK(hipMemcpyAsync(&h, b.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h != 0) throw Err(CCSC_E_INVALID, kCscMalformed);
  }
};

}  // namespace ccsc
