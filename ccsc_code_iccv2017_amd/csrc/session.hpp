// What the learner sessions share (session2d.cpp, session_hs.cpp) and what the C-ABI sees of
// them (engine.cpp): the iteration log, the abstract Session, the event pool, the allocation
// of a memory plan, the slice transforms and the crop of the learned filters.
#pragma once

#include "host.hpp"

#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>

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

// A learner session as the C-ABI drives it: the consensus learners (make_session2d) and the
// 2-3D learner (make_session_hs).
struct Session {
  ccsc_ctx* ctx;
  ccsc_problem p;   // resolved by the learner's constructor
  hipStream_t st;
  HostLog lg;

  Session(ccsc_ctx* c, const ccsc_problem& pin) : ctx(c), p(pin), st(c->stream) {}
  virtual ~Session() = default;

  virtual void outer_iteration() = 0;
  virtual void results(ccsc_outputs* out) = 0;
  virtual double objective_now() = 0;   // the objective of the current iterate
  // the codes as results() copies them into z_res: device, column-major [M, n], stream idle
  virtual const double* codes_dense(int64_t* M, int64_t* n) = 0;
  // per-kernel timers (ccsc_session_kernel_stats); a learner without them leaves the zeros
  virtual void set_profiling(bool) {}
  virtual void kernel_stats(int, int64_t* launches, double* total_ms, double* alg_bytes) const {}
};
std::unique_ptr<Session> make_session2d(ccsc_ctx* ctx, const ccsc_problem& p, const double* b,
                                        const double* d0, const double* z0);
std::unique_ptr<Session> make_session_hs(ccsc_ctx* ctx, const ccsc_problem& p, const double* b,
                                         const double* smooth_init, const double* d0,
                                         const double* z0);

// HIP events handed out and given back
struct EventPool {
  std::vector<hipEvent_t> idle;
  ~EventPool() {
    for (hipEvent_t e : idle) (void)hipEventDestroy(e);
  }
  hipEvent_t get() {
    if (!idle.empty()) {
      hipEvent_t e = idle.back();
      idle.pop_back();
      return e;
    }
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    return e;
  }
  void put(hipEvent_t e) { idle.push_back(e); }
};

// buf[i] of the memory plan `rows` for every row that lives as long as the session (scope 0),
// after checking that the plan fits the free device memory (`note` ends that message);
// `after(i)` runs once row i is done
inline void alloc_plan(const std::vector<BufRow>& rows, DevBuf* buf, int count,
                       const std::string& note, const std::function<void(int)>& after = nullptr) {
  size_t freeb = 0, totalb = 0;
  HIPCHK(hipMemGetInfo(&freeb, &totalb));
  if (plan_total(rows) > freeb)
    throw Err(CCSC_E_NOMEM, "device plan needs " + std::to_string(plan_total(rows) >> 20) +
                                " MiB, " + std::to_string(freeb >> 20) + " MiB free" + note);
  for (int i = 0; i < count; ++i) {
    if (rows[i].scope == 0) buf[i].alloc(rows[i].bytes);
    if (after) after(i);
  }
}

// d_res = circshift(D1, +r)(1:psf, 1:psf(, 1:psf), :) of KG filter slices D1 [KG][P] on the
// host (dP:195-196; 4D L4:208-209: per view; 3D L3:226-227; 2-3D L23:231-232)
inline void crop_filters(const std::vector<double>& D1, double* d_res, int KG, int s, int r,
                         const Grid2D& G, int Tn, int P) {
  const int st3 = Tn > 1 ? s : 1;
  for (int k = 0; k < KG; ++k)
    for (int l = 0; l < st3; ++l)
      for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i) {
          const int x = (i - r + G.X) % G.X, y = (j - r + G.Y) % G.Y;
          const int t = Tn > 1 ? (l - r + Tn) % Tn : 0;
          d_res[i + (size_t)s * (j + (size_t)s * (l + (size_t)st3 * k))] =
              D1[(size_t)k * P + ((size_t)t * G.Y + y) * G.X + x];
        }
}

// The transforms of whole slices that both learners run around the same elementwise stages,
// in one of three forms: the fused LDS slice kernels; 3D, the plane kernels with the t-lines
// (kernels3d.hip); slices past one CU's LDS (Geom::gp), the global line passes of recon.hip
// around gslice.hip's elementwise halves over the real scratch gR.  On global passes an
// inverse consumes its input spectrum (the column pass runs in place): the inverses of Dh,
// which stays intact, run on a copy in Ch (free between the d-solve and the next dual).
struct SliceXf {
  Geom g;
  int r = 0;   // psf / 2
  bool is3 = false;
  hipStream_t st = nullptr;
  const DevBuf *tw = nullptr, *twt = nullptr, *gR = nullptr;   // of the session's memory plan
  LinePass lines;

  // dst[count][F] = R2C of the zero-padded [sx, sy, stt] sub-volumes of src placed at
  // offset o in every dimension (o = r: padarray of b, dP:23 / L3:23; o = 0: full grid)
  void fwd_embed(const double* src, int sx, int sy, int stt, int o, cpx<double>* dst,
                 int64_t count) const {
    const Grid2D& G = g.G;
    if (g.gp) {
      if (sx == G.X && sy == G.Y && stt == g.Tn && o == 0) {
        lines.r2c(src, dst, count);
        return;
      }
      HIPCHK(launch_gp_prolog<double>(0, src, nullptr, nullptr, sx, sy, o, 0.0, 1, r, gR->re(),
                                      G.X, G.Y, count, st, g.Tn, stt, g.Tn > 1 ? o : 0));
      lines.r2c(gR->re(), dst, count);
      return;
    }
    if (!is3) {
      HIPCHK(launch_r2c_embed<double>(src, (int64_t)sx * sy, sx, sy, o, o, dst, g.F(), count,
                                      tw->cx(), G, st));
      return;
    }
    HIPCHK(launch_plane_fwd<double>(0, src, nullptr, nullptr, sx, sy, stt, o, 0.0, 1, 0, dst,
                                    count, g.Tn, tw->cx(), G, st));
    HIPCHK(launch_tfft<double>(dst, dst, count, G.Y, G.F, -1, twt->cx(), g.Gt, st));
  }
  // D-step dual + R2C of (u - y) into Ch over `count` slices, KG per block (dP:107-111;
  // L23:113,117,120-121)
  void dual_r2c(const double* D, double* yD, const double* Usup, cpx<double>* Ch, int64_t count,
                int KG) const {
    const Grid2D& G = g.G;
    if (g.gp) {
      HIPCHK(launch_gp_prolog<double>(2, D, yD, Usup, 0, 0, 0, 0.0, KG, r, gR->re(), G.X, G.Y,
                                      count, st, g.Tn));
      lines.r2c(gR->re(), Ch, count);
      return;
    }
    if (!is3) {
      HIPCHK(launch_dual_r2c<double>(D, yD, Usup, Ch, count, tw->cx(), G, KG, r, st));
      return;
    }
    HIPCHK(launch_plane_fwd<double>(2, D, yD, Usup, 0, 0, 0, 0, 0.0, KG, r, Ch, count, g.Tn,
                                    tw->cx(), G, st));
    HIPCHK(launch_tfft<double>(Ch, Ch, count, G.Y, G.F, -1, twt->cx(), g.Gt, st));
  }
  // C2R of Dh -> D, the support of D + y, the d-norms of the first nfirst slices
  // (dP:112-121; L23:126)
  void c2r_dout(const cpx<double>* Dh, cpx<double>* Ch, double* D, const double* yD,
                double* supp, double* dnorm, int nfirst, int64_t count) const {
    const Grid2D& G = g.G;
    const double sc = 1.0 / (double)g.P();
    if (g.gp) {
      HIPCHK(hipMemcpyAsync(Ch, Dh, (size_t)count * g.F() * 16, hipMemcpyDeviceToDevice, st));
      lines.c2r(Ch, gR->re(), count);
      HIPCHK(launch_gp_epilog<double>(2, gR->re(), D, yD, supp, dnorm, nfirst, sc, r, G.X, G.Y,
                                      count, nullptr, 0.0, 0, st, g.Tn));
      return;
    }
    if (!is3) {
      HIPCHK(launch_c2r_dout<double>(Dh, D, yD, supp, dnorm, nfirst, count, tw->cx(), G, r, st));
      return;
    }
    HIPCHK(launch_tfft<double>(Dh, Ch, count, G.Y, G.F, +1, twt->cx(), g.Gt, st));
    HIPCHK(launch_plane_inv<double>(2, Ch, D, yD, supp, dnorm, nfirst, sc, r, count, g.Tn,
                                    tw->cx(), G, st));
  }
  // D = real(ifft2(Dh)) alone (2D slices)
  void c2r_plain(const cpx<double>* Dh, cpx<double>* Ch, double* D, int64_t count) const {
    const Grid2D& G = g.G;
    const double sc = 1.0 / (double)g.P();
    if (!g.gp) {
      HIPCHK(launch_c2r_plain<double>(Dh, g.F(), D, g.P(), count, tw->cx(), G, sc, st));
      return;
    }
    HIPCHK(hipMemcpyAsync(Ch, Dh, (size_t)count * g.F() * 16, hipMemcpyDeviceToDevice, st));
    lines.c2r(Ch, gR->re(), count);
    HIPCHK(launch_gp_epilog<double>(0, gR->re(), D, nullptr, nullptr, nullptr, 0, sc, r, G.X, G.Y,
                                    count, nullptr, 0.0, 0, st));
  }
};

}  // namespace ccsc
