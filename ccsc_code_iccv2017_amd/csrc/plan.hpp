// Host planning unit of libccsc: everything that is decided from a ccsc_problem (or a
// solver grid) before a device is touched -- radix plans and their twiddle tables, slice
// and line geometry, problem resolution, the capability check, the shard of a rank, the
// kernels a problem runs on (its Route) and the device buffers its session allocates.
// plan.cpp makes no HIP runtime calls.
#pragma once

#include "../../include/ccsc.h"
#include "recon.hpp"

#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

namespace ccsc {

struct Err : std::runtime_error {
  int code;
  Err(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// ---- radix plans and twiddle tables ---------------------------------------------------
bool is_native_radix(int R);                          // unrolled butterfly (fft_pass_dispatch)
int64_t generic_tasks(int n, int nlines, int p);      // tasks of a generic pass of prime p
// slice kernels (kNT threads, kMaxPass passes): fewest generic passes, then fewest passes
bool plan1d(int n, int nlines, Plan1D& out);
// line kernels (kLineNT threads, kPlanSlots passes): fewest passes, then fewest generic ones
bool plan_line(int n, int nlines, Plan1D& out);
// Twiddle layout: pass s of a plan holds (R-1)*Ns entries exp(-2 pi i r k / (Ns R)) and, for
// a generic radix, its R roots.  Sets p.twoff from table offset `off`; returns the offset
// past the plan's entries.
int assign_twiddles(Plan1D& p, int off);
// the table of ntw entries (1 where no pass reads) with every plan filled in at its offsets
std::vector<cpx<double>> make_twiddles(int ntw, std::initializer_list<const Plan1D*> plans);

// ---- slice geometry (the LDS-resident transforms) ---------------------------------------
bool make_grid2d(int X, int Y, Grid2D& G, std::string& why);
// tile of the 3D learner's t-direction FFT: Tn rows of Xh complex lines (plan in Gt.py)
bool make_gridt(int Tn, int Xh, Grid2D& Gt, std::string& why);
inline std::vector<cpx<double>> make_twiddles(const Grid2D& G) {
  return make_twiddles(G.ntw, {&G.px, &G.py});
}

// ---- global line passes (recon.hip): rows over the Y T rows of a slice, y-lines per
// plane and, with_t, t-lines over the Y rows of a slice ------------------------------------
struct LinePlan {
  RowGeom rg{};
  ColGeom cy{}, ct{};
  int Y = 1, Tn = 1;
  bool with_t = false;
};
// 0, or the first grid length (X, Y, then Tn) that has no line plan
int plan_lines(int X, int Y, int Tn, bool with_t, LinePlan& lp);

// ---- problems -------------------------------------------------------------------------
void resolve_problem(ccsc_problem& p);   // defaults and validation (Appendix A of SURVEY.md)
// the consensus learners refresh the objective after every d- / z-iteration (the reference's
// verbose rules are the same for both phases)
bool objective_refresh(const ccsc_problem& p);

// Transform geometry of one slice: the (x, y) plane grid and, for the 3D
// learner, the t-direction tile (Tn = 1 otherwise).
struct Geom {
  Grid2D G{};
  Grid2D Gt{};
  int Tn = 1;
  // 2D slices past one CU's LDS (or past the slice planner): transforms as the global
  // line passes of recon.hip (lp), the elementwise stages in gslice.hip (G holds X, Y, Xh, F)
  bool gp = false;
  LinePlan lp{};
  int64_t P() const { return (int64_t)G.X * G.Y * Tn; }   // voxels per slice
  int64_t F() const { return (int64_t)G.F * Tn; }         // half-spectrum bins per slice
};

// engine capability check (separate from validity: valid reference inputs we
// do not run yet throw CCSC_E_UNSUPPORTED)
void check_supported(const ccsc_problem& p, Geom* Gout);
// (the 2-3D learner has one block of all n images, L23: its shards are runs of images)
void shard(const ccsc_problem& p, int rank, int nranks, int64_t& b0, int64_t& nb);

// ---- the route: which kernels a problem runs on ----------------------------------------
enum class ZStep {
  Line,      // k_zline, the register-line z-step of the 110 grid (zline.hip)
  Split,     // k_zsplit, every other 2D grid (zsplit.hip)
  Diag4,     // the 4D diagonal solve against the view correlations (zstep.hip)
  Planes3,   // 3D plane kernels, with k_tsolve3 when tsolve_tc > 0 (kernels3d.hip)
  Global,    // slices past one CU's LDS: global line passes + gslice.hip
  Hs23,      // the 2-3D learner's own z-phase (hs23.hip; global passes when Geom::gp)
};
enum class DFactor {
  Mfma,   // register-resident Gram + Cholesky on the matrix cores (gramchol.hip)
  Valu,   // the VALU form of the same (dstep.hip)
  Big,    // K > 192: HBM-resident Gram + Cholesky (gramchol_big.hip); 2-3D: per-rank Grams
  Wb,     // Woodbury on the ni x ni factor, ni <= 8 (k_gram_wb)
  WBig,   // ... past that (wbig.hip; K > 400, and the 2-3D learner past K = 192)
};
enum class DSolve { Tile, Sweep, Woodbury };   // dstep.hip; Woodbury: the factor's own solve

struct Route {
  int nranks = 1;
  int64_t b0 = 0, nb = 0;   // this rank's shard (blocks; 2-3D: images)
  bool dist = false;        // collectives run (several ranks, or the one-rank RCCL self-test)
  ZStep z = ZStep::Split;
  DFactor dfactor = DFactor::Mfma;
  DSolve dsolve = DSolve::Sweep;
  // right-hand sides h = A^H b past what the Gram kernels hold (K NV > 2048 or NV > 16 for
  // gramchol.hip, K NV > 8192 for gramchol_big.hip): the Gram runs with NV = 0 and the
  // per-bin GEMM of hs23.hip forms h (its Zh^H Xi, L23:289-295), same [F][NV][K] layout
  bool h_sep = false;
  // 3D: x' columns per k_tsolve3 workgroup (0: the three-kernel z-solve) and its t plan
  // (K * tsolve_tc lines)
  int tsolve_tc = 0;
  Grid2D gt2{};
  bool st2 = false;   // side stream: block j's diagonal-tile inversion beside block j+1's R2C
  bool st3 = false;   // side stream of the 110 grid: precompute R2C into Zh2, split z-phase
  // switches, read once: CCSC_WB_STAGE (0 keeps k_dsolve_wbv), CCSC_ZSPLIT2 (0 keeps the
  // z-phase on one stream); CCSC_DS_TILE=0 (the two-sweep k_dsolve) is folded into dsolve
  bool wb_stage = true, zsplit2 = true;
  // register-line z-step, tol = 0, MFMA factor, no objective evaluation after the
  // z-iterations (verbose refresh or trace_objective: it materialises the state over `yz`,
  // so the spectra would never be read and the larger buffer would buy nothing): the last
  // z-iteration of a phase also stores the code spectra it forms into `yz` (idle in that
  // route) and the next D-precompute's Gram reads them instead of a k_zhat_line pass;
  // CCSC_ZEMIT=0 keeps that pass
  bool zemit = false;
  // zemit: every local block's spectra lie in `yz` before the precompute starts, so it runs
  // as one k_gram_chol_mf launch over the rank's blocks (steps that start from a materialised
  // state keep the per-block loop); CCSC_DGROUP=0 keeps one launch per block, and dinv off
  bool dgroup = false;
  // tile d-solve on the MFMA factor: k_gram_chol_mf leaves the inverted diagonal tiles
  // itself (no k_invert_diag, no side stream) where its TM = 7 per-wave form serves the
  // problem (K NV <= 256) and the three extra LDS tiles still leave a CU to two workgroups
  bool dinv = false;
};
// consensus learners (dP, dZ, 3D, 4D) / the 2-3D learner; the problem resolved, g from
// check_supported.  route_hs throws for several ranks past K = 192.
Route route2d(const ccsc_problem& p, const Geom& g, int rank, int nranks, bool rccl_self);
Route route_hs(const ccsc_problem& p, const Geom& g, int rank, int nranks, bool rccl_self);

// ---- the memory plan: one row per device buffer of a session, in allocation order --------
// scope 0: lives as long as the session; scope n > 0: staging of the constructor, the
// scopes live one after the other.  A session allocates every buffer from its row, and
// plan_total is what ccsc_plan_bytes reports: the persistent rows plus the largest scope.
struct BufRow {
  size_t bytes = 0;
  int scope = 0;
};
size_t plan_total(const std::vector<BufRow>& rows);

namespace b2 {   // Session2D
enum {
  tw, twt, gtwr, gtwc, gtwt, gR, oacc, odz, twt2, Cg, b, Bhat, z, yz, cbuf, W, dhatw, Zh2, Bhs,
  dhs, dhws, sdens, D, yD, Usup, ssum, supp, Ch, Dh, L, h, Zh, Xbig, dhat, dtmp, sden, dnorm,
  znorm, part, pair, E, BhatT, dhatT, sdenT, d0, count
};
}
namespace bh {   // SessionHS
enum {
  tw, gtwr, gtwc, gR, b, smp, v, eD, eZ, D, yD, Dold, z, eZ2, zold, Zh, Xw, Xi, Ch, Dh, Dhold,
  L, h, sden, Usup, supp, dnorm, part, pair, stage, rm, d0, d0w, count
};
}
std::vector<BufRow> mem_plan2d(const ccsc_problem& p, const Geom& g, const Route& rt);
std::vector<BufRow> mem_plan_hs(const ccsc_problem& p, const Geom& g, const Route& rt);

}  // namespace ccsc
