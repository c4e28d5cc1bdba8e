// Host planning (plan.hpp): radix plans, twiddle tables, slice and line geometry, problem
// resolution, capability check, shard, route and memory plan.  No HIP runtime calls.
#include "plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>

namespace ccsc {

// ---------------------------------------------------------------------------
// FFT planning
// ---------------------------------------------------------------------------
static const int kRadices[] = {11, 10, 8, 7, 5, 4, 3, 2};  // fft_pass_dispatch

bool is_native_radix(int R) {
  for (int r : kRadices)
    if (r == R) return true;
  return false;
}

// Fewest passes over the native (unrolled) radices; lengths they cannot factor take
// generic passes (fft_pass_generic: here odd primes of any length, one task of kGenericQP conjugate
// output pairs per thread, inputs streamed from LDS, roots from the twiddle table) for
// their other prime factors -- primes above 11 of any size (131 of a 262 grid) and several
// of them (13 x 17) -- after the native passes: fewest generic passes, then fewest passes
// (e.g. 74 = 2 * 37, the prime-factor pfa pass).  Register budget: a native pass holds
// n/R butterflies per line (<= kMaxButterflies), a generic pass one task per thread.
int64_t generic_tasks(int n, int nlines, int p) {
  return (int64_t)nlines * (n / p) * (((p - 1) / 2 + kGenericQP - 1) / kGenericQP);
}

static bool is_prime(int p) {
  if (p < 2) return false;
  for (int d = 2; d * d <= p; ++d)
    if (p % d == 0) return false;
  return true;
}

bool plan1d(int n, int nlines, Plan1D& out) {
  if (n == 1) {
    out = Plan1D{1, 0, {0}, {0}};
    return true;
  }
  constexpr int nrad = (int)(sizeof(kRadices) / sizeof(int));
  Plan1D best{};
  best.npass = 99;
  int best_ng = 99;
  std::vector<int> nat, gen;
  // natives in kRadices order from `start`, generic primes non-decreasing
  std::function<void(int, int, bool)> dfs = [&](int rem, int start, bool allow_gen) {
    const int np = (int)(nat.size() + gen.size()), ng = (int)gen.size();
    if (rem == 1) {
      if (ng < best_ng || (ng == best_ng && np < best.npass)) {
        best_ng = ng;
        best = Plan1D{};
        best.n = n;
        best.npass = np;
        for (int i = 0; i < (int)nat.size(); ++i) best.rad[i] = nat[i];
        for (int i = 0; i < ng; ++i) best.rad[nat.size() + i] = gen[i];
      }
      return;
    }
    if (np >= kMaxPass) return;
    if (ng > best_ng || (ng == best_ng && np + 1 >= best.npass)) return;
    for (int i = start; i < nrad; ++i) {
      const int R = kRadices[i];
      if (rem % R) continue;
      if ((int64_t)(n / R) * nlines > (int64_t)maxb_for_radix(R) * kNT) continue;  // registers
      nat.push_back(R);
      dfs(rem / R, i, allow_gen);
      nat.pop_back();
    }
    if (!allow_gen) return;
    for (int R = gen.empty() ? 13 : gen.back(); R <= rem; ++R) {
      if (rem % R || !is_prime(R)) continue;
      if (generic_tasks(n, nlines, R) > kNT) continue;
      gen.push_back(R);
      dfs(rem / R, start, true);
      gen.pop_back();
    }
  };
  dfs(n, 0, false);   // native radices only (every plan of earlier rounds stays as it was)
  if (best.npass == 99) dfs(n, 0, true);
  if (best.npass == 99) return false;
  // 2 * kPfaM: the prime-factor pass with immediate roots (fft_pass_pfa)
  best.pfa = (n == 2 * kPfaM && best.npass == 2 && best.rad[0] == 2 && best.rad[1] == kPfaM &&
              pfa_slots(nlines, kPfaM, kPfaQP) <= kNT);
  out = best;
  return true;
}

// Line plan of length n for `nlines` lines per workgroup: fewest passes (<= kPlanSlots),
// then fewest generic passes.  Native radices need (n/R) * nlines butterflies within
// the register budget; any other odd factor runs as a generic pass (fft_pass_generic,
// one task per thread).  Lengths with an even factor outside {2,4,8,10} beyond the
// native set, e.g. 2^5 * 3 = 96 = 8 * 4 * 3, still plan.
bool plan_line(int n, int nlines, Plan1D& out) {
  if (n == 1) {
    out = Plan1D{};
    out.n = 1;
    return true;
  }
  Plan1D best{};
  int best_np = 99, best_ng = 99;
  std::vector<int> cur;
  std::function<void(int, int)> dfs = [&](int rem, int ng) {
    if (rem == 1) {
      const int np = (int)cur.size();
      if (np < best_np || (np == best_np && ng < best_ng)) {
        best_np = np;
        best_ng = ng;
        best = Plan1D{};
        best.n = n;
        best.npass = np;
        for (int i = 0; i < np; ++i) best.rad[i] = cur[i];
      }
      return;
    }
    if ((int)cur.size() >= kPlanSlots || (int)cur.size() + 1 > best_np) return;
    for (int R : kRadices) {
      if (rem % R) continue;
      if ((int64_t)(n / R) * nlines > (int64_t)maxb_for_radix(R) * kLineBS * kLineNT) continue;
      cur.push_back(R);
      dfs(rem / R, ng);
      cur.pop_back();
    }
    for (int R = 3; R <= rem; R += 2) {
      if (rem % R || is_native_radix(R)) continue;
      if (generic_tasks(n, nlines, R) > (int64_t)kLineGT * kLineNT) continue;
      cur.push_back(R);
      dfs(rem / R, ng + 1);
      cur.pop_back();
    }
  };
  dfs(n, 0);
  if (best_np == 99) return false;
  out = best;
  return true;
}

int assign_twiddles(Plan1D& p, int off) {
  int Ns = 1;
  for (int s = 0; s < p.npass; ++s) {
    p.twoff[s] = off;
    off += (p.rad[s] - 1) * Ns + (is_native_radix(p.rad[s]) ? 0 : p.rad[s]);
    Ns *= p.rad[s];
  }
  return off;
}

std::vector<cpx<double>> make_twiddles(int ntw, std::initializer_list<const Plan1D*> plans) {
  std::vector<cpx<double>> t(ntw, cpx<double>{1.0, 0.0});
  const long double pi = 3.141592653589793238462643383279502884L;
  for (const Plan1D* p : plans) {
    int Ns = 1;
    for (int s = 0; s < p->npass; ++s) {
      const int R = p->rad[s];
      for (int r = 1; r < R; ++r)
        for (int k = 0; k < Ns; ++k) {
          const long double a = -2.0L * pi * (long double)(r * k) / (long double)(Ns * R);
          t[p->twoff[s] + (r - 1) * Ns + k] = {(double)cosl(a), (double)sinl(a)};
        }
      if (!is_native_radix(R))
        for (int m = 0; m < R; ++m) {
          const long double a = -2.0L * pi * (long double)m / (long double)R;
          t[p->twoff[s] + (R - 1) * Ns + m] = {(double)cosl(a), (double)sinl(a)};
        }
      Ns *= R;
    }
  }
  return t;
}

bool make_grid2d(int X, int Y, Grid2D& G, std::string& why) {
  G.X = X;
  G.Y = Y;
  G.Xh = X / 2 + 1;
  // LDS row stride (units of T): >= 2*Xh, even (16-B complex alignment), and
  // 4*RS = 24 (mod 64) dwords so the column-pair lines of the x passes do not
  // alias onto the same LDS banks (measured: 6e9 conflict cycles per z-step
  // launch with RS = 2*Xh = 112).
  G.RS = 2 * G.Xh;
  while (G.RS % 16 != 6) G.RS += 2;
  G.Yp = Y + (Y & 1);
  G.F = G.Xh * Y;
  if (!plan1d(X, G.Yp / 2, G.px)) {
    why = "grid length " + std::to_string(X) +
          " has no radix plan within kMaxPass passes and the per-thread task budget";
    return false;
  }
  if (!plan1d(Y, G.Xh, G.py)) {
    why = "grid length " + std::to_string(Y) +
          " has no radix plan within kMaxPass passes and the per-thread task budget";
    return false;
  }
  // per-pass twiddle tables, x passes then y passes
  G.ntw = std::max(assign_twiddles(G.py, assign_twiddles(G.px, 0)), 1);
  const size_t lds = fused_smem_bytes(G, sizeof(double), 3);
  if (lds > 160 * 1024) {
    why = "padded slice " + std::to_string(X) + "x" + std::to_string(Y) +
          " does not fit one CU's LDS in fp64";
    return false;
  }
  if (pick_nb(G.F) < 0) {
    why = "half spectrum too large for the register-resident z-solve";
    return false;
  }
  return true;
}

bool make_gridt(int Tn, int Xh, Grid2D& Gt, std::string& why) {
  Gt = Grid2D{};
  Gt.Y = Gt.Yp = Tn;
  Gt.Xh = Xh;
  Gt.RS = 2 * Xh;  // lanes run along x' (lines): 16-B consecutive, conflict-free
  Gt.F = Xh * Tn;
  Gt.px = Plan1D{1, 0, {0}, {0}};
  if (!plan1d(Tn, Xh, Gt.py)) {
    why = "grid length " + std::to_string(Tn) + " has no radix plan for the t-direction FFT";
    return false;
  }
  Gt.ntw = std::max(assign_twiddles(Gt.py, 0), 1);
  if (tfft_smem_bytes(Gt, sizeof(double)) > 160 * 1024) {
    why = "t-direction tile does not fit one CU's LDS";
    return false;
  }
  return true;
}

// LDS budget of one line-kernel workgroup (four or more per CU)
static size_t line_lds() { return (size_t)40 * 1024; }

static bool plan_rows(int X, int rows, RowGeom& rg) {
  rg = RowGeom{};
  Grid2D& G = rg.G;
  G.X = X;
  G.Xh = X / 2 + 1;
  G.RS = 2 * G.Xh;
  while (G.RS % 16 != 6) G.RS += 2;   // column-pair lines off the same LDS banks (make_grid2d)
  rg.rows = rows;
  // the twiddle table next to the rows in LDS; lines too long for both (a 2048-point table
  // and one row pair, or the n roots of a one-pass generic plan past n = 853, are more than
  // the budget) keep the table in global memory (twg)
  for (int twg = 0; twg < 2; ++twg)
    for (int L = (rows + 1) / 2; L >= 1; --L) {
      rg.L = L;
      rg.twg = twg;
      if (!plan_line(X, L, G.px)) continue;
      rg.ntw = std::max(assign_twiddles(G.px, 0), 1);
      if (rows_smem_bytes(rg, sizeof(double)) > line_lds()) continue;
      rg.groups = (rows + 2 * L - 1) / (2 * L);
      return true;
    }
  return false;
}

static bool plan_cols(int n, int Xh, ColGeom& cg) {
  cg = ColGeom{};
  cg.n = n;
  cg.Xh = Xh;
  for (int twg = 0; twg < 2; ++twg)   // (as plan_rows)
    for (int TC = std::min(32, Xh); TC >= 1; --TC) {
      cg.TC = TC;
      cg.twg = twg;
      if (!plan_line(n, TC, cg.p)) continue;
      cg.ntw = std::max(assign_twiddles(cg.p, 0), 1);
      if (cols_smem_bytes(cg, sizeof(double)) > line_lds()) continue;
      cg.xtiles = (Xh + TC - 1) / TC;
      return true;
    }
  return false;
}

int plan_lines(int X, int Y, int Tn, bool with_t, LinePlan& lp) {
  lp = LinePlan{};
  lp.Y = Y;
  lp.Tn = Tn;
  lp.with_t = with_t;
  const int Xh = X / 2 + 1;
  if (!plan_rows(X, Y * Tn, lp.rg)) return X;
  if (!plan_cols(Y, Xh, lp.cy)) return Y;
  lp.cy.es = Xh;
  lp.cy.ninner = 1;
  lp.cy.sin = 0;
  lp.cy.sout = (int64_t)Xh * Y;
  if (!with_t) return 0;
  if (!plan_cols(Tn, Xh, lp.ct)) return Tn;
  lp.ct.es = (int64_t)Xh * Y;
  lp.ct.ninner = Y;
  lp.ct.sin = Xh;
  lp.ct.sout = (int64_t)Xh * Y * Tn;
  return 0;
}

// ---------------------------------------------------------------------------
// Problem resolution (Appendix A of SURVEY.md)
// ---------------------------------------------------------------------------
void resolve_problem(ccsc_problem& p) {
  if (p.variant < CCSC_DPAR || p.variant > CCSC_HS23) throw Err(CCSC_E_INVALID, "unknown variant");
  const bool is3 = p.variant == CCSC_L3D;
  const bool isHS = p.variant == CCSC_HS23;
  const int want_ndim = is3 ? 3 : 2;
  if (p.ndim == 0) p.ndim = want_ndim;
  if (p.ndim != want_ndim) throw Err(CCSC_E_INVALID, "ndim does not match the variant");
  for (int i = 0; i < p.ndim; ++i)
    if (p.sb[i] <= 0) throw Err(CCSC_E_INVALID, "spatial size of b must be positive");
  if (isHS) {
    // W wavelengths = kernel_size(3) = size(b, 3) (L23:6-15); they play the role of views
    if (p.views[0] <= 0)
      throw Err(CCSC_E_INVALID, "2-3D learner needs the wavelength count W (kernel_size(3)) in views[0]");
    p.views[1] = 1;
    if (!(p.lambda_prior > 0))
      throw Err(CCSC_E_INVALID, "2-3D learner needs lambda_prior > 0 (gamma_heuristic = 60*lambda/max(b), L23:36)");
  } else if (p.variant != CCSC_L4D) {
    p.views[0] = p.views[1] = 1;
  } else if (p.views[0] <= 0 || p.views[1] <= 0 || p.views[0] != p.views[1]) {
    throw Err(CCSC_E_INVALID, "4D needs equal positive view counts U == V (L4:9-10, Q9)");
  }
  if (p.n <= 0) throw Err(CCSC_E_INVALID, "n must be positive");
  if (p.K <= 0) throw Err(CCSC_E_INVALID, "K must be positive");
  if (p.psf <= 0 || (p.psf & 1) == 0) throw Err(CCSC_E_INVALID, "psf size must be odd and positive");
  if (p.max_it < 0) throw Err(CCSC_E_INVALID, "max_it must be >= 0");
  // variant constants
  int ni = 100, mid = 10, miz = 10;
  double rd = 500, rz = 50, td = 50;
  switch (p.variant) {
    case CCSC_DPAR: break;                                     // dP:11,75-76,98,150,153
    case CCSC_DZPAR: mid = 5; rd = 5000; rz = 1; td = 1; break;  // dZ:75,99,151,154
    case CCSC_L3D:
    case CCSC_L4D: {
      // the square root only defines the DEFAULT block size: a caller's own ni (a multiple
      // check below) takes any n, e.g. three blocks of two patches
      const int64_t s = (int64_t)std::llround(std::sqrt((double)p.n));
      if (p.ni <= 0 && s * s != p.n)
        throw Err(CCSC_E_INVALID, "3D/4D learners need n to be a perfect square (ni = sqrt(n), L3:11) "
                                  "unless ni is given");
      ni = (int)s;
      if (p.variant == CCSC_L3D) { rd = 5000; rz = 1; td = 1; }  // L3:109,168,175
      break;                                                      // L4:105,159,162
    }
    case CCSC_HS23:
      // one non-consensus ADMM over all images; rho_D = gamma_D(2)/gamma_D(1) = 5000
      // (L23:37,93), rho_Z = W gamma_Z(2)/gamma_Z(1) = 500 W (L23:38,311); the prox
      // thresholds follow from gamma_heuristic at run time (engine: SessionHS)
      if (p.n > INT32_MAX) throw Err(CCSC_E_INVALID, "n too large");
      ni = (int)p.n;
      rd = 5000;
      rz = 500.0 * p.views[0];
      td = 1;
      break;
  }
  if (p.ni <= 0) p.ni = ni;
  if (p.max_it_d <= 0) p.max_it_d = mid;
  if (p.max_it_z <= 0) p.max_it_z = miz;
  if (!(p.rho_d > 0)) p.rho_d = rd;
  if (!(p.rho_z > 0)) p.rho_z = rz;
  if (!(p.theta_div > 0)) p.theta_div = td;
  if (p.n % p.ni != 0)
    throw Err(CCSC_E_INVALID, "n (" + std::to_string(p.n) + ") must be a multiple of ni (" +
                                  std::to_string(p.ni) + "); the reference floors n/ni silently (Q13)");
  if (p.verbose < CCSC_VERBOSE_NONE || p.verbose > CCSC_VERBOSE_ALL)
    throw Err(CCSC_E_INVALID, "bad verbose");
  if (p.precision == CCSC_FP32)
    throw Err(CCSC_E_UNSUPPORTED, "CCSC_FP32 was never built and is deprecated (ABI 7): use CCSC_FP64");
  if (p.precision != CCSC_FP64) throw Err(CCSC_E_INVALID, "precision must be CCSC_FP64 (double, as the reference)");
  if (p.dfactor < CCSC_DFACTOR_AUTO || p.dfactor > CCSC_DFACTOR_WOODBURY)
    throw Err(CCSC_E_INVALID, "bad dfactor");
  // AUTO resolves to the form the consensus learners will run (observable through
  // ccsc_resolve): the ni x ni Woodbury factor for blocks of few patches, else K x K
  if (p.variant != CCSC_HS23 && p.dfactor == CCSC_DFACTOR_AUTO)
    p.dfactor = (woodbury_fits(p.K, p.ni) || (p.K > 400 && wbig_ok(p.K, p.ni)))
                    ? CCSC_DFACTOR_WOODBURY
                    : CCSC_DFACTOR_CHOLESKY;
  const int r = p.psf / 2;
  for (int i = 0; i < p.ndim; ++i)
    if (p.sb[i] + 2 * r < p.psf) throw Err(CCSC_E_INVALID, "grid smaller than the filter");
}

bool objective_refresh(const ccsc_problem& p) {
  if (p.variant == CCSC_DPAR) return p.verbose == CCSC_VERBOSE_BRIEF;  // dP:126,161
  if (p.variant == CCSC_L4D) return p.verbose == CCSC_VERBOSE_ALL;     // L4:135,170
  if (p.variant == CCSC_L3D) return p.verbose == CCSC_VERBOSE_ALL;     // L3:145,185
  return p.verbose != CCSC_VERBOSE_NONE;                               // dZ:127,165
}

void check_supported(const ccsc_problem& p, Geom* Gout) {
  // (right-hand sides past the Gram kernels' budget, K * views > 2048 or views > 16, are
  // formed by the per-bin GEMM of hs23.hip instead, Route::h_sep)
  if ((int64_t)p.K * p.views[0] * p.views[1] > (int64_t)1 << 20)
    throw Err(CCSC_E_UNSUPPORTED, "K * views > 2^20 filter slices");
  // K <= 192: the register-resident MFMA factor (gramchol.hip); 192 < K <= 400: the
  // HBM-resident Gram + left-looking Cholesky of gramchol_big.hip (consensus learners);
  // K > 400 (consensus) and K > 192 (2-3D): the reference's Woodbury form on the ni x ni
  // (n x n) factor (wbig.hip), for ni <= 100 and ni K + ni^2 <= K (K + 1) / 2
  if (p.K > 400 && p.variant != CCSC_HS23 &&
      !(p.dfactor == CCSC_DFACTOR_WOODBURY && wbig_ok(p.K, p.ni)))
    throw Err(CCSC_E_UNSUPPORTED, "K > 400 runs the Woodbury D-factor only, which needs ni <= 100 and "
                                  "ni K + ni^2 <= K (K + 1) / 2");
  if (p.K > 192 && p.variant == CCSC_HS23 && (p.n > INT32_MAX || !wbig_ok(p.K, (int)p.n)))
    throw Err(CCSC_E_UNSUPPORTED, "the 2-3D learner past K = 192 runs the n x n Woodbury factor "
                                  "(L23:290), which needs n <= 100 and n K + n^2 <= K (K + 1) / 2");
  if (p.dfactor == CCSC_DFACTOR_WOODBURY &&
      (p.variant == CCSC_HS23 || !(woodbury_ok(p.K, p.ni) || wbig_ok(p.K, p.ni))))
    throw Err(CCSC_E_UNSUPPORTED, "the Woodbury D-factor needs ni <= 100 and ni K + ni^2 <= K (K + 1) / 2 "
                                  "(consensus learners only)");
  const int r = p.psf / 2;
  Geom g;
  std::string why;
  const int X = (int)(p.sb[0] + 2 * r), Y = (int)(p.sb[1] + 2 * r);
  const bool is3 = p.variant == CCSC_L3D;
  const int Tn = is3 ? (int)(p.sb[2] + 2 * r) : 1;
  bool fits = make_grid2d(X, Y, g.G, why);
  // 3D: the plane kernels also need a t-tile plan (k_tfft / k_tsolve3 hold whole t-columns)
  if (fits && is3 && !make_gridt(Tn, g.G.Xh, g.Gt, why)) fits = false;
  if (!fits) {
    // every learner on any grid the reference accepts (dP:16,23-24; L3:16,23-26;
    // L23:12-26): slices past one CU's LDS (or 3D t-columns past the t-tile kernels) take
    // the global line passes
    if (plan_lines(X, Y, Tn, is3, g.lp) != 0)
      throw Err(CCSC_E_UNSUPPORTED, why + "; no global line plan either");
    g.lp.with_t = Tn > 1;   // (a one-plane 3D grid plans t-lines and runs none)
    g.gp = true;
    g.G = Grid2D{};
    g.G.X = X;
    g.G.Y = Y;
    g.G.Xh = X / 2 + 1;
    g.G.Yp = Y + (Y & 1);
    g.G.F = g.G.Xh * Y;
    g.G.ntw = 1;   // (the slice twiddle table is unused)
    g.Gt = Grid2D{};
    if ((int64_t)g.G.F * 16 > INT32_MAX / 2) throw Err(CCSC_E_UNSUPPORTED, "2D half spectrum too large");
  }
  if (is3) {
    g.Tn = Tn;
    if (g.F() > INT32_MAX / 2 || g.P() > INT32_MAX / 2)
      throw Err(CCSC_E_UNSUPPORTED, "3D half spectrum too large");
  }
  if (Gout) *Gout = g;
}

void shard(const ccsc_problem& p, int rank, int nranks, int64_t& b0, int64_t& nb) {
  if (nranks <= 0 || rank < 0 || rank >= nranks) throw Err(CCSC_E_INVALID, "bad rank/nranks");
  const int64_t N = p.variant == CCSC_HS23 ? p.n : p.n / p.ni;
  if (N < nranks) throw Err(CCSC_E_INVALID, "fewer blocks than ranks");
  const int64_t base = N / nranks, rem = N % nranks;
  nb = base + (rank < rem ? 1 : 0);
  b0 = rank * base + std::min<int64_t>(rank, rem);
}

// ---------------------------------------------------------------------------
// Routes
// ---------------------------------------------------------------------------
// an A/B switch of the environment: on unless its value starts with 0
static bool env_on(const char* name) {
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}

Route route2d(const ccsc_problem& p, const Geom& g, int rank, int nranks, bool rccl_self) {
  Route rt;
  rt.nranks = nranks;
  shard(p, rank, nranks, rt.b0, rt.nb);
  rt.dist = nranks > 1 || rccl_self;
  const int K = p.K, ni = p.ni, NV = p.views[0] * p.views[1];
  const bool is4 = p.variant == CCSC_L4D, is3 = p.variant == CCSC_L3D;
  rt.wb_stage = env_on("CCSC_WB_STAGE");
  rt.zsplit2 = env_on("CCSC_ZSPLIT2");
  // the register-line z-step serves the 110 grid (k_zsplit every other 2D grid)
  rt.z = g.gp ? ZStep::Global
         : is4 ? ZStep::Diag4
         : is3 ? ZStep::Planes3
         : zline_grid(g.G) ? ZStep::Line
                           : ZStep::Split;
  rt.st3 = rt.z == ZStep::Line;
  // (resolve_problem left no AUTO for the consensus learners)
  if (p.dfactor == CCSC_DFACTOR_WOODBURY) {
    rt.dfactor = woodbury_ok(K, ni) ? DFactor::Wb : DFactor::WBig;
    rt.dsolve = DSolve::Woodbury;
  } else {
    rt.h_sep = K > 192 ? !gram_big_ok(K, NV) : !gram_chol_mf_ok(K, NV);
    const int NVg = rt.h_sep ? 0 : NV;
    rt.dfactor = K > 192 && gram_big_ok(K, NVg) ? DFactor::Big
                 : gram_chol_mf_ok(K, NVg)      ? DFactor::Mfma
                                                : DFactor::Valu;
    // tile d-solve (one read of the factor per solve) on the MFMA factor with inverted
    // diagonal tiles; CCSC_DS_TILE=0 keeps the two-sweep k_dsolve
    if (rt.dfactor == DFactor::Mfma && dsolve_tile_ok(K, NV) && env_on("CCSC_DS_TILE"))
      rt.dsolve = DSolve::Tile;
    rt.st2 = rt.dsolve == DSolve::Tile;
    // tol = 0 fixes the last z-iteration of a phase in advance; only k_gram_chol_mf reads
    // the emitted spectra (every other factor keeps k_zhat_line); a run that evaluates the
    // objective after every z-iteration materialises the state before any precompute
    rt.zemit = rt.z == ZStep::Line && !(p.tol > 0) && rt.dfactor == DFactor::Mfma && !rt.h_sep &&
               !objective_refresh(p) && !p.trace_objective && gram_chol_mf_emit_ok(K, NV, ni) &&
               env_on("CCSC_ZEMIT");
    const bool dg = env_on("CCSC_DGROUP");
    // (blockIdx.y carries the block: a rank of more blocks keeps the per-block loop)
    rt.dgroup = rt.zemit && dg && rt.nb <= 65535;
    // (the emitted form's staging is the larger of the kernel's two)
    rt.dinv = dg && rt.dsolve == DSolve::Tile && rt.dfactor == DFactor::Mfma && !rt.h_sep &&
              gram_chol_mf_dinv_ok(K, NV, rt.zemit ? ni : 0);
    if (rt.dinv) rt.st2 = false;
  }
  if (rt.z == ZStep::Planes3) {
    // fused t-FFT + z-solve (k_tsolve3): TC x' columns per workgroup; C4 (74x74x42,
    // K = 49) measured 0.432 s per outer iteration at TC = 2, 0.456 at TC = 4 and with
    // the three-kernel form, 0.587 at TC = 1; the three-kernel form serves what k_tsolve3
    // cannot hold
    // (C4 itself runs TC = 1 on narrow workgroups when kernels3d.hip builds that form:
    // two workgroups per CU, tsolve3_nt)
    std::string why;
    const bool narrow = tsolve3_nt(g.Tn, K, 1) != kNT;
    for (int tc : narrow ? std::initializer_list<int>{1, 2, 4} : std::initializer_list<int>{2, 4, 1}) {
      Grid2D Gt2{};
      if (!tsolve3_ok(g.Tn, K, tc) || !make_gridt(g.Tn, K * tc, Gt2, why)) continue;
      if (tsolve3_smem_bytes(Gt2, K, tc, sizeof(double)) > 160 * 1024) continue;
      rt.tsolve_tc = tc;
      rt.gt2 = Gt2;
      break;
    }
  }
  return rt;
}

// The 2-3D learner's d-solve couples every image per frequency (L23:289-295).  On several
// ranks each forms the Gram of its images (gramchol_big.hip) and the sum is factored on
// every rank; past K = 192 the n x n Woodbury factor (wbig.hip) has no such split.
Route route_hs(const ccsc_problem& p, const Geom& g, int rank, int nranks, bool rccl_self) {
  Route rt;
  rt.nranks = nranks;
  rt.dist = nranks > 1 || rccl_self;
  if (rt.dist && p.K > 192)
    throw Err(CCSC_E_UNSUPPORTED, "the 2-3D learner past K = 192 (the n x n Woodbury factor "
                                  "couples every image) runs on one rank");
  shard(p, rank, nranks, rt.b0, rt.nb);
  rt.z = ZStep::Hs23;
  if (p.K > 192) {
    rt.dfactor = DFactor::WBig;
    rt.dsolve = DSolve::Woodbury;
  } else {
    rt.dfactor = rt.dist ? DFactor::Big : DFactor::Mfma;
    // 64 < K <= 112: the tile d-solve over the W wavelengths on a factor with inverted
    // diagonal tiles (dstep.hip; CCSC_DS_TILE=0 keeps the two-sweep k_dsolve)
    if (dsolve_tile_ok(p.K, p.views[0]) && env_on("CCSC_DS_TILE")) rt.dsolve = DSolve::Tile;
  }
  return rt;
}

// ---------------------------------------------------------------------------
// Memory plans
// ---------------------------------------------------------------------------
size_t plan_total(const std::vector<BufRow>& rows) {
  std::vector<size_t> live(1, 0);   // [0]: persistent; [s]: staging scope s
  for (const BufRow& r : rows) {
    if ((size_t)r.scope >= live.size()) live.resize(r.scope + 1, 0);
    live[r.scope] += r.bytes;
  }
  return live[0] + (live.size() > 1 ? *std::max_element(live.begin() + 1, live.end()) : 0);
}

std::vector<BufRow> mem_plan2d(const ccsc_problem& p, const Geom& g, const Route& rt) {
  std::vector<BufRow> row(b2::count);
  const Grid2D& G = g.G;
  const size_t R = 8, C = 16;   // bytes per real / complex
  const size_t np = (size_t)rt.nb * p.ni, nbl = (size_t)rt.nb, ni = p.ni;
  const size_t P = g.P(), F = g.F(), K = p.K, Tn = g.Tn;
  const size_t NV = (size_t)p.views[0] * p.views[1], KG = K * NV, Kp = K * (K + 1) / 2;
  const size_t s = p.psf, SS = s * s * (Tn > 1 ? s : 1);   // filter support (2r+1)^ndim
  const bool is4 = p.variant == CCSC_L4D, is3 = p.variant == CCSC_L3D, gp = g.gp;
  const bool planes3 = rt.z == ZStep::Planes3, line = rt.z == ZStep::Line,
             split = rt.z == ZStep::Split;
  auto set = [&](int i, size_t bytes) { row[i].bytes = bytes; };
  // twiddles; the 3D objective's scratch (also the global path's)
  set(b2::tw, G.ntw * C);
  if (planes3) set(b2::twt, g.Gt.ntw * C);
  if (gp) {
    set(b2::gtwr, g.lp.rg.ntw * C);
    set(b2::gtwc, g.lp.cy.ntw * C);
    if (is3) set(b2::gtwt, g.lp.ct.ntw * C);
    // a real scratch of the largest transform batch (the z-step's np K slices, the
    // D-step's nbl K NV, the precompute's ni K, the objective's views)
    set(b2::gR, std::max({np * K, nbl * KG, ni * K, np * NV}) * P * R);
  }
  if (planes3 || gp) {
    set(b2::oacc, (gp ? NV : 1) * F * C);
    set(b2::odz, (gp ? NV : 1) * P * R);
  }
  if (rt.tsolve_tc) set(b2::twt2, rt.gt2.ntw * C);
  // 4D on global-pass slices: E keeps the view correlations, the z-step spectra go to Cg
  if (is4 && gp) set(b2::Cg, np * K * F * C);
  set(b2::b, np * NV * (size_t)p.sb[0] * p.sb[1] * (is3 ? (size_t)p.sb[2] : 1) * R);
  set(b2::Bhat, np * NV * F * C);
  for (int i : {b2::z, b2::yz}) set(i, np * K * P * R);
  // the emitted half spectra (F complex per slice, 1.8% more than its P reals) share `yz`
  if (rt.zemit) set(b2::yz, std::max(np * K * P * R, np * K * F * C));
  // 2D split z-state (zsplit.hip): w per patch + the filter spectrum it was solved with;
  // with tol > 0 a buffer so z_old survives for the tol test (the 4D and 3D z-steps
  // compare per slice/plane; the register-line z-step keeps z_old in the y buffer)
  if (split && p.tol > 0) set(b2::cbuf, np * K * P * R);
  if (split || line) {
    set(b2::W, np * F * C);
    set(b2::dhatw, K * F * C);
  }
  // register-line z-step: the second precompute workspace (the R2C of block j+1 beside the
  // Gram of block j); B^, the two filter spectra and sden in bin-slot order
  if (line) {
    set(b2::Zh2, ni * K * F * C);
    set(b2::Bhs, np * F * C);
    for (int i : {b2::dhs, b2::dhws}) set(i, K * F * C);
    set(b2::sdens, F * R);
  }
  for (int i : {b2::D, b2::yD}) set(i, nbl * KG * P * R);
  for (int i : {b2::Usup, b2::ssum}) set(i, KG * SS * R);
  set(b2::supp, nbl * KG * SS * R);
  for (int i : {b2::Ch, b2::Dh}) set(i, nbl * KG * F * C);
  set(b2::L, nbl * F * Kp * C);
  set(b2::h, nbl * F * KG * C);
  set(b2::Zh, ni * K * F * C);
  // the block's code spectra transposed frequency-major (gramchol_big.hip, wbig.hip)
  if (rt.dfactor == DFactor::Big || rt.dfactor == DFactor::WBig) set(b2::Xbig, ni * K * F * C);
  for (int i : {b2::dhat, b2::dtmp}) set(i, KG * F * C);
  set(b2::sden, F * R);
  set(b2::dnorm, 2 * KG * Tn * R);
  set(b2::znorm, 2 * std::max<size_t>(np * K * Tn, 1) * R);
  set(b2::part, 2 * std::max<size_t>(np * NV, 1) * R);
  set(b2::pair, 4 * R);
  // 4D: view correlations; global passes and 3D: the z-step's spectra, for k_tsolve3 in its
  // t-minor tile order (padded to whole tiles) with B^, the filter spectrum and sden alike
  // (E keeps the size it always had, whole tiles of the wider of TC = 2 and 4, so that no
  // allocation moves; only the tile-order copies follow the chosen width)
  const size_t F3t = rt.tsolve_tc ? (size_t)ttile_bins(g.Tn, G.Y, G.Xh, rt.tsolve_tc) : 0;
  const size_t FE = planes3 ? (size_t)std::max({(int64_t)F, ttile_bins(g.Tn, G.Y, G.Xh, 4),
                                                ttile_bins(g.Tn, G.Y, G.Xh, 2)})
                            : F;
  if (is4 || is3 || gp) set(b2::E, np * K * FE * C);
  set(b2::BhatT, np * F3t * C);
  set(b2::dhatT, K * F3t * C);
  set(b2::sdenT, F3t * R);
  row[b2::d0] = BufRow{SS * KG * R, 1};   // the initial filters before they are embedded
  return row;
}

// Device state of the 2-3D learner (hs23.hip), n this rank's images:
//   real     [X,Y,W,n]  v = H z (= Dz - smoothinit), eD = d_D{1}, eZ = d_Z{1}, smp = smoothinit
//            [X,Y,W,K]  D, yD = -d_D{2} (the consensus kernels' sign), Dold
//            [X,Y,K,n]  z, eZ2 = d_Z{2}, zold
//   spectra  Zh [n][K][F] (zhat; xi_Z{2} in place), Xi [n][W][F] (xi{1}, also H zhat),
//            Ch [K][W][F] (xi_D{2}), Dh, Dhold [K][W][F] (d_hat), h [F][W][K],
//            L [F][K(K+1)/2] (Cholesky of Z'Z + rho I per bin)
std::vector<BufRow> mem_plan_hs(const ccsc_problem& p, const Geom& g, const Route& rt) {
  std::vector<BufRow> row(bh::count);
  const size_t R = 8, C = 16;
  const size_t P = g.P(), F = g.F(), K = p.K, W = p.views[0], n = (size_t)rt.nb, KG = K * W;
  const size_t SS = (size_t)p.psf * p.psf;
  auto set = [&](int i, size_t bytes) { row[i].bytes = bytes; };
  set(bh::tw, g.G.ntw * C);
  if (g.gp) {
    set(bh::gtwr, g.lp.rg.ntw * C);
    set(bh::gtwc, g.lp.cy.ntw * C);
    set(bh::gR, std::max({W * n, K * n, KG}) * P * R);   // the largest transform batch
  }
  set(bh::b, (size_t)p.sb[0] * p.sb[1] * W * n * R);
  for (int i : {bh::smp, bh::v, bh::eD, bh::eZ}) set(i, P * W * n * R);
  for (int i : {bh::D, bh::yD, bh::Dold}) set(i, P * KG * R);
  for (int i : {bh::z, bh::eZ2, bh::zold}) set(i, P * K * n * R);
  set(bh::Zh, F * K * n * C);
  // K > 192: the frequency-major workspace of the n x n Woodbury factor (wbig.hip);
  // several ranks: the same for the per-rank Gram (gramchol_big.hip)
  if (rt.dfactor != DFactor::Mfma) set(bh::Xw, F * K * n * C);
  set(bh::Xi, F * W * n * C);
  for (int i : {bh::Ch, bh::Dh, bh::Dhold}) set(i, F * KG * C);
  set(bh::L, F * (K * (K + 1) / 2) * C);
  set(bh::h, F * KG * C);
  set(bh::sden, F * R);
  for (int i : {bh::Usup, bh::supp}) set(i, KG * SS * R);
  set(bh::dnorm, 2 * KG * R);
  set(bh::part, 2 * std::max({W * n, K * n, (size_t)kNormParts}) * R);
  set(bh::pair, 12 * R);
  row[bh::stage] = BufRow{row[bh::b].bytes, 1};                        // smooth_init before padding
  row[bh::rm] = BufRow{rt.dist ? (size_t)rt.nranks * R : 0, 2};        // max(b) of every rank
  row[bh::d0] = BufRow{SS * K * R, 3};                                 // d0, and d0 over W
  row[bh::d0w] = BufRow{SS * KG * R, 3};
  return row;
}

}  // namespace ccsc
