// Host-visible launchers of the libccsc device kernels.
#pragma once

#include "fft.hpp"

namespace ccsc {

size_t slice_smem_bytes(const Grid2D& G, size_t tsize);
size_t fused_smem_bytes(const Grid2D& G, size_t tsize, int nbl);  // + NBL*kNT accumulator bins
int pick_nb(int F);

// ---- kernels2d.hip -------------------------------------------------------
template <typename T>
hipError_t launch_r2c_embed(const T* src, int64_t src_slice, int sx, int sy, int ox, int oy,
                            cpx<T>* dst, int64_t dst_slice, int64_t count, const cpx<T>* tw,
                            const Grid2D& G, hipStream_t st);
template <typename T>
hipError_t launch_c2r_plain(const cpx<T>* src, int64_t src_slice, T* dst, int64_t dst_slice,
                            int64_t count, const cpx<T>* tw, const Grid2D& G, T scale,
                            hipStream_t st);
template <typename T>
hipError_t launch_dual_r2c(const T* D, T* yD, const T* Usup, cpx<T>* Ch, int64_t nslices,
                           const cpx<T>* tw, const Grid2D& G, int K, int r, hipStream_t st);
template <typename T>
hipError_t launch_c2r_dout(const cpx<T>* Dh, T* D, const T* yD, T* supp, T* dnorm, int nfirst,
                           int64_t nslices, const cpx<T>* tw, const Grid2D& G, int r,
                           hipStream_t st);
template <typename T>
hipError_t launch_supp_reduce(const T* supp, T* ssum, int nbl, int per_block, hipStream_t st);
template <typename T>
hipError_t launch_project(const T* ssum, T* Usup, int ngroups, int glen, T invN,
                          hipStream_t st);
template <typename T>
hipError_t launch_sden(const cpx<T>* dhat, T* sden, int F, int K, T rho, T invP,
                       hipStream_t st);
template <typename T>
hipError_t launch_objective(const T* z, const cpx<T>* dhat, const T* b, int sbx, int sby, int r,
                            T* DZ, T* part, int64_t npatch, const cpx<T>* tw, const Grid2D& G,
                            int K, int NV, hipStream_t st);
template <typename T>
hipError_t launch_zstep_diag(T* z, T* as, const cpx<T>* E, const T* sden, int64_t nslices,
                             const cpx<T>* tw, const Grid2D& G, T theta, T rho, T* znorm,
                             bool tol, bool write_z, hipStream_t st);
template <typename T>
hipError_t launch_view_corr(const cpx<T>* dhat, const cpx<T>* Bhat, cpx<T>* E, int64_t npatch,
                            int F, int K, int NV, hipStream_t st);
template <typename T>
hipError_t launch_sum_pairs(const T* part, int count, T* out, hipStream_t st);

// ---- zsplit.hip: the 2D learners' z-iteration on the pre-threshold state ----
// a = z + y per slice + w per patch: u = soft(a), y = a - u, z = u - y +
// ifft2(conj(dcorr) w); see zsplit.hip.
size_t zsplit_smem_bytes(const Grid2D& G);
template <typename T>
hipError_t launch_zsplit(const T* A, T* Ao, const T* Yz, cpx<T>* W, const cpx<T>* Bhat,
                         const cpx<T>* dcorr, const cpx<T>* dhat, const T* sden, int64_t npatch,
                         const cpx<T>* tw, const Grid2D& G, int K, T theta, int mode,
                         hipStream_t st);
// wslot: W and dcorr in bin-slot order (zline state); astate: A in state order.
template <typename T>
hipError_t launch_zmat(const T* As, T* Yz, const cpx<T>* W, const cpx<T>* dcorr, T* Zd,
                       const T* zold, T* znorm, int64_t npatch, const cpx<T>* tw, const Grid2D& G,
                       int K, T theta, hipStream_t st, bool wslot = false);
template <typename T>
hipError_t launch_zhat_split(const T* A, const cpx<T>* W, const cpx<T>* dcorr, cpx<T>* dst,
                             int64_t npatch, const cpx<T>* tw, const Grid2D& G, int K, T theta,
                             hipStream_t st, bool zline_order = false);

// ---- zline.hip: register-line z-iteration on the 110 x 110 grid -------------
// State a in "state order" and w, B^, d^, sden in "bin-slot order" (zline.hpp).
// mode 0: (z, y) materialised in Zn / Yn (natural layout); mode 2: state in A.
bool zline_grid(const Grid2D& G);
size_t zline_smem_bytes();
// tol (kZlTol* bits): Store: z of the starting iterate -> Zt (state order); Cmp: also the
// patch sums of ||z - Zt||^2, ||z||^2 -> zpart[2p..2p+1]; Form: the patch sums of
// ||z_new - z||^2, ||z_new||^2 of the produced iterate -> fpart[2p..2p+1] (needs
// dcorr == dhat); mode 3 = finalize (Store | Cmp, no advance).
// Cz (mode 2, tol 0 only): the launch also stores fft2(u - y) of the state it writes,
// unscaled (twice the spectrum), as [npatch][K][F] half spectra in bin-slot order.
template <typename T>
hipError_t launch_zline(const T* A, T* Ao, const T* Zn, const T* Yn, cpx<T>* W, const cpx<T>* Bs,
                        const cpx<T>* dcorr, const cpx<T>* dhat, const T* sden, int64_t npatch,
                        int K, T theta, T rho, int mode, hipStream_t st, int tol = 0,
                        T* Zt = nullptr, T* zpart = nullptr, T* fpart = nullptr,
                        cpx<T>* Cz = nullptr);
// tol bits of launch_zline (zline.hip): store z_cur / compare with the stored z / the
// Parseval test of the produced iterate
constexpr int kZlTolStore = 1, kZlTolCmp = 2, kZlTolForm = 4;
template <typename T>
hipError_t launch_state_to_nat_inplace(T* a, int64_t count, hipStream_t st);
// fft2(z) of the register-line state for the D-precompute (k_zhat_split's result in
// natural order, the transforms on the lanes): dst [npatch][K][F]
template <typename T>
hipError_t launch_zhat_line(const T* A, const cpx<T>* W, const cpx<T>* dcorr, cpx<T>* dst,
                            int64_t npatch, int K, T theta, hipStream_t st);
template <typename T>
hipError_t launch_to_slots(const cpx<T>* src, cpx<T>* dst, int64_t count, hipStream_t st);
template <typename T>
hipError_t launch_to_slots_real(const T* src, T* dst, hipStream_t st);
template <typename T>
hipError_t launch_state_to_nat(const T* st_, T* nat, int64_t count, hipStream_t st);

// ---- dstep.hip ------------------------------------------------------------
// Per frequency f of one block: G = A^H A + rho I (A = ni x K code spectra),
// h = A^H b, Cholesky G = L L^H; L packed lower column-major per f.
// NV views: h [F][NV][K], B [ni][NV][F] (NV = 1 in 2D).
template <typename T>
hipError_t launch_gram_chol(const cpx<T>* Zh, const cpx<T>* Bh, cpx<T>* L, cpx<T>* h, int F,
                            int K, int ni, T rho, int NV, hipStream_t st);
// The same outputs on the matrix cores (gramchol.hip): fp64 MFMA Gram and blocked
// Cholesky, K <= 112, K * NV <= 2048.
// With Wb and ds (the 110 x 110 grid only): Zh is what launch_zline's Cz received for the
// block, [ni][K][F] in bin-slot order; the kernel forms zhat = Zh / 2 + XY conj(ds_k) Wb_p
// per bin as it stages the rows (Wb [ni][F] the block's w, ds [K][F] the filter spectrum w
// was solved with, both in bin-slot order).  Bh is then B^ in bin-slot order too (one view);
// L and h stay in natural bin order.
bool gram_chol_mf_ok(int K, int NV);
bool gram_chol_mf_emit_ok(int K, int NV, int ni);   // the Wb / ds form (the block's w fits the LDS)
// nblocks > 1: one launch over nblocks consecutive blocks (Zh, Bh, Wb, L and h contiguous over
// the blocks, ds shared).  dinv (gram_chol_mf_dinv_ok; ni = 0 without Wb): the kernel leaves
// L_jj^-1 in the diagonal tiles' slots itself, what launch_invert_diag would make of its L.
bool gram_chol_mf_dinv_ok(int K, int NV, int ni);
hipError_t launch_gram_chol_mf(const cpx<double>* Zh, const cpx<double>* Bh, cpx<double>* L,
                               cpx<double>* h, int F, int K, int ni, double rho, int NV,
                               hipStream_t st, const cpx<double>* Wb = nullptr,
                               const cpx<double>* ds = nullptr, int nblocks = 1,
                               bool dinv = false);
// The same outputs for 192 < K <= 400 (gramchol_big.hip): the block's code spectra
// transposed into X ([F][ni][K], ni K F complex of workspace), the Gram on the matrix
// cores into the packed slots of L, then a left-looking Cholesky in place.
bool gram_big_ok(int K, int NV);
// X[f][r] = Z[r][f] for the R = ni K rows of a block's code spectra (frequency-major slabs)
hipError_t launch_zh_fmajor(const cpx<double>* Z, cpx<double>* X, int R, int F, hipStream_t st);
// The reference's Woodbury form past the packed K x K kernels (wbig.hip): per f the slot of
// K(K+1)/2 complex holds A_f (ni x K) and the Cholesky factor of M_f = rho I + A_f A_f^H
// (ni x ni), as k_gram_wb's layout; X is the ni K F complex frequency-major workspace.
constexpr int kWgMaxNi = 100;
bool wbig_ok(int K, int ni);
size_t wbig_workspace(int K, int ni, int F);
hipError_t launch_wbig_gram(const cpx<double>* Zh, const cpx<double>* Bh, cpx<double>* X,
                            cpx<double>* L, cpx<double>* h, int F, int K, int ni, double rho, int NV,
                            hipStream_t st);
hipError_t launch_wbig_solve(const cpx<double>* L, const cpx<double>* h, const cpx<double>* Ch,
                             cpx<double>* Dh, int nblocks, int F, int K, int ni, double rho, int NV,
                             hipStream_t st);
hipError_t launch_gram_big(const cpx<double>* Zh, const cpx<double>* Bh, cpx<double>* X,
                           cpx<double>* L, cpx<double>* h, int F, int K, int ni, double rho, int NV,
                           hipStream_t st, bool factor = true);
// the Cholesky of launch_gram_big alone, in place on packed lower Grams (factor = false above,
// e.g. after a sum of per-rank Grams)
hipError_t launch_chol_big(cpx<double>* L, int F, int K, hipStream_t st);
// x_{f,uv} = (L L^H)^{-1} (h_{f,uv} + rho * C_{f,uv}) for every (block, f, view);
// C and Dh are [blk][K][NV][F].
template <typename T>
hipError_t launch_dsolve(const cpx<T>* L, const cpx<T>* h, const cpx<T>* Ch, cpx<T>* Dh,
                         int nblocks, int F, int K, T rho, int NV, hipStream_t st);
// The same solve (NV = 1, 64 < K <= 112) on a factor whose diagonal 16 x 16 tiles hold
// L_jj^-1 (launch_invert_diag, in place after the Gram/Cholesky kernel): one workgroup
// per (block, f) holds the factor's
// 16 x 16 tiles in registers and both sweeps are tile matrix-vector products, so L is
// read once per solve instead of twice.
bool dsolve_tile_ok(int K, int NV);
hipError_t launch_invert_diag(cpx<double>* L, int F, int K, hipStream_t st);
// The inversion of one diagonal tile by one wave, shared by k_invert_diag (dstep.hip, the
// tile read back from the packed factor) and k_gram_chol_mf's fused form (gramchol.hip, the
// tile from the panel sweep's registers): the same staging rule, substitution and scaling,
// so both leave the same bits.  An LDS tile holds element (row, col) at col * kDiTS + row.
constexpr int kDiTS = 17;
constexpr int kDiTSZ = 16 * kDiTS;
__device__ __forceinline__ void wave_sync_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// staged element (r, cc) of diagonal tile J: the factor's entry on and below the diagonal
// of a real row (ld() fetches it), identity above it and on the padding rows R >= K
template <typename Ld>
__device__ __forceinline__ cpx<double> diag_tile_elem(int J, int r, int cc, int K, Ld&& ld) {
  return (r >= cc && 16 * J + r < K) ? ld() : cpx<double>{(r == cc) ? 1.0 : 0.0, 0.0};
}
// Lw staged (and visible to the wave): lane c & 15 forms column c of M = L_JJ^-1 by forward
// substitution into the wave's LDS copy Mw (each lane reads back only its own column; the
// four lanes of a column write the same values):
//   M[r][c] = (delta_rc - sum_{k<r} L[r][k] M[k][c]) / L[r][r],
// a row's 2r broadcast reads issued together; then M to the packed slots of tile J
__device__ __forceinline__ void diag_tile_invert(const cpx<double>* Lw, cpx<double>* Mw,
                                                 cpx<double>* Lf, int J, int K, int lane) {
  const int c = lane & 15;
  for (int r = 0; r < 16; ++r) {
    cpx<double> s0 = {(r == c) ? 1.0 : 0.0, 0.0}, s1 = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      if (k < r) {
        const cpx<double> p = cmul(Lw[k * kDiTS + r], Mw[k * kDiTS + c]);
        if (k & 1) s1 = csub(s1, p);
        else s0 = csub(s0, p);
      }
    }
    Mw[r * kDiTS + c] = cscale(cadd(s0, s1), 1.0 / Lw[r * kDiTS + r].x);
  }
  if (lane < 16) {
    const int C = 16 * J + c;
    for (int r = c; r < 16 && 16 * J + r < K; ++r)
      Lf[C * K - (C * (C - 1)) / 2 + 16 * J + r - C] = Mw[r * kDiTS + c];
  }
}
hipError_t launch_dsolve_tile(const cpx<double>* L, const cpx<double>* h, const cpx<double>* Ch,
                              cpx<double>* Dh, int nblocks, int F, int K, double rho, int NV,
                              hipStream_t st);
// Woodbury form for blocks of few patches (woodbury_fits): per f the slot of
// Kp = K(K+1)/2 complex holds A (ni x K, row-major) and the Cholesky factor of
// M = rho I + A A^H (ni x ni dense, row-major, zeros above the diagonal);
// (A^H A + rho I)^{-1} = (I - A^H M^{-1} A) / rho.  Same h, C, Dh layouts.
// woodbury_ok: the kernels can hold the form (lanes over k, ni <= 8 rows of A,
// A and L_M within the K(K+1)/2 slot); woodbury_fits: the AUTO choice, blocks
// of few patches (ni <= K/4) where the form saves bytes and flops.  The form is
// the reference's pinv(rho I + A A^H) (dP:230-236); its solve loses digits when
// ||A||^2 >> rho, which CCSC_DFACTOR_CHOLESKY avoids.
constexpr int kWbMaxNi = 8;
inline bool woodbury_ok(int K, int ni) {
  return ni <= kWbMaxNi && K <= 128 && ni * K + ni * ni <= K * (K + 1) / 2;
}
inline bool woodbury_fits(int K, int ni) { return woodbury_ok(K, ni) && 4 * ni <= K; }
template <typename T>
hipError_t launch_gram_wb(const cpx<T>* Zh, const cpx<T>* Bh, cpx<T>* L, cpx<T>* h, int F, int K,
                          int ni, T rho, int NV, bool staged, hipStream_t st);
// staged: the session's choice of the staged many-view solve (CCSC_WB_STAGE, read once);
// the same value must reach launch_gram_wb and launch_dsolve_wb (it sets h's layout)
template <typename T>
hipError_t launch_dsolve_wb(const cpx<T>* L, const cpx<T>* h, const cpx<T>* Ch, cpx<T>* Dh,
                            int nblocks, int F, int K, int ni, T rho, int NV, bool staged,
                            hipStream_t st);

// ---- kernels3d.hip: the 3D learner's factored transforms -------------------
// Spectra [slice][t][F2]; P2 = X*Y plane voxels.  Modes: see kernels3d.hip.
size_t tfft_smem_bytes(const Grid2D& Gt, size_t tsize);
// tc > 0: the plane spectra go to / come from the t-minor tile order of k_tsolve3
// ([slice][y][x'/tc][t][tc], ttile_bins per slice) instead of [slice][t][F2]
template <typename T>
hipError_t launch_plane_fwd(int mode, const T* a, T* b, const T* usup, int sx, int sy, int st,
                            int o, T theta, int KG, int r, cpx<T>* dst, int64_t nslices, int Tn,
                            const cpx<T>* tw, const Grid2D& G, hipStream_t stream, int tc = 0);
int64_t ttile_bins(int Tn, int Yn, int Xh, int tc);
template <typename T>
hipError_t launch_to_ttiles(const cpx<T>* src, cpx<T>* dst, int Tn, int Yn, int Xh, int tc,
                            int64_t count, hipStream_t stream);
template <typename T>
hipError_t launch_to_ttiles_real(const T* src, T* dst, int Tn, int Yn, int Xh, int tc,
                                 hipStream_t stream);
template <typename T>
hipError_t launch_tfft(const cpx<T>* src, cpx<T>* dst, int64_t nslices, int Yn, int F2, int sign,
                       const cpx<T>* tw, const Grid2D& Gt, hipStream_t stream);
// the k_tfft instantiation launch_tfft runs on tile Gt (values of CCSC_FFT_INST_*, ccsc.h)
constexpr int kTfftAll = 0, kTfftRm42 = 1, kTfftFixed38 = 2;
int tfft_instantiation(const Grid2D& Gt);
template <typename T>
hipError_t launch_plane_inv(int mode, const cpx<T>* src, T* dst, const T* yv, T* supp, T* norms,
                            int64_t nfirst, T scale, int r, int64_t nslices, int Tn,
                            const cpx<T>* tw, const Grid2D& G, hipStream_t stream, int tc = 0,
                            T* state = nullptr, T theta = 0, bool wz = true,
                            cpx<T>* nxt = nullptr);
// fused t-FFT + z-solve + inverse t-FFT over (patch, y, TC x' columns) tiles; Gt2 plans
// the t lines of K * TC columns (make_gridt with Xh = K * TC); C, Bhat, dhat, sden in the
// t-minor tile order of tile width TC; ppw patches per workgroup (the filter-spectrum
// columns of a block stay in L2 across them)
bool tsolve3_ok(int Tn, int K, int TC);
int tsolve3_nt(int Tn, int K, int TC);   // threads per k_tsolve3 workgroup
size_t tsolve3_smem_bytes(const Grid2D& Gt2, int K, int TC, size_t tsize, bool dl = false);
template <typename T>
hipError_t launch_tsolve3(cpx<T>* C, const cpx<T>* Bhat, const cpx<T>* dhat, const T* sden,
                          int64_t npatch, int K, int Yn, int Xh, int TC, T invP3,
                          const cpx<T>* tw, const Grid2D& Gt2, hipStream_t stream, int ppw);
template <typename T>
hipError_t launch_zsolve3(cpx<T>* C, const cpx<T>* Bhat, const cpx<T>* dhat, const T* sden,
                          int64_t F3, int64_t npatch, int K, T invP3, hipStream_t stream);
template <typename T>
hipError_t launch_corr_sum(const cpx<T>* Zh, const cpx<T>* dhat, cpx<T>* out, int64_t F3, int K,
                           hipStream_t stream);
template <typename T>
hipError_t launch_crop_sq(const T* Dz, const T* b, int sx, int sy, int st, int r, int rt, int X,
                          int Y, const T* z, int64_t zcount, T* part, hipStream_t stream);

// ---- gslice.hip: elementwise stages of 2D slices past one CU's LDS (global-pass path) ----
template <typename T>
hipError_t launch_gp_zdiag(cpx<T>* C, const cpx<T>* E, const T* sden, T rho, int F, int64_t count,
                           hipStream_t st);
template <typename T>
hipError_t launch_gp_views(const cpx<T>* Z, const cpx<T>* dhat, cpx<T>* out, int F, int K, int NV,
                           hipStream_t st);
template <typename T>
hipError_t launch_gp_crop(const T* R, const T* b, T* DZ, int sbx, int sby, int r, int X, int Y,
                          T scale, T* part, int count, hipStream_t st);
template <typename T>
hipError_t launch_gp_prolog(int mode, const T* a, T* b, const T* usup, int sx, int sy, int o,
                            T theta, int KG, int r, T* R, int X, int Y, int64_t count,
                            hipStream_t st, int Tn = 1, int sst = 1, int ot = 0);
template <typename T>
hipError_t launch_gp_epilog(int mode, const T* R, T* dst, const T* yv, T* supp, T* norms,
                            int64_t nfirst, T scale, int r, int X, int Y, int64_t count,
                            T* state, T theta, int wz, hipStream_t st, int Tn = 1);
// the 2-3D learner's slices past one CU's LDS: prologues (masked data prox / sparsity prox +
// dual into R) and epilogues (v or z from the C2R output + the objective's per-slice parts)
enum GpHsMode : int { kHsData = 0, kHsSparse = 1, kHsV = 2, kHsZ = 3 };
template <typename T>
hipError_t launch_gp_hs_prolog(int mode, const T* a, T* e, const T* b, const T* sm, T* R, int X,
                               int Y, int r, int sbx, int sby, T theta, int64_t count,
                               hipStream_t st);
template <typename T>
hipError_t launch_gp_hs_epilog(int mode, const T* R, T* dst, const T* b, const T* sm, T* DZ,
                               T* part, int X, int Y, int r, int sbx, int sby, T invP,
                               int64_t count, hipStream_t st);

// ---- hs23.hip: the 2-3D hyperspectral learner (L23) ----------------------------
// Spectra slice-major [slice][F]: dhat [K][W], zhat [n][K], Xi1 / Yv [n][W]; h [F][W][K].
template <typename T>
hipError_t launch_hs_synth(const cpx<T>* dhat, const cpx<T>* zhat, cpx<T>* Yv, int F, int W,
                           int K, int n, hipStream_t st);
template <typename T>
hipError_t launch_hs_analysis(const cpx<T>* dhat, const cpx<T>* Xi1, const cpx<T>* Xi2,
                              const T* sden, T rho, cpx<T>* zhat, int F, int W, int K, int n,
                              hipStream_t st);
template <typename T>
hipError_t launch_hs_corr(const cpx<T>* zhat, const cpx<T>* Xi1, cpx<T>* h, int F, int W, int K,
                          int n, hipStream_t st);
template <typename T>
hipError_t launch_hs_c2r_v(const cpx<T>* Ys, T* v, const T* b, const T* sm, T* DZ, T* part,
                           int64_t nslices, const cpx<T>* tw, const Grid2D& G, int r, int sbx,
                           int sby, hipStream_t st);
template <typename T>
hipError_t launch_hs_data_r2c(const T* v, T* e, const T* b, const T* sm, cpx<T>* Xi,
                              int64_t nslices, const cpx<T>* tw, const Grid2D& G, int r, int sbx,
                              int sby, T theta, hipStream_t st);
template <typename T>
hipError_t launch_hs_z_r2c(const T* z, T* e, cpx<T>* Xi, int64_t nslices, const cpx<T>* tw,
                           const Grid2D& G, T theta, hipStream_t st);
template <typename T>
hipError_t launch_hs_c2r_z(const cpx<T>* Zh, T* z, T* part, int64_t nslices, const cpx<T>* tw,
                           const Grid2D& G, hipStream_t st);
template <typename T>
hipError_t launch_pad_symmetric(const T* a, T* out, int sbx, int sby, int r, int X, int Y,
                                int64_t nslices, hipStream_t st);
template <typename T>
hipError_t launch_rep_filters(const T* d0, T* out, int SS, int W, int K, hipStream_t st);
template <typename T>
hipError_t launch_gather_support(const T* D, const T* y, T* supp, int KG, int r, int X, int Y,
                                 hipStream_t st);
constexpr int kNormParts = 1024;  // scratch pairs of launch_norms / launch_max
template <typename T>
hipError_t launch_norms(const T* a, const T* b, int64_t count, T* part, T* out2, hipStream_t st);
template <typename T>
hipError_t launch_max(const T* a, int64_t count, T* part, T* out, hipStream_t st);

// ---- localcn.hip: CreateImages.m:299-369 'local_cn' + ZERO_MEAN (:652-657) ---------
// n column-major [H, W] fp64 images (device pointers).  LDS path: one workgroup per
// image, shapes local_cn_ok accepts (at most 12288 pixels).
bool local_cn_ok(int H, int W);
hipError_t launch_local_cn(const double* in, double* out, int64_t n, int H, int W,
                           hipStream_t st);
// Tiled path: many workgroups per image, any H, W >= 7 with H * W < 2^31
// (local_cn_tiled_ok).  One launch serves m images over a workspace of
// local_cn_tiled_ws_bytes(m, H, W) bytes, which must stay allocated until the stream has
// run it; out may alias in.  local_cn_tiled_chunk: the images per launch, at most n, that
// keep the workspace within budget bytes (one image when a single image exceeds it).
bool local_cn_tiled_ok(int H, int W);
size_t local_cn_tiled_ws_bytes(int64_t m, int H, int W);
int64_t local_cn_tiled_chunk(int64_t n, int H, int W, size_t budget);
hipError_t launch_local_cn_tiled(const double* in, double* out, int64_t m, int H, int W,
                                 void* workspace, hipStream_t st);

// ---- imfilter.hip: imfilter(A, k, 'same', 'conv', boundary) ------------------------
// n column-major [H, W, T] fp64 arrays (device pointers, out must not overlap in) with
// one [kh, kw, kt] kernel; boundary: CCSC_PAD_*.  `taps` (device) holds the kernel as
// imfilter_pack_taps lays it out from the column-major host array k: [s][u][v], v fastest.
// imfilter_ok: extents >= 1, H * W * T < 2^31, kernel extents odd and at most
// kImfMaxExt, at most kImfMaxTaps taps.  Launches in chunks of workgroups, so any n runs.
constexpr int kImfMaxExt = 31;
constexpr int kImfMaxTaps = 4096;
bool imfilter_ok(const int dims[3], const int kdims[3]);
void imfilter_pack_taps(const double* k, const int kdims[3], double* packed);
hipError_t launch_imfilter(const double* in, double* out, int64_t n, const int dims[3],
                           const double* taps, const int kdims[3], int boundary,
                           hipStream_t st);

// ---- prep.hip: nearest-sample fill and per-plane standardisation ---------------------
// Fill: n column-major [H, W] fp64 planes (device pointers).  known: NULL (a sample is
// in != 0) or planes of the same shape (a sample is known != 0); out may be in, never
// known; idx: NULL or n * H * W int32; r: n * H * W int32 of workspace.
// nn_fill_ok: 1 <= H, W <= kFillMaxExt (a squared distance fits int32), H * W < 2^31.
constexpr int kFillMaxExt = 32768;
bool nn_fill_ok(int H, int W);
hipError_t launch_nn_fill(const double* in, const double* known, double* out, int* idx, int* r,
                          int64_t n, int H, int W, hipStream_t st);
// Standardise: `planes` runs of N contiguous values (device pointers), mean and sdev one
// value per plane, out may be in; workspace: standardize_ws_bytes(planes, N).
// standardize_ok: 2 <= N < 2^31.
bool standardize_ok(int64_t N);
int64_t standardize_ws_bytes(int64_t planes, int64_t N);
hipError_t launch_standardize(const double* in, double* out, double* mean, double* sdev,
                              int64_t planes, int64_t N, void* workspace, hipStream_t st);
hipError_t launch_unstandardize(const double* in, double* out, const double* mean,
                                const double* sdev, int64_t planes, int64_t N, hipStream_t st);

// ---- util.hip ---------------------------------------------------------------
template <typename T>
hipError_t launch_randn(T* out, int64_t count, uint64_t seed, uint64_t offset, hipStream_t st);
// Embed [psf,psf,K] (Tn == 1) or [psf,psf,psf,K] filters (column-major) into nrep
// copies of the [K][Tn][Y][X] grid at circshift(-r) positions (dP:38-39, L3:39-40).
template <typename T>
hipError_t launch_embed_filters(const T* d0, T* D, int nrep, int K, int psf, const Grid2D& G,
                                int Tn, hipStream_t st);
template <typename T>
hipError_t launch_replicate(const T* src, T* dst, int64_t n, int nrep, hipStream_t st);
template <typename T>
hipError_t launch_sub_inplace(T* a, const T* b, int64_t n, hipStream_t st);

}  // namespace ccsc
