/*
 * ccsc.h -- C-ABI of libccsc, the MI355X (gfx950) consensus-ADMM convolutional
 * sparse coding engine.  Drop-in boundary for the four learners of the CCSC
 * reference (paths relative to the reference repository):
 *
 *   admm_learn_conv2D_large_dParallel   2D/admm_learn_conv2D_large_dParallel.m:1-4
 *   admm_learn_conv2D_large_dzParallel  2D/admm_learn_conv2D_large_dzParallel.m:1-4
 *   admm_learn_conv3D_large             3D/admm_learn_conv3D_large.m:1-4
 *   admm_learn_conv4D_lightfield        4D/admm_learn_conv4D_lightfield.m:1-4
 *   admm_learn (2-3D hyperspectral)     2-3D/DictionaryLearning/admm_learn.m:1-4
 *
 * Each MATLAB function above becomes a thin .m wrapper over a MEX gateway that
 * calls ccsc_learn(); the Python mirror in
 * ccsc_code_iccv2017_amd/learners.py binds the same entry points via ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every host array is MATLAB column-major
 *    (first index fastest), float64, caller-owned; the library never retains a
 *    host pointer past return.  Output pointers are nullable: a NULL output is
 *    not computed/copied (z_res at the 10^4-patch config is ~97 GB).
 *  - Every function returns 0 on success or a negative CCSC_E* code; when
 *    `err` is non-NULL a NUL-terminated message (<= errlen bytes) says why.
 *    No C++ exception crosses the ABI.
 *  - Calls on one context come from one thread (MATLAB's / Python's).  The
 *    progress callback runs on that calling thread only.
 *  - Multi-GPU, one process per GPU (bench, MPI/torch jobs): rank 0 calls ccsc_get_unique_id(); the
 *    caller ships the 128 bytes to every rank (torch.distributed / MPI / file)
 *    and each rank calls ccsc_create(device, rank, nranks, uid).  Blocks of
 *    `ni` patches are sharded contiguously over ranks (ccsc_shard); the
 *    consensus mean of the reference (dP:114-121) becomes one RCCL all-reduce
 *    per d-iteration, the z-step's use of block 1's filters (dP:143) one RCCL
 *    broadcast per outer iteration.
 *  - Multi-GPU, one process (the MATLAB drop-in): ccsc_create_multi(devices, ndev)
 *    and one ccsc_learn call over the whole problem; same sharding and exchanges.
 */
#ifndef CCSC_H_
#define CCSC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCSC_ABI_VERSION 7

/* status codes */
#define CCSC_OK 0
#define CCSC_E_INVALID (-1)    /* bad argument / shape (e.g. n % ni != 0, Q13) */
#define CCSC_E_HIP (-2)        /* HIP runtime error                            */
#define CCSC_E_RCCL (-3)       /* RCCL error                                   */
#define CCSC_E_NOMEM (-4)      /* device memory plan exceeds the GPU           */
#define CCSC_E_UNSUPPORTED (-5)/* valid reference input not supported yet      */
#define CCSC_E_STATE (-6)      /* call out of order                            */

/* learner variants */
#define CCSC_DPAR 0  /* 2D dParallel   dP:1-199  */
#define CCSC_DZPAR 1 /* 2D dzParallel  dZ:1-206  */
#define CCSC_L3D 2   /* 3D             L3:1-230  */
#define CCSC_L4D 3   /* 4D light field L4:1-212  */
#define CCSC_HS23 4  /* 2-3D hyperspectral admm_learn L23:1-237 (ccsc_learn_hs23)  */

/* verbose: which objectives the reference evaluates (dP:50-60,126,161) */
#define CCSC_VERBOSE_NONE 0
#define CCSC_VERBOSE_BRIEF 1
#define CCSC_VERBOSE_ALL 2

/* arithmetic and storage precision: double only, as the reference computes (MATLAB
 * double; the 4D driver's single-precision b, learn_kernels_4D_extract_patches.m:46,
 * is widened on input).  A reduced-precision storage mode was declared in earlier
 * rounds and never built.  ABI 7 keeps its value as a deprecated name so callers built
 * against ABI <= 6 still compile; requesting it returns CCSC_E_UNSUPPORTED. */
#define CCSC_FP64 0
#define CCSC_FP32 1 /* deprecated (ABI <= 6): always CCSC_E_UNSUPPORTED */

/* form of the per-frequency D-step factor (precompute_H_hat_D, dP:221-237).
 * AUTO: Woodbury when blocks hold few patches (ni <= 8 and 4 ni <= K), else the
 * K x K Cholesky of A^H A + rho I.  The Woodbury solve (I - A^H M^-1 A) / rho,
 * M = rho I + A A^H, is the reference's own pinv form; it loses digits when
 * ||A||^2 >> rho, so CHOLESKY forces the better-conditioned K x K factor.
 * WOODBURY forces the ni x ni form (ni <= 8, ni K + ni^2 <= K (K + 1) / 2). */
#define CCSC_DFACTOR_AUTO 0
#define CCSC_DFACTOR_CHOLESKY 1
#define CCSC_DFACTOR_WOODBURY 2

typedef struct ccsc_problem {
  int32_t variant;          /* CCSC_DPAR .. CCSC_HS23                               */
  int32_t ndim;             /* spatial dims of b: 2 (2D, 4D) or 3 (3D)              */
  int64_t sb[3];            /* spatial size of b: x, y (, t for 3D)                 */
  int32_t views[2];         /* 4D: U, V (angular views; kernel_size(3:4));
                               2-3D: W, 1 (wavelengths, kernel_size(3)); else 1,1      */
  int64_t n;                /* number of patches (size(b, end))                     */
  int32_t K;                /* number of filters (kernel_size(end)); K <= 400 (2-3D:
                               K <= 192), larger K returns CCSC_E_UNSUPPORTED         */
  int32_t psf;              /* psf_s = kernel_size(1), odd                          */
  double lambda_residual;   /* objective weight only (dP:21, Q-note)                */
  double lambda_prior;      /* lambda: soft threshold = lambda / theta_div          */
  int32_t max_it;           /* outer iterations                                     */
  double tol;               /* relative-change tolerance; <= 0 disables the tests   */
  int32_t verbose;          /* CCSC_VERBOSE_*                                       */
  /* internal constants of the learners; 0 / <= 0 selects the variant default   */
  int32_t ni;               /* patches per block (dP:11 = 100, L3:11 = sqrt(n): the
                               3D/4D default needs a square n, a given ni does not) */
  int32_t max_it_d;         /* dP:75                                                */
  int32_t max_it_z;         /* dP:76                                                */
  double rho_d;             /* dP:98,111                                            */
  double rho_z;             /* dP:153                                               */
  double theta_div;         /* soft threshold = lambda_prior / theta_div (dP:150)   */
  int32_t precision;        /* CCSC_FP64 (the only value; others: CCSC_E_INVALID)   */
  int32_t trace_objective;  /* 1: evaluate the objective after every inner iter     */
  uint64_t seed;            /* device RNG seed for d0/z0 when not supplied          */
  int32_t dfactor;          /* CCSC_DFACTOR_* (0 = AUTO)                            */
} ccsc_problem;

typedef struct ccsc_outputs {
  double* d_res; /* [psf,psf,(psf | U,V),K] cropped filters of block 1 (dP:195-196) */
  double* z_res; /* this rank's codes: [X,Y,(T),K,n_local]; 4D: real part of the complex
                    [X,Y,1,1,K,n_local] (L4:164; its imaginary part is round-off, Q8)  */
  double* DZ;    /* this rank's reconstruction (dP:193 uncropped; L4:205-206 cropped) */
  double* obj_val; /* scalar final objective (L3:229, L4:211)                           */
} ccsc_outputs;

typedef struct ccsc_iterlog {
  int32_t capacity;      /* entries available per array below (>= max_it + 1)         */
  int32_t count;         /* entries written (outer iterations run + 1)                */
  double* obj_vals_d;    /* iterations.obj_vals_d (dP:63,174), nullable                 */
  double* obj_vals_z;    /* iterations.obj_vals_z (dP:64,175), nullable                 */
  double* tim_vals;      /* iterations.tim_vals, seconds, objective excluded (dP:176)   */
  /* extended trace (nullable; sized capacity * max_it_d / max_it_z)                   */
  double* trace_obj_d;   /* objective after each d-iteration (trace_objective=1)        */
  double* trace_obj_z;   /* objective after each z-iteration                            */
  double* trace_d_diff;  /* ||D1 - D1_old|| / ||D1|| per d-iteration (tol > 0)          */
  double* trace_z_diff;  /* ||z - z_old|| / ||z|| per z-iteration (tol > 0)             */
  int32_t* n_d;          /* d-iterations run per outer iteration                        */
  int32_t* n_z;          /* z-iterations run per outer iteration                        */
  int32_t* flags;        /* per outer iteration, bit 0: the 2-3D learner rolled back to
                            the previous iterate and stopped (L23:204-213); nullable      */
} ccsc_iterlog;

/* Progress callback, on the calling thread after each outer iteration. */
typedef void (*ccsc_cb)(void* user, int32_t outer_it, double obj_d, double obj_z,
                        double seconds);

typedef struct ccsc_ctx ccsc_ctx;
typedef struct ccsc_session ccsc_session;

/* ---- host-only helpers (no GPU needed) ---------------------------------- */
int32_t ccsc_abi_version(void);
/* Fill variant defaults (Appendix A) in place and validate shapes. */
int32_t ccsc_resolve(ccsc_problem* p, char* err, size_t errlen);
/* CCSC_OK if this build runs the (valid) problem on the GPU engine, else
 * CCSC_E_UNSUPPORTED with the reason (grid radices, LDS budget, K, variant). */
int32_t ccsc_supported(const ccsc_problem* p, char* err, size_t errlen);
/* Blocks [*block_begin, *block_begin + *block_count) of ni patches go to `rank`.  The 2-3D
 * learner (one block of all n images, L23) shards single images: its "blocks" are images; on
 * several ranks each passes its images' b / smooth_init / z0 with the global n in the problem,
 * and every rank holds the same filters (the Gram Z'Z and Z'xi1 are summed over the ranks).
 * The 2-3D learner with K > 192 runs on one rank only: with nranks > 1 its session and
 * ccsc_plan_bytes return CCSC_E_UNSUPPORTED. */
int32_t ccsc_shard(const ccsc_problem* p, int32_t rank, int32_t nranks,
                   int64_t* block_begin, int64_t* block_count, char* err, size_t errlen);
/* Device bytes one rank needs for this problem (CCSC_E_UNSUPPORTED where no session of
 * that rank count would run it). */
int32_t ccsc_plan_bytes(const ccsc_problem* p, int32_t rank, int32_t nranks,
                        uint64_t* bytes, char* err, size_t errlen);

/* ---- device / communicator ---------------------------------------------- */
int32_t ccsc_device_count(int32_t* count, char* err, size_t errlen);
/* RCCL unique id (128 bytes) for a multi-rank context; call on rank 0. */
int32_t ccsc_get_unique_id(uint8_t* uid128, char* err, size_t errlen);
/* nranks == 1: uid may be NULL and no communicator is created. */
ccsc_ctx* ccsc_create(int32_t device, int32_t rank, int32_t nranks, const uint8_t* uid128,
                      char* err, size_t errlen);
/* Host-transport communicator (testing / hosts without RCCL): the engine stages
 * each exchange through host memory and calls fn on the calling thread.
 * op 0 = in-place sum all-reduce, op 1 = in-place broadcast from rank 0.
 * fn returns 0 on success. */
#define CCSC_COMM_ALLREDUCE_SUM 0
#define CCSC_COMM_BCAST0 1
typedef int32_t (*ccsc_comm_fn)(void* user, int32_t op, double* buf, int64_t count);
ccsc_ctx* ccsc_create_hostcomm(int32_t device, int32_t rank, int32_t nranks, ccsc_comm_fn fn,
                               void* user, char* err, size_t errlen);
/* Single-process multi-device context: the drop-in path of one MATLAB call over a
 * node's GPUs (learn_kernels_2D_large.m:28 calls the learner once).
 * devices[0..ndev-1] become ranks 0..ndev-1 (one stream each, ncclCommInitAll over
 * xGMI; a list that repeats a device, e.g. {0, 0} on a one-GPU host, exchanges
 * through host memory instead).  ccsc_learn on this context takes the caller's
 * WHOLE problem (b and z0 over all n patches, outputs for all n), shards the blocks
 * with ccsc_shard, runs rank i in a host thread on devices[i] and calls back on the
 * calling thread only.  Sessions and the 2-3D learner need a one-device context
 * (CCSC_E_UNSUPPORTED here).  ndev == 1 is ccsc_create(devices[0], 0, 1, NULL). */
ccsc_ctx* ccsc_create_multi(const int32_t* devices, int32_t ndev, char* err, size_t errlen);
void ccsc_destroy(ccsc_ctx* ctx);
/* Ranks the context's communicator spans and its transport: RCCL reports
 * ncclCommCount (of rank 0's communicator for a multi-device context), the host
 * transport its nranks; a one-rank context reports 1 and NONE.  Evidence that a
 * multi-GPU run exchanged over RCCL across the ranks it claims (bench.py). */
#define CCSC_TRANSPORT_NONE 0
#define CCSC_TRANSPORT_RCCL 1
#define CCSC_TRANSPORT_HOST 2
int32_t ccsc_comm_ranks(ccsc_ctx* ctx, int32_t* ranks, int32_t* transport, char* err,
                        size_t errlen);

/* ---- one-shot learner: the literal drop-in for the .m functions --------- */
/* b: this rank's patches, [sb..., (U,V), n_local] column-major float64.
 * d0: [psf,psf,(psf|U,V),K] (init.d) or NULL (device RNG from p->seed).
 * z0: init.z -- dP/L3/L4: size_z of this rank's patches; dZ: size_z_crop
 *     ([X,Y,K,ni], replicated into every block, dZ:44-47); NULL = device RNG. */
int32_t ccsc_learn(ccsc_ctx* ctx, const ccsc_problem* p, const double* b, const double* d0,
                   const double* z0, ccsc_outputs* out, ccsc_iterlog* log, ccsc_cb cb,
                   void* user, char* err, size_t errlen);

/* 2-3D hyperspectral learner, the drop-in for admm_learn(b, kernel_size, lambda_residual,
 * lambda, max_it, tol, verbose, init, smooth_init) (2-3D/DictionaryLearning/admm_learn.m:1-4,
 * called by learn_hyperspectral.m:30).  p->variant = CCSC_HS23, p->views[0] = W.
 * b, smooth_init: [x, y, W, n] (smooth_init = the caller's low-pass of b,
 * learn_hyperspectral.m:16-17).  d0: [psf, psf, K], replicated over the W wavelengths
 * (L23:54-56), or NULL; z0: [X, Y, K, n] or NULL (device RNG from p->seed).
 * Outputs: d_res [psf,psf,W,K]; z_res [X,Y,K,n]; DZ [X,Y,W,n] = Dz incl. smoothinit,
 * uncropped (L23:234-235); obj_val = the last objective evaluated (L23:195 / :211).
 * Several ranks (one rank context of ccsc_create / ccsc_create_hostcomm per process, not a
 * ccsc_create_multi device list): each passes its images (ccsc_shard) with the global n in
 * the problem and z0 = NULL draws its images' part of the one global stream; K <= 192 only
 * (past it the n x n Woodbury factor couples every image: one rank). */
int32_t ccsc_learn_hs23(ccsc_ctx* ctx, const ccsc_problem* p, const double* b,
                        const double* smooth_init, const double* d0, const double* z0,
                        ccsc_outputs* out, ccsc_iterlog* log, ccsc_cb cb, void* user, char* err,
                        size_t errlen);

/* ---- stateful session (bench / warm restart) ---------------------------- */
ccsc_session* ccsc_session_create(ccsc_ctx* ctx, const ccsc_problem* p, const double* b,
                                  const double* d0, const double* z0, char* err, size_t errlen);
/* The 2-3D learner's session (arguments as ccsc_learn_hs23). */
ccsc_session* ccsc_session_create_hs23(ccsc_ctx* ctx, const ccsc_problem* p, const double* b,
                                       const double* smooth_init, const double* d0,
                                       const double* z0, char* err, size_t errlen);
/* Run `n_outer` outer iterations (tol tests honoured); returns when the device is
 * idle.  *done = 1 when the tol test ended the learning early. */
int32_t ccsc_session_step(ccsc_session* s, int32_t n_outer, int32_t* done, char* err,
                          size_t errlen);
/* Objective of the current iterate: lambda_res/2||crop(Dz) - b||^2 + lambda|z|_1. */
int32_t ccsc_session_objective(ccsc_session* s, double* obj, char* err, size_t errlen);
int32_t ccsc_session_results(ccsc_session* s, ccsc_outputs* out, char* err, size_t errlen);
int32_t ccsc_session_iterlog(ccsc_session* s, ccsc_iterlog* log, char* err, size_t errlen);
/* The codes as a compressed sparse column matrix (MATLAB's sparse, scipy.sparse.csc_matrix)
 * instead of the dense z_res: one column per local patch (2-3D: per local image), n_local
 * columns of M = X Y (T) K rows, the row index being the 0-based column-major index into
 * that patch's [X, Y, (T), K] slice of z_res (4D: of the real [X, Y, 1, 1, K] slice).  An entry
 * is kept iff !(|z| <= eps): strictly above the threshold, and a NaN is kept.  eps >= 0
 * (+inf keeps only NaNs, 0 keeps every nonzero); a negative or NaN eps is CCSC_E_INVALID,
 * M >= 2^31 CCSC_E_UNSUPPORTED.  Two steps: the count call fills jc[0 .. n_local] (the
 * caller learns nnz = jc[n_local]; rows / cols, nullable, receive M and n_local), the fill
 * call takes caller-allocated ir[capacity], pr[capacity]: row indices strictly ascending
 * inside a column, pr the dense values' bits unchanged, everything 0-based.  A capacity below
 * nnz is CCSC_E_INVALID with the needed count in the message and nothing written.  Both
 * materialise the codes as the results call with z_res set does and leave the session in
 * the state that call leaves it in; the dense array never exists on the host (the triple is
 * formed on the device chunk by chunk, see the sparsify entry points below).  The result is
 * bitwise reproducible and does not depend on the chunking or on the other patches. */
int32_t ccsc_session_codes_count(ccsc_session* s, double eps, int64_t* jc, int64_t* rows,
                                 int64_t* cols, char* err, size_t errlen);
int32_t ccsc_session_codes_fill(ccsc_session* s, double eps, int64_t* ir, double* pr,
                                int64_t capacity, char* err, size_t errlen);
/* Per-kernel timing with HIP events on the engine stream.  kernel ids: 0 = fused
 * z-step, 1 = gram+cholesky, 2 = d-solve, 3 = dual+R2C, 4 = C2R+support.  Returns
 * launches, total milliseconds and the algorithmic bytes of ONE launch.  Kernel 1 launches
 * once per block or, where the precompute is grouped, once per outer iteration over the
 * rank's blocks: its bytes are those of one block times the mean number of blocks per launch
 * timed so far, so launches x bytes is what the timed launches moved. */
int32_t ccsc_session_set_profiling(ccsc_session* s, int32_t on);
int32_t ccsc_session_kernel_stats(ccsc_session* s, int32_t kernel_id, int64_t* launches,
                                  double* total_ms, double* alg_bytes_per_launch, char* err,
                                  size_t errlen);
void ccsc_session_destroy(ccsc_session* s);

/* ---- reconstruction solvers ------------------------
 * Sparse-coding reconstruction of images from learned filters; each variant is the
 * drop-in for one reference function (paths relative to the reference root):
 *   CCSC_SOLVE_INPAINT2D  [z, res] = admm_solve_conv2D_weighted_sampling(b, kernels, mask,
 *                         lambda_residual, lambda_prior, smooth_init, max_it, tol, x_orig,
 *                         verbose)          2D/Inpainting/admm_solve_conv2D_weighted_sampling.m:1-4
 *   CCSC_SOLVE_POISSON2D  [z, res] = admm_solve_conv_poisson(b, kmat, mask, lambda_residual,
 *                         lambda_prior, max_it, tol, x_orig, verbose)
 *                                           2D/Poisson_deconv/admm_solve_conv_poisson.m:1-2
 *   CCSC_SOLVE_MULTICH    [z, res] = admm_solve_conv23D_weighted_sampling(b, kmat, mask,
 *                         lambda_residual, lambda_prior, max_it, tol, ~, verbose, smooth_init)
 *                                           2-3D/Demosaicing/admm_solve_conv23D_weighted_sampling.m:1-2
 *                         and admm_solve_conv_weighted_sampling_lf (the same text)
 *                                           4D/ViewSynthesis/admm_solve_conv_weighted_sampling_lf.m:1-2
 *   CCSC_SOLVE_VIDEO3D    [z, res] = admm_solve_video_weighted_sampling(b, kmat, mask,
 *                         lambda_residual, lambda_prior, max_it, tol, verbose, psf, smooth_init)
 *                                           3D/Deblurring/admm_solve_video_weighted_sampling.m:1-2
 * One call solves n independent images of one shape (the reference's callers loop over
 * images, e.g. reconstruct_poisson_noise.m:24); each image keeps its own gamma
 * heuristic (c * lambda_prior / max(b(:))) and its own tol test.  Arrays are
 * column-major float64 with the image index last. */
#define CCSC_SOLVE_INPAINT2D 0
#define CCSC_SOLVE_POISSON2D 1
#define CCSC_SOLVE_MULTICH 2
#define CCSC_SOLVE_VIDEO3D 3

typedef struct ccsc_solve_problem {
  int32_t variant;          /* CCSC_SOLVE_*                                                */
  int64_t sb[3];            /* image extent x, y (, t for VIDEO3D)                         */
  int32_t nch;              /* MULTICH: channels W = size(b, 3) (wavelengths / views); else 1 */
  int64_t n;                /* images solved by this call                                  */
  int32_t K;                /* learned filters (kernel_size(end)), without the dirac that
                               POISSON2D appends and VIDEO3D prepends                      */
  int32_t ksize[3];         /* filter extent x, y (, t); odd                                 */
  int32_t psf_size[3];      /* VIDEO3D: extent of the blur psf                             */
  double lambda_residual;
  double lambda_prior;
  int32_t max_it;
  double tol;               /* relative change ||z - z_old|| / ||z||; <= 0: never stops early */
  int32_t verbose;          /* CCSC_VERBOSE_*: BRIEF/ALL fill the objective / PSNR trace   */
} ccsc_solve_problem;

typedef struct ccsc_solve_inputs {
  const double* b;           /* [sx, sy, (st | W), n]                                       */
  const double* kernels;     /* INPAINT2D/POISSON2D [k,k,K]; MULTICH [k,k,W,K]; VIDEO3D [k,k,k,K] */
  const double* mask;        /* same shape as b                                              */
  const double* smooth_init; /* same shape as b; NULL for POISSON2D (it has none)            */
  const double* psf;         /* VIDEO3D: blur kernel [psf_size]; else NULL                   */
  const double* x_orig;      /* INPAINT2D/POISSON2D: [sx, sy, n] for the PSNR trace; nullable */
} ccsc_solve_inputs;

typedef struct ccsc_solve_outputs {
  double* z;    /* [X, Y, (T), K', n] codes on the padded grid (K' includes the dirac:
                   POISSON2D last, VIDEO3D first; MULTICH: X, Y = sx, sy); nullable       */
  double* res;  /* INPAINT2D/POISSON2D [sx, sy, n]; MULTICH [sx, sy, W, n];
                   VIDEO3D [sx, sy, st, n]; nullable                                       */
} ccsc_solve_outputs;

typedef struct ccsc_solvelog {
  int32_t capacity;   /* entries per image in the arrays below (>= max_it + 1)            */
  int32_t* iters;     /* [n] ADMM iterations run per image (tol may stop an image early)  */
  double* obj;        /* [n][capacity] objective of iterate 0..iters (verbose BRIEF/ALL)  */
  double* psnr;       /* [n][capacity] PSNR vs x_orig (INPAINT2D/POISSON2D)               */
  double* diff;       /* [n][capacity] ||z - z_old|| / ||z|| (0 for iterate 0)            */
  double* seconds;    /* [1] device time of the ADMM iterations (setup and output excluded) */
} ccsc_solvelog;

/* CCSC_OK if this build runs the (valid) problem, else CCSC_E_INVALID /
 * CCSC_E_UNSUPPORTED with the reason (e.g. a grid length with no FFT plan). */
int32_t ccsc_solve_supported(const ccsc_solve_problem* p, char* err, size_t errlen);
int32_t ccsc_solve(ccsc_ctx* ctx, const ccsc_solve_problem* p, const ccsc_solve_inputs* in,
                   ccsc_solve_outputs* out, ccsc_solvelog* log, char* err, size_t errlen);

/* ---- input preprocessing ----------------------------
 * Local contrast normalisation of the learners' input images: the 'local_cn' and
 * ZERO_MEAN branches of image_helpers/CreateImages.m:299-369, :652-657 (13x13 Gaussian,
 * sigma 3*1.591, reflection padding of image_helpers/rconv2.m:22-58, std floored at
 * its median, single-precision result), for images and frames of any size:
 * H, W >= 7 and H * W < 2^31, anything else is CCSC_E_UNSUPPORTED with the reason.
 * in/out: n column-major [H, W] float64 images (out = double(single(...)), may alias in).
 * ccsc_local_cn takes host arrays; ccsc_local_cn_dev device arrays on the context's
 * device (e.g. torch tensors), ordered on the context's stream, synchronised on return.
 * Two GPU paths, chosen by shape: images of at most 12288 pixels (110 x 110) whose
 * padded (H+12) x (W+12) image fits the LDS run one workgroup per image; others run tiled, many
 * workgroups per image (32 x 32 tiles, radix-select median over global memory).  Both
 * share the 13x13 accumulate, so local mean, local std and the median floor are the same
 * bits on either path; the results can differ by the single-precision rounding of the
 * mean.  Each image's result is bitwise reproducible and independent of the batch.
 * The tiled path allocates its workspace inside the call (16 B per pixel + 48 KiB per
 * image) and frees it before returning; images go in chunks so that it stays within
 * 256 MiB whatever n is (a single image larger than that still gets its own).
 * Environment, read per call: CCSC_CN_TILED=1 forces the tiled path on any shape;
 * CCSC_CN_WS_MB=<MiB> lowers the workspace budget (0: one image per chunk). */
int32_t ccsc_local_cn(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t H,
                      int32_t W, char* err, size_t errlen);
int32_t ccsc_local_cn_dev(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t H,
                          int32_t W, char* err, size_t errlen);

/* N-dimensional image filtering: imfilter(A, k, 'same', 'conv', <boundary>), the call
 * with which the reference's drivers compute smooth_init (the low-pass image that
 * ccsc_learn_hs23 and ccsc_solve_inputs.smooth_init take) and blur their data:
 *   k = fspecial('gaussian', [13 13], 3*1.591); imfilter(b, k, 'same', 'conv', 'symmetric')
 *     2-3D/DictionaryLearning/learn_hyperspectral.m:16-17
 *     2-3D/Demosaicing/reconstruct_subsampling_hyperspectral.m:54-55
 *     4D/ViewSynthesis/reconstruct_subsampling_lightfield.m:58-59
 *     3D/Deblurring/reconstruct_subsampling_video.m:50-51 (15x15), :40 (its 3x3x3 psf)
 *   image_helpers/CreateImages.m:388-399 'box_cn' (imfilter 'replicate'),
 *   :371-387 'laplacian_cn' (conv2 'same': zero padding).
 * in/out: n column-major float64 arrays of nd = 1, 2 or 3 dimensions dims = [H, W, T];
 * k: one column-major float64 kernel of the same nd, kdims = [kh, kw, kt]; unused trailing
 * entries of dims and kdims are 1 (a 2D kernel over the planes of a 3D array is kt = 1).
 * With the zero-based centre c = (extent - 1) / 2,
 *   out[i, j, t] = sum_{u,v,s} k[u, v, s] * A_pad[i + c1 - u, j + c2 - v, t + c3 - s]
 * (convolution, not correlation), accumulated s outer, v middle, u inner, ascending, one
 * fma per tap from 0: bitwise reproducible and independent of the batch.  boundary says
 * what A_pad reads outside A. */
#define CCSC_PAD_SYMMETRIC 0 /* mirror, edge sample repeated: m = i mod 2N, m < N ? m : 2N-1-m
                                (any half-width, any extent >= 1)                         */
#define CCSC_PAD_REPLICATE 1 /* clamp the index                                          */
#define CCSC_PAD_ZERO 2      /* out-of-range samples are 0                               */
/* Limits: kernel extents odd, 1..31 each, at most 4096 taps; image extents >= 1 with
 * H * W * T < 2^31: an even or larger extent, more taps or more pixels are
 * CCSC_E_UNSUPPORTED with the reason.  NULL pointers, n < 0, nd outside 1..3, an extent
 * < 1, a trailing extent that is not 1, an unknown boundary and out == in (a stencil
 * cannot run in place) are CCSC_E_INVALID.  Both entry points validate before they touch
 * the device; n == 0 is CCSC_OK and launches nothing.
 * ccsc_imfilter takes host arrays and stages them in chunks of images of at most 256 MiB
 * per buffer (a single larger image still gets its own); ccsc_imfilter_dev takes in/out
 * on the context's device (e.g. torch tensors), ordered on the context's stream,
 * synchronised on return.  k is a host array for both. */
int32_t ccsc_imfilter(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t nd,
                      const int32_t dims[3], const double* k, const int32_t kdims[3],
                      int32_t boundary, char* err, size_t errlen);
int32_t ccsc_imfilter_dev(ccsc_ctx* ctx, const double* in, double* out, int64_t n, int32_t nd,
                          const int32_t dims[3], const double* k, const int32_t kdims[3],
                          int32_t boundary, char* err, size_t errlen);

/* Nearest-sample fill of the unsampled pixels, per wavelength plane
 *   [~, idx] = bwdist(a ~= 0); a(a == 0) = a(idx(a == 0));
 *     2-3D/Demosaicing/reconstruct_subsampling_hyperspectral.m:43-51
 * (the filled cube is what that driver filters smooth_init from, :54-55).
 * in/out: n column-major [H, W] float64 planes; known: NULL or the same shape; idx: NULL or
 * n * H * W int32.  Per plane, independent of the other planes: pixel q is a sample iff
 * known[q] != 0, or in[q] != 0 where known is NULL (the reference's a ~= 0: a NaN is a
 * sample, -0.0 is not).  A sample keeps out[q] = in[q], idx[q] = q, the zero-based
 * column-major index i + H * j.  Any other pixel gets out[q] = in[s], idx[q] = s, with s the
 * sample that minimises the exact squared Euclidean distance (i - i')^2 + (j - j')^2,
 * compared in integer arithmetic; among equally near samples the smallest column-major
 * index wins (the smallest j', then the smallest i').  bwdist does not document which of
 * several nearest samples it reports, so ties cannot be pinned to MATLAB: parity here means
 * exact distances.  A plane without a sample has out = in and idx = -1 everywhere (the
 * reference would index with 0 and stop).  out may be in: only non-samples are written and
 * only samples are read.  Results are bitwise reproducible, independent of the batch and
 * equal between the two entry points.
 * Limits: 1 <= H, W <= 32768, so that a squared distance fits int32 and H * W < 2^31; a
 * larger extent is CCSC_E_UNSUPPORTED with the reason.  NULL in or out, n < 0, an extent < 1 and
 * known == out are CCSC_E_INVALID.  Both entry points validate before they touch the
 * device; n == 0 is CCSC_OK and launches nothing.  ccsc_nn_fill takes host arrays and stages
 * them in chunks of planes of at most 256 MiB per buffer; ccsc_nn_fill_dev takes arrays on
 * the context's device, is ordered on the context's stream and synchronised on return.  The
 * int32 workspace of one entry per pixel of a chunk is allocated inside the call and freed
 * before it returns. */
int32_t ccsc_nn_fill(ccsc_ctx* ctx, const double* in, const double* known, double* out,
                     int32_t* idx, int64_t n, int32_t H, int32_t W, char* err, size_t errlen);
int32_t ccsc_nn_fill_dev(ccsc_ctx* ctx, const double* in, const double* known, double* out,
                         int32_t* idx, int64_t n, int32_t H, int32_t W, char* err,
                         size_t errlen);

/* Per-plane standardisation and its inverse after the solve ("all data should be similarly
 * normalized"):
 *   veam = mean(v, 2); vstd = std(v, 0, 2); nb = (v - veam) ./ vstd; ... sig_rec .* vssd + vemm
 *     3D/Deblurring/reconstruct_subsampling_video.m:42-47, 63-68          per frame
 *     4D/ViewSynthesis/reconstruct_subsampling_lightfield.m:36-41, 67-72  per view
 *     2D/Poisson_deconv/reconstruct_poisson_noise.m:49-54, 98-102         per image (commented)
 * in/out: `planes` runs of N contiguous float64 values (a frame, a view or an image in
 * MATLAB order); mean, sdev: one value per plane; out may be in.  As MATLAB's two-pass std:
 *   mean_p = (sum x) / N,  sdev_p = sqrt(sum (x - mean_p)^2 / (N - 1)) with the rounded mean_p,
 *   standardize:    out = (x - mean_p) / sdev_p   (a true division)
 *   unstandardize:  out = in * sdev_p + mean_p    (a multiply, then an add: two roundings)
 * A plane of zero spread divides by zero as the reference does.  Both sums are taken with
 * one fixed tree whose shape depends on N alone (no atomics), so results are bitwise
 * reproducible, independent of `planes` and equal between the entry points.
 * Limits: 2 <= N < 2^31; N < 2, planes < 0 and NULL pointers are CCSC_E_INVALID, a larger N
 * is CCSC_E_UNSUPPORTED; planes == 0 is CCSC_OK and launches nothing.  The host entries
 * stage planes in chunks of at most 256 MiB; the _dev entries take every array on the
 * context's device, are ordered on the context's stream and synchronised on return. */
int32_t ccsc_standardize(ccsc_ctx* ctx, const double* in, double* out, double* mean, double* sdev,
                         int64_t planes, int64_t N, char* err, size_t errlen);
int32_t ccsc_standardize_dev(ccsc_ctx* ctx, const double* in, double* out, double* mean,
                             double* sdev, int64_t planes, int64_t N, char* err, size_t errlen);
int32_t ccsc_unstandardize(ccsc_ctx* ctx, const double* in, double* out, const double* mean,
                           const double* sdev, int64_t planes, int64_t N, char* err,
                           size_t errlen);
int32_t ccsc_unstandardize_dev(ccsc_ctx* ctx, const double* in, double* out, const double* mean,
                               const double* sdev, int64_t planes, int64_t N, char* err,
                               size_t errlen);

/* Threshold-and-compact of any dense matrix into compressed sparse columns: a is column-major
 * [M, n] float64; entry (i, j) is kept iff !(|a| <= eps) (see the session form above for
 * eps, the layout and the two-step protocol: jc[n + 1], then ir / pr [capacity], int64 / int64 /
 * double, 0-based, rows ascending inside a column, values bit for bit).  The host forms take
 * host arrays and stage the matrix in chunks of columns; the _dev forms take a, jc, ir and pr
 * on the context's device (e.g. torch tensors).  All run on the context's stream,
 * synchronise on return and take a one-device context only.  They validate eps, the outputs
 * and the shape before they touch the device; M == 0 or n == 0 gives an empty matrix.
 * Per tile of 2048 rows of a column a count pass finds the kept entries with wave ballots,
 * a 64-bit exclusive scan over the tiles places them, and a scatter gives each lane its slot
 * from the ballot's lower lanes: index order with no sort and no atomics, so the result
 * is bitwise reproducible, the same for every chunking and for a column taken alone.  The
 * workspace (8 B per tile, and for host outputs 16 B per kept entry) is allocated inside the
 * call and freed before return; columns go in chunks that keep it within 256 MiB whatever
 * n is (a single column that needs more gets its own).  Environment, read per call:
 * CCSC_CODES_WS_MB=<MiB> lowers that budget (0: one column per chunk). */
int32_t ccsc_sparsify_count(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                            int64_t* jc, char* err, size_t errlen);
int32_t ccsc_sparsify_fill(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                           int64_t* ir, double* pr, int64_t capacity, char* err, size_t errlen);
int32_t ccsc_sparsify_count_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                                int64_t* jc, char* err, size_t errlen);
int32_t ccsc_sparsify_fill_dev(ccsc_ctx* ctx, const double* a, int64_t M, int64_t n, double eps,
                               int64_t* ir, double* pr, int64_t capacity, char* err,
                               size_t errlen);
/* Host only: the index arithmetic of the kernels above, for checks with offsets past 2^32
 * that no test-sized matrix reaches.  For lane `lane` of step `step` of wave `wave` in tile
 * `tile` of a chunk of columns of M rows: out4 = {column, row, element index column * M + row,
 * slot tile_off + before + prefix}.  wave 0..3, step 0..7, lane and prefix 0..63. */
int32_t ccsc_test_codes_index(int64_t M, int64_t tile, int32_t wave, int32_t step, int32_t lane,
                              int64_t tile_off, int64_t before, int32_t prefix, int64_t* out4,
                              char* err, size_t errlen);

/* Synthesis from sparse codes: the reconstructions sum_k d_k (*) z_k of the columns of a
 * compressed sparse column matrix (the triple of ccsc_session_codes_* / ccsc_sparsify_*), as a
 * direct sparse convolution on the GPU.
 *   g  = (X, Y, T), T = 1 for two spatial dimensions; ks = (s0, s1, s2), odd, 1 <= ks[i] <= g[i]
 *        (s2 = 1 when T = 1), radii r_i = ks[i] / 2; C >= 1 channels, K >= 1 filters.
 *   d  : column-major [s0, s1, s2, C, K] -- the learners' d_res as it is: 2D [s,s,K] and 3D
 *        [s,s,s,K] have C = 1, 4D [s,s,U,V,K] has C = U V, 2-3D [s,s,W,K] has C = W.
 *   jc[n + 1], ir[nnz], pr[nnz] : int64 / int64 / double, 0-based, M = X Y T K rows; row
 *        x + X (y + Y (t + T k)) is code k at (x, y, t), the index the session entries emit.
 *   out: column-major [X, Y, T, C, n],
 *        out[x,y,t,c,j] = sum over the entries e of column j, in storage order,
 *                         pr[e] * d[i0, i1, i2, c, k_e],  i_a = (p_a - p_a(e) + r_a) mod g_a,
 *        an entry contributing only when i_a < ks[a] on every axis.
 * That is the circular convolution with the filter embedded the way the learners embed it:
 * padarray(d, size_x - ks, 0, 'post') then circshift by -r (2D/admm_learn_conv2D_large_
 * dParallel.m:38-39; the products and sums over k it stands for: the same file :193,
 * 3D/admm_learn_conv3D_large.m:218-224, 4D/admm_learn_conv4D_lightfield.m:205-206,
 * 2-3D/DictionaryLearning/admm_learn.m:326-343).  The sessions' DZ is a different quantity:
 * it is formed from dup{1}, the spectrum the last d-solve left (:193), which is not the
 * spectrum of the d_res that is returned, and from the full codes, not the thresholded ones.
 * Each output element starts at +0.0 and takes one fma(value, tap, acc) per contributing
 * entry in the column's storage order (for a session's matrix: ascending k, t, y, x); there
 * are no floating-point atomics, so a column's result is the same bits whatever else is in
 * the call, however the host form chunks the columns, and when the column is taken alone.
 * Rows need not be sorted or unique: duplicates add.
 * One-device context only; ordered on the context's stream and synchronised on return.
 * Every argument is validated before the device is touched: CCSC_E_INVALID for a NULL array,
 * an even or non-positive ks[i], ks[i] > g[i], C, K or g[i] < 1, n < 0 or nnz < 0;
 * CCSC_E_UNSUPPORTED for M >= 2^31 and for filters of 2^31 values or more (C K s0 s1 s2; the
 * taps are read from device memory, so this is the only filter budget).  n == 0 is CCSC_OK
 * and writes nothing; nnz == 0 gives zeros.  A malformed matrix reaches no memory: a column
 * range outside [0, nnz] or decreasing and a row outside [0, M) are skipped on the device and
 * the call returns CCSC_E_INVALID (out is then unspecified); the host form also checks jc
 * before any launch.  The host form takes host arrays and stages columns in chunks that keep
 * the device staging (16 B per entry, the chunk's output planes) within 256 MiB, a single
 * column that needs more getting its own; CCSC_CODES_WS_MB=<MiB> lowers that budget (0: one
 * column per chunk).  The _dev form takes every array on the context's device.  Workspace is
 * allocated inside the call and freed before it returns (ccsc_plan_bytes is unchanged). */
int32_t ccsc_synthesize(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C, int32_t K,
                        const int32_t* g, const int64_t* jc, const int64_t* ir, const double* pr,
                        int64_t n, int64_t nnz, double* out, char* err, size_t errlen);
int32_t ccsc_synthesize_dev(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C,
                            int32_t K, const int32_t* g, const int64_t* jc, const int64_t* ir,
                            const double* pr, int64_t n, int64_t nnz, double* out, char* err,
                            size_t errlen);
/* The inverse of ccsc_sparsify_*: out, column-major [M, n], is zero-filled and every entry is
 * stored at its row, bit for bit.  Rows must be strictly ascending inside a column (no two
 * entries may meet); a column that breaks this, a column range outside [0, nnz] and a row
 * outside [0, M) are skipped and the call returns CCSC_E_INVALID.  Validation, context,
 * chunking (8 M bytes of output and 16 B per entry per column) as for ccsc_synthesize. */
int32_t ccsc_densify(ccsc_ctx* ctx, const int64_t* jc, const int64_t* ir, const double* pr,
                     int64_t M, int64_t n, int64_t nnz, double* out, char* err, size_t errlen);
int32_t ccsc_densify_dev(ccsc_ctx* ctx, const int64_t* jc, const int64_t* ir, const double* pr,
                         int64_t M, int64_t n, int64_t nnz, double* out, char* err,
                         size_t errlen);
/* Host only: the index arithmetic of k_synth_codes, for grids whose row count reaches 2^31 - 1.
 * For row `row` of a [g, K] code volume, the output tile [lo, lo + len) per axis, the output
 * point p, channel c and column col: out8 = {x, y, t, k of the row; 1 if the entry lies in
 * the tile's source window (the tile grown by r, circularly); the index into d of the tap
 * that carries the entry to p, or -1 if p is outside the entry's footprint; the index into
 * out of (p, c, col); M}. */
int32_t ccsc_test_synth_index(const int32_t* g, const int32_t* ks, int32_t C, int32_t K,
                              int64_t row, const int32_t* lo, const int32_t* len,
                              const int32_t* p, int32_t c, int64_t col, int64_t* out8, char* err,
                              size_t errlen);

/* Threshold sweep of sparse codes against the data: how an eps for ccsc_session_codes_* /
 * ccsc_sparsify_* is chosen, in one pass over the entries instead of one ccsc_synthesize and
 * one dense reconstruction per candidate.  d, ks, C, K, g, jc, ir, pr, n, nnz: as for
 * ccsc_synthesize.  eps[E], E >= 1: the candidate thresholds, in any order, duplicates,
 * negative values (which keep stored zeros too) and +-inf allowed, a NaN is CCSC_E_INVALID.
 * For threshold e and column j, with "kept" meaning !(|pr| <= eps[e]) -- the predicate of the
 * threshold-and-compact, so a NaN value is kept at every threshold:
 *   nnz_out[e + E j] = the number of kept entries of column j            (int64)
 *   l1_out [e + E j] = sum |pr| over them                                (double)
 *   sse_out[e + E j] = sum over the compared region of (b - R_e)^2       (double)
 * R_e[x, y, t, c, j] is ccsc_synthesize's out for the kept entries alone -- the same embedding,
 * each element from +0.0, one fma(value, tap, acc) per contributing kept entry in storage
 * order, duplicates add -- so it has the bits ccsc_synthesize gives for the filtered triple;
 * it is held in registers and never stored.
 *   crop = 1: b is column-major [g0 - 2 r0, g1 - 2 r1, g2 - 2 r2, C, n] and the interior
 *             r_a <= p_a < g_a - r_a of every axis is compared (the objectives' Dz against the
 *             learners' b; the 2-3D learner's b minus smooth_init);
 *   crop = 0: b is [g0, g1, g2, C, n] and every element is compared.
 * A column without entries, or with none kept, has sse = sum b^2 (in the order below) and
 * l1 = +0.0.  Results come back in the caller's order of eps and do not depend on the other
 * thresholds of the call: the thresholds are sorted and served eight per launch, and a
 * threshold's sums involve its own kept entries only.
 * Order of the sums (no floating-point atomics): inside a workgroup -- one 16 x 16 tile of a
 * t-plane and four channels -- each thread sums its channels in order, a fixed tree joins the
 * threads, and a second kernel adds a column's workgroup partials in block order; nnz is exact
 * and l1 is summed in a fixed order of the column's entries.  So a column's three results are
 * the same bits alone or in any batch, for every chunking, and for both forms.
 * Validation (before the device is touched and before the context check): that of
 * ccsc_synthesize, then CCSC_E_INVALID for a NULL b, eps or output (b and the outputs only
 * when n > 0), E < 1 and a NaN threshold.  One-device context only; n == 0 is CCSC_OK.  A
 * malformed matrix is skipped on the device and gives CCSC_E_INVALID as for ccsc_synthesize.
 * The host form takes host arrays and stages columns in chunks (16 B per entry, the column's
 * slice of b, 24 B per threshold and column, 64 B per workgroup) within 256 MiB or
 * CCSC_CODES_WS_MB; the _dev form takes every array but ks, g and eps on the context's device,
 * runs ordered on its stream and is synchronised on return.  Workspace is allocated inside
 * the call and freed before it returns (ccsc_plan_bytes is unchanged). */
int32_t ccsc_threshold_sweep(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C,
                             int32_t K, const int32_t* g, const int64_t* jc, const int64_t* ir,
                             const double* pr, int64_t n, int64_t nnz, const double* b,
                             int32_t crop, const double* eps, int32_t E, int64_t* nnz_out,
                             double* l1_out, double* sse_out, char* err, size_t errlen);
int32_t ccsc_threshold_sweep_dev(ccsc_ctx* ctx, const double* d, const int32_t* ks, int32_t C,
                                 int32_t K, const int32_t* g, const int64_t* jc,
                                 const int64_t* ir, const double* pr, int64_t n, int64_t nnz,
                                 const double* b, int32_t crop, const double* eps, int32_t E,
                                 int64_t* nnz_out, double* l1_out, double* sse_out, char* err,
                                 size_t errlen);
/* Host only: the threshold class the sweep's kernels give a value -- *m = the number of
 * thresholds of eps[E] that v survives, through the same sort, grouping and inline function. */
int32_t ccsc_test_sweep_class(const double* eps, int32_t E, double v, int32_t* m, char* err,
                              size_t errlen);

/* ---- kernel-level entry points (parity tests of single stages) ---------- */
/* 2D R2C of `count` real slices [X,Y] -> half spectra [Y][X/2+1] (re,im). */
int32_t ccsc_test_fft2d(ccsc_ctx* ctx, int32_t X, int32_t Y, int32_t count, const double* in,
                        double* out_halfspec, double* roundtrip, char* err, size_t errlen);

/* The hooks below are additive test entry points: they add no kernel and change no
 * structure or constant of ABI 7, so CCSC_ABI_VERSION stays (it moves when an existing
 * caller would have to change).  Every hook validates its arguments and plans before
 * it launches anything: a geometry the planner rejects returns CCSC_E_UNSUPPORTED with
 * the planner's message and launches nothing.
 *
 * Transform families (SLICE2D: the LDS slice R2C / C2R of the learners; TTILE: the 3D
 * learner's t-direction tile; LINE2D / LINE3D: the global row / column line passes). */
#define CCSC_FFT_SLICE2D 0
#define CCSC_FFT_TTILE 1
#define CCSC_FFT_LINE2D 2
#define CCSC_FFT_LINE3D 3
/* kernel instantiation a plan runs on: every pass kind; the {2, 3, 7} build of the t
 * tiles; its compile-time 42 x 38 form; the {2, prime-factor 37} build of the slices */
#define CCSC_FFT_INST_ALL 0
#define CCSC_FFT_INST_RM42 1
#define CCSC_FFT_INST_FIXED38 2
#define CCSC_FFT_INST_RM74 3

/* Plan of one transform direction.  n == 0: the family has no such direction. */
typedef struct ccsc_fft_dir_plan {
  int32_t n;         /* line length                                                      */
  int32_t npass;     /* passes, rad[0..npass-1] in execution order                       */
  int32_t rad[4];
  int32_t twoff[4];  /* offset (complex) of pass s's table in the direction's twiddle
                        buffer: (R-1) Ns twiddles, then the R roots of a non-native R    */
  int32_t pfa;       /* 1: pass 1 is the prime-factor pass (74 = 2 * 37)                 */
  int32_t lines;     /* lines per workgroup: Yp/2 (slice x), Xh (slice y, t tile), L row
                        pairs (line rows), TC columns (line columns)                     */
  int32_t groups;    /* workgroups per slice (slice, t tile: 1; rows: groups; columns:
                        xtiles per line set)                                             */
  int32_t ntw;       /* length (complex) of the twiddle buffer the direction reads; the
                        two directions of a slice share one (x tables, then y tables)    */
  int32_t lds_bytes; /* dynamic LDS of a workgroup (slice: the largest any slice kernel
                        asks for, the figure the planner bounds)                         */
  int32_t threads;   /* threads per workgroup                                            */
  int32_t cap[4];    /* per pass, what the instantiation holds: butterflies (native
                        radix), tasks of 3 conjugate output pairs (generic radix), task
                        slots (prime-factor pass)                                        */
  int32_t mask;      /* pass kinds the plan needs: bit R per native radix R, bit 12 the
                        generic pass, bit 13 the prime-factor pass                       */
  int32_t tw_global; /* 1: the twiddle buffer is read from global memory, not staged into
                        LDS (long lines of the line families), lds_bytes excludes it     */
} ccsc_fft_dir_plan;

typedef struct ccsc_fft_plan {
  ccsc_fft_dir_plan dir[3]; /* x, y, t (TTILE: t only)                                   */
  int32_t inst;             /* CCSC_FFT_INST_*: SLICE2D and TTILE; lines are always ALL  */
  int32_t inst_mask;        /* pass kinds that instantiation compiles                    */
} ccsc_fft_plan;

/* Host only (no context, no GPU): the plan the sessions would run, from the planners
 * they call.  SLICE2D: grid X x Y (T ignored); TTILE: X carries Xh (lines), T carries
 * Tn (Y ignored); LINE2D: X x Y; LINE3D: X x Y x T. */
int32_t ccsc_test_fft_plan(int32_t family, int32_t X, int32_t Y, int32_t T, ccsc_fft_plan* out,
                           char* err, size_t errlen);
/* Global line passes on `count` real slices [X, Y, T] (T == 1: the 2D plan): row R2C,
 * then the y (and t) column passes -> out_halfspec [count][T][Y][X/2+1] (re,im); then
 * the inverse column passes and the row C2R scaled by 1/(X Y T) -> roundtrip (same shape
 * as in).  Either output may be NULL. */
int32_t ccsc_test_gfft(ccsc_ctx* ctx, int32_t X, int32_t Y, int32_t T, int32_t count,
                       const double* in, double* out_halfspec, double* roundtrip, char* err,
                       size_t errlen);
/* t-tile transform of `count` complex slices [count][Tn][Yn * Xh] (re,im), one
 * workgroup per (slice, y): forward along t -> out; then the inverse of that result ->
 * roundtrip.  The inverse is NOT normalised: roundtrip = Tn * in.  Either may be NULL. */
int32_t ccsc_test_tfft(ccsc_ctx* ctx, int32_t Tn, int32_t Xh, int32_t Yn, int32_t count,
                       const double* in, double* out, double* roundtrip, char* err,
                       size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* CCSC_H_ */
