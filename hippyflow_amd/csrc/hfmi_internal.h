// Internal declarations shared by the libhfmi translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "hfmi.h"
#include "hfmi_fftcov_plan.h"
#include "hfmi_own.h"
#include "hfmi_qr_rules.h"
#include "hfmi_small_plan.h"
#include "hfmi_spsolve_rules.h"
#include "hfmi_tsgemm_plan.h"

// ------------------------------------------------------------------ errors
void hfmi_set_error(const char* fmt, ...);
#define HFMI_FAIL(code, ...)      \
  do {                            \
    hfmi_set_error(__VA_ARGS__);  \
    return (code);                \
  } while (0)
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      hfmi_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return HFMI_ERR_HIP;                                                                     \
    }                                                                                          \
  } while (0)
#define OWN_TRY(expr) HIP_TRY((hipError_t)(expr))   // own_acquire, the owners' alloc / create and grow (hfmi_own.h)
#define HFMI_TRY(expr)        \
  do {                        \
    int _s = (expr);          \
    if (_s != HFMI_OK) return _s; \
  } while (0)

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
// an A/B or diagnostic switch from the environment: on when set to anything but "" or "0"
static inline bool env_flag(const char* name) {
  const char* e = getenv(name);
  return e && e[0] && !(e[0] == '0' && e[1] == 0);
}

// ------------------------------------------------------------------ objects
enum { WS_PART = 0, WS_G, WS_STAGE, WS_MISC, WS_MGS, WS_COMM, WS_INGEST, WS_NSLOTS };
#define HFMI_INGEST_RING 8

struct hfmi_block {
  hfmi_ctx* ctx;
  double* p;
  int64_t N;
  int nvec;
  int64_t ld;
  bool owner;
};

// Small dense matrices live in one fixed device arena (row-major, ld = SM_LD).
#define SM_MAXK 256
#define SM_LD 256
static_assert(SMALL_MAXK == SM_MAXK, "hfmi_small_plan.h plans for matrices of the small arena");
enum { SM_GRAM = 0, SM_R, SM_RINV, SM_RTOT, SM_T, SM_V, SM_TMP, SM_TMP2, SM_AUX, SM_NSLOTS };

// Small dense matrices of 256 < k <= HFMI_WIDE_MAXK vectors (the wide Cholesky-QR and double pass) live in a second arena that a
// context allocates the first time a wide call arrives: row-major, ld = round_up(k, 32) for the call at hand, slots spaced by the
// arena's capacity (hfmi_chol_wide.hip)
#define HFMI_WIDE_MAXK 2048
enum { WA_GRAM = 0, WA_WORK, WA_R, WA_RINV, WA_RTOT, WA_TMP, WA_T, WA_V, WA_NSLOTS };

struct hfmi_status_words {  // device-resident, read back by the host after small kernels
  double min_pivot_ratio;   // min_j pivot_j / G_jj
  double gram_dev;          // || D^-1/2 G D^-1/2 - I ||_F  (orthonormality defect of the input)
  double offdiag;           // Jacobi: final off-diagonal norm / Frobenius norm
  int shifted;              // Cholesky needed a diagonal shift
  int failed;               // breakdown even after shifting / not converged
  int sweeps;               // Jacobi sweeps used
  int pad;
  long long tick[8];        // shader-clock section timings of the last small kernel (HFMI_DEBUG_TIMING=1 prints them)
};

struct hfmi_comm;
struct xfer_state;
// Owns everything below it.  Members are destroyed in reverse order of declaration, after the destructor's body (hfmi_ctx.hip) has
// waited for the streams: the streams are declared first so that they outlive the events and buffers used on them.
struct hfmi_ctx {
  ~hfmi_ctx();
  int device = 0;
  hip_stream stream;              // the library's own, or the caller's (hfmi_ctx_set_stream: referred to, never released)
  hip_stream aux_stream;          // status read-backs that overlap work queued on `stream`
  hip_stream ingest_stream;       // streaming ingest: uploads from pinned host memory on their own stream; made by the first upload
  hip_event ev0, ev1;
  hip_event ev_status;
  hip_event ev_side;              // small device -> host copies taken off the main stream (late QR checks, eigenvalues)
  int num_cus = 0;
  size_t lds_per_block = 0;       // LDS a workgroup may have on this device (static + dynamic; hipDeviceProp_t::sharedMemPerBlock)
  size_t defl1_static_lds = 0;    // static LDS of k_dcl_deflate<1>, read once per context (hfmi_eig_blocked.hip)
  bool defl1_static_known = false;
  dev_buf<unsigned char> ws[WS_NSLOTS];   // workspaces (ctx_ws); count = bytes
  dev_buf<double> small;          // SM_NSLOTS * SM_MAXK * SM_LD doubles
  dev_buf<double> wide;           // wide arena: WA_NSLOTS matrices of wide_cap x wide_cap doubles + wa_tail_doubles(); empty until needed
  int wide_cap = 0;               // leading dimension the arena is laid out for (a multiple of 32; ctx_wide)
  dev_buf<hfmi_status_words> status_words;   // [1]: a factorisation taken on trust (qr_chol)
  hfmi_status_words* status_dev = nullptr;   // the slot of status_words the next small kernel reports into (qr_chol redirects it around one launch)
  pinned_buf<hfmi_status_words> status_host;
  pinned_buf<unsigned char> pinned;       // pinned host staging (ctx_pinned); count = bytes
  std::vector<hfmi_block*> tmp_blocks;  // cached temporaries for the fused solves
  // storage of destroyed blocks kept for the next hfmi_block_create of the same size (a solve per step returns a fresh
  // U and the caller drops the previous one: without the pool every step pays a hipFree -- a device synchronisation --
  // and a hipMalloc); entries <= 2 GB, at most 16 entries / 8 GB, flushed when an allocation fails
  struct pool_entry { void* p; size_t bytes; };
  std::vector<pool_entry> pool;
  size_t pool_bytes = 0;
  // optional per-launch event timing of the two MFMA kernel classes
  bool profiling = false;
  struct prof_rec { int kind; int64_t m, k, N; hip_event e0, e1; double flops, bytes; };
  std::vector<prof_rec> prof;
  // phases of the fused solves (HFMI_PHASE_*, include/hfmi.h): event pairs on the stream while profiling, plus the
  // host-side wall clock of the host-callback legs
  struct phase_rec { int phase; hip_event e0, e1; };
  std::vector<phase_rec> phase_events;
  double phase_ms[HFMI_PHASE_COUNT] = {};
  // row-panel hook of tsgemm_nn (hfmi_gemm_nn.hip): when set, a large product is issued as a few launches over consecutive
  // row ranges and the hook is called after each with the rows that are final -- hfmi_op_apply reduces those rows over the
  // ranks on the auxiliary stream while the next panel is computed
  int (*nn_hook)(void* user, double* Y, int64_t ldy, int r, int64_t row0, int64_t rows) = nullptr;
  void* nn_hook_user = nullptr;
  int nn_hook_panels = 0;
  bool nn_hook_called = false;
  // set around ONE launch_tsgemm_nn call by a caller that knows its small matrix is upper triangular (Q <- Q R^-1 of the QR):
  // the resident-S kernel then skips the column tiles that are structurally zero at each reduction step (bit-identical results)
  bool nn_upper_hint = false;
  hip_event ev_panel[8], ev_join;
  hip_event ev_ingest[HFMI_INGEST_RING];   // ring of completion events of the ingest stream = tickets
  int64_t ingest_seq = 0;
  pinned_buf<unsigned char> late_pinned;   // status words / R_jj table of an orthogonalisation pass taken on trust (qr_late_buffer, hfmi_qr.hip)
  std::vector<hfmi_comm*> watched_comms;   // communicators whose device-side error word the host synchronisation points check
  pinned_buf<double> pinned_cb;   // second pinned staging area (host-callback operators: double-buffered W and Y slabs)
  hip_event ev_cb[4];             // D2H done x2, H2D done x2
  xfer_state* xfer = nullptr;     // pinned ring + host threads of the large host <-> device transfers (hfmi_xfer.hip), lazily created
  int compose_depth = 0;          // OP_COMPOSE3 applications in progress (nested compositions use separate temporaries)
  // plan record (hfmi_plan_clear / hfmi_plan_read, include/hfmi.h): which contraction / reduction instance every launch was
  int plan_ring[HFMI_PLAN_RING][HFMI_PLAN_WORDS];
  int64_t plan_count = 0;         // launches since the last clear
};
// the slot of the next record, to be filled by one of the *_plan_words helpers (hfmi_tsgemm_plan.h)
static inline int* plan_slot(hfmi_ctx* ctx) { return ctx->plan_ring[ctx->plan_count++ % HFMI_PLAN_RING]; }
// large transfers between the caller's pageable arrays and device memory, pipelined through pinned chunks (hfmi_xfer.hip)
int xfer_d2h(hfmi_ctx* ctx, void* host, const void* dev, size_t bytes);   // returns when the host array is complete
int xfer_h2d(hfmi_ctx* ctx, void* dev, const void* host, size_t bytes);   // returns when the host array has been read
void xfer_destroy(hfmi_ctx* ctx);
int phase_begin(hfmi_ctx* ctx, int phase);     // returns a record index or -1 when not profiling
void phase_end(hfmi_ctx* ctx, int idx);
int phase_begin_on(hfmi_ctx* ctx, int phase, hipStream_t st);   // the same with the events on another stream of the context
void phase_end_on(hfmi_ctx* ctx, int idx, hipStream_t st);
int prof_start(hfmi_ctx* ctx, int kind, int64_t m, int64_t k, int64_t N);  // returns record index or -1
int prof_start_pass(hfmi_ctx* ctx, int64_t L, int64_t flags_part, int64_t index, double bytes);   // a grid covariance pass ("prof_level" 3)
int prof_stop(hfmi_ctx* ctx, int idx);

static inline double* sm_ptr(hfmi_ctx* c, int slot) { return c->small.get() + (size_t)slot * SM_MAXK * SM_LD; }
int ctx_ws(hfmi_ctx* ctx, int slot, size_t bytes, void** out);
int ctx_pinned(hfmi_ctx* ctx, size_t bytes, void** out);
// uninitialised storage for an N x nvec block, from the pool of released blocks or the device; pool_release gives it back (to the pool,
// or when that is full to the device after waiting for the stream).  hfmi_block stays a plain struct that views copy by value.
int block_alloc(hfmi_ctx* ctx, int64_t N, int nvec, hfmi_block** out);
void pool_release(hfmi_ctx* ctx, void* p, size_t bytes);
// Cached temporaries of the context, one block per slot.  Slots of different owners may all be live at once, because the owners
// nest: a fused solve (SOLVE, SKETCH) orthogonalises (QR) and applies operators; an application may be a composition (COMPOSE,
// one pair per nesting depth) whose stages are sparse solves (KRYLOV) or a JJT product; ACCUM belongs to the outermost
// accumulating apply.  No owner calls itself: the sparse solves apply no operator, compositions index their pair by depth.
enum hfmi_tmp_slot {
  TMP_SOLVE_Q = 0,        // double_pass_impl / single_pass_impl: iterate Q (X_0)
  TMP_SOLVE_Y = 1,        // double_pass_impl / single_pass_impl: iterate Y (X_1)
  TMP_SKETCH_Q = 2,       // single_pass_impl (Ybar, then Q), hfmi_sketch_eig (Q)
  TMP_SKETCH_BQ = 3,      // single_pass_impl, hfmi_sketch_eig: B Q
  TMP_QR_BZ = 4,          // qr_chol / qr_mgs: B Q when the caller wants no BQ
  TMP_QR_SAVE = 5,        // borth_qr(AUTO): the input, for the Gram-Schmidt fall-back
  TMP_QR_WIDE = 6,        // qr_chol_wide: the other half of the Q <- Q R^-1 ping-pong (out of place beyond 256 columns)
  TMP_KRYLOV_0 = 8,       // csr_pcg_solve (hfmi_sparse.hip) and its Chebyshev route (hfmi_cheb.hip): r / row-major b
  TMP_KRYLOV_1 = 9,       //   z / x_0
  TMP_KRYLOV_2 = 10,      //   p / x_1
  TMP_KRYLOV_3 = 11,      //   A p
  TMP_JJT_H = 12,         // op_apply_raw(OP_JJT): J_i^T W
  TMP_ACCUM = 13,         // op_apply_raw with beta != 0: the result of a solver / host operator before it is added to Y
  TMP_COMPOSE_BASE = 14   // op_apply_raw(OP_COMPOSE3): tmp_compose_slot(depth) and the slot after it
};
static inline int tmp_compose_slot(int depth) { return depth == 0 ? TMP_COMPOSE_BASE : TMP_COMPOSE_BASE + 2 * depth + 2; }
// *out: a view (by value, not owned) of exactly nvec vectors of the slot's block; the cached block may be wider
int ctx_tmp_view(hfmi_ctx* ctx, int slot, int64_t N, int nvec, hfmi_block* out);
int read_back(hfmi_ctx* ctx, const double* dev, size_t count, double* host);   // `count` doubles to the host; synchronises
int read_status(hfmi_ctx* ctx, hfmi_status_words* out);                        // the status words; synchronises
int side_copies_begin(hfmi_ctx* ctx);   // small device -> host copies on the auxiliary stream, behind this point of the main one
int side_copies_end(hfmi_ctx* ctx);     // ... leaves ev_side for the next writer of their source to wait for
void print_status_dbg(const hfmi_status_words* out);   // HFMI_DEBUG_TIMING=1: the section timings of the last small kernel
// hfmi_block.hip: a host row-major (rows x cols) matrix into device memory with leading dimension ld (zero padded); shape check
int upload_small(hfmi_ctx* ctx, const double* host, int rows, int cols, double* dev, int ld);
int check_same_shape(const hfmi_block* a, const hfmi_block* b, const char* what);

struct hfmi_csr {
  hfmi_ctx* ctx = nullptr;
  int64_t nrows = 0, ncols = 0, nnz = 0;
  dev_buf<int64_t> indptr;
  dev_buf<int32_t> indices;
  dev_buf<double> data;
  // ELLPACK image (slot-major: entry s of row i at [s * nrows + i]) built at creation when the rows are short and
  // even (FEM matrices): consecutive lanes then read consecutive (index, value) pairs.  ell_w == 0: CSR kernel only.
  int ell_w = 0;
  dev_buf<int32_t> ell_idx;
  dev_buf<double> ell_val;
  // What the solvers learn about the matrix, lazily: the matrix itself is const to them.  inv_diag: the Jacobi preconditioner
  // (csr_prepare_jacobi).  Spectrum of the Jacobi-scaled matrix D^-1 A for the Chebyshev solve (hfmi_cheb.hip): an upper bound from
  // Gershgorin's circles (computed from the host arrays at creation), a bracket from the Lanczos matrix of one scalar CG run on
  // the device (first solve); cheb_state: 0 = not estimated yet, 1 = usable, -1 = do not use (estimate failed / a solve did not
  // reach its tolerance)
  mutable struct solve_state {
    dev_buf<double> inv_diag;
    double gersh_lmax = 0.0, cheb_lmin = 0.0, cheb_lmax = 0.0;
    int cheb_state = 0;
  } solve;
};

// what a launcher needs of a general Matern kernel (HFMI_KERNEL_MATERN) beside (family, sigma, ell, nugget)
struct kcov_nu_ref {
  double nu = 0.0;
  double ca = 0.0;                // sqrt(2 nu), word KNU_W_CA of the table
  const double* tab = nullptr;    // the table words on the device (hfmi_kcov_nu.h)
};
struct fftcov_state;
struct interp_state;
struct boxcov_state;
enum hfmi_op_kind { OP_SNAPSHOT_GRAM, OP_JTJ, OP_JJT, OP_DENSE_SYM, OP_CSR, OP_CSR_PCG, OP_COMPOSE3, OP_HOST, OP_AMG_PCG, OP_KERNEL_COV, OP_KERNEL_CROSS, OP_KERNEL_COV_GRID, OP_GRID_FACTOR, OP_GRID_INTERP, OP_KERNEL_COV_INTERP, OP_INTERP_FACTOR, OP_BOX };

struct hfmi_op {
  ~hfmi_op();              // waits for the stream when the operator owns device memory (hfmi_op.hip)
  hfmi_ctx* ctx = nullptr;
  hfmi_op_kind kind = OP_SNAPSHOT_GRAM;
  hfmi_block X = {};     // snapshot / Jacobian / dense block (by value: a view, not owned)
  int ndata = 0, q = 0;
  dev_buf<double> gamma_inv;   // q x q row-major (ld = round_up(q,16)) or empty
  dev_buf<double> weights;     // one per vector of X (general diagonal of a low-rank operator) or empty
  double scale = 1.0;
  const hfmi_csr* csr = nullptr;
  double rel_tol = 0.0;
  int max_iter = 0;
  int last_iters = 0;
  int last_method = 0;    // sparse solver: 0 = block CG, 1 = Chebyshev, 2 = AMG-preconditioned CG (hfmi_op_solver_info)
  hfmi_amg* amg = nullptr;   // OP_AMG_PCG: the multigrid hierarchy (not owned)
  hfmi_op *a = nullptr, *b = nullptr, *c = nullptr;
  // OP_KERNEL_COV: the point coordinates on the device, one array of kc_N doubles per dimension, and the kernel
  dev_buf<double> kc_x;
  int64_t kc_N = 0;
  int kc_d = 0, kc_family = 0;
  double kc_sigma = 0.0, kc_ell = 0.0, kc_nugget = 0.0;
  // OP_KERNEL_CROSS: K(T, S) with S in kc_x (kc_N points).  kc_slab: T = S[kc_diag : kc_diag + kc_M], Y is addressed at row kc_diag and
  // an overwriting apply zeroes its other rows (hfmi_op_kernel_cov_rows).  Otherwise T is kc_t (one array of kc_M doubles per
  // dimension) and Y has kc_M rows; kc_diag: target i is source i + kc_diag, HFMI_KERNEL_NO_DIAGONAL for none (hfmi_op_kernel_cross_cov).
  dev_buf<double> kc_t;
  int64_t kc_M = 0, kc_diag = 0;
  bool kc_slab = false;
  // family HFMI_KERNEL_MATERN: the smoothness, sqrt(2 nu) as the table builder rounded it, and the table words on the device
  double kc_nu = 0.0, kc_nuca = 0.0;
  dev_buf<double> kc_nutab;
  kcov_nu_ref kc_nu_ref() const { return kcov_nu_ref{kc_nu, kc_nuca, kc_nutab}; }
  fftcov_state* fc = nullptr;   // OP_KERNEL_COV_GRID: the grid, the node map, Lambda, the twiddles and the work buffer (owned; hfmi_fftcov.hip)
  // OP_GRID_FACTOR: the state of the sampler the factor was made from, shared with it (hfmi_op_grid_factor); 0: S, 1: S^T
  std::shared_ptr<fftcov_state> fac;
  int fac_transpose = 0;
  // OP_GRID_INTERP: W (ip_transpose 0: length prod n -> N) or W^T (1) of a sparse cubic interpolation from grid nodes to points;
  // OP_KERNEL_COV_INTERP: K = W Cg W^T + diag(delta) with Cg = ip_grid (a grid covariance, not owned: hfmi_op_compose3's rule).  The
  // state (binned weights, delta, the work block) is owned (hfmi_interp.hip)
  // OP_INTERP_FACTOR: F = [W S | diag(sqrt(delta))] (fac_transpose 0) or F^T (1): `fac` is the sampler's state as for OP_GRID_FACTOR, ip_grid
  // the interpolated operator (not owned, as its own grid operator is not) whose state and work block the applies use; ip stays null
  interp_state* ip = nullptr;
  int ip_transpose = 0;
  hfmi_op* ip_grid = nullptr;
  // OP_BOX: W^a T_s W^b of a box (hfmi_op_box): the box's state (grid, twiddles, work buffer), shared with it as OP_GRID_FACTOR shares its
  // sampler's; the table lambda^s / prod P_c of this operator (owned) and the powers of the quadrature weights
  std::shared_ptr<boxcov_state> box;
  dev_buf<double> box_table;
  double box_a = 0.0, box_b = 0.0;
  hfmi_host_apply_fn host_fn = nullptr;
  void* host_user = nullptr;
  int64_t host_N = 0;
  int host_chunk = 0;    // > 0: the callback is invoked on slabs of this many vectors (pipelined with the copies)
  hfmi_post_apply_fn post_fn = nullptr;
  void* post_user = nullptr;
  hfmi_comm* comm = nullptr;   // rank average / sum of the result block (hfmi_op_set_collective), null = none
  int comm_op = 0;
  bool reduced_by_panels = false; // the last apply already reduced its result over the ranks, panel by panel (hfmi_op.hip)
};
// Y = M^-1 W for an SPD CSR matrix by Chebyshev iteration, or Jacobi-preconditioned block CG (hfmi_sparse.hip)
int csr_pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y);
int csr_prepare_jacobi(hfmi_ctx* ctx, const hfmi_csr* M);   // M->solve.inv_diag, made the first time it is asked for
// the Chebyshev route of csr_pcg_solve (hfmi_cheb.hip); *handled = false: nothing written to Y, the caller runs the block CG
int cheb_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, bool* handled);
// Y = A^-1 W by AMG-preconditioned block CG (hfmi_amg.hip); Y zero-filled on error
int amg_pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y);
// in-place all-reduce of `count` doubles of device memory on the communicator's context stream (hfmi_comm.hip)
int comm_allreduce_device(hfmi_comm* c, double* data, int64_t count, int op);
int comm_allreduce_device_on(hfmi_comm* c, double* data, int64_t count, int op, void* hip_stream /* null = the context's */);
int comm_transport(const hfmi_comm* c);   // 0 host, 1 rccl, 2 p2p
// HFMI_ERR_COMM if a stream-ordered collective of this communicator gave up (time-out) or met a peer that had; no device call
int comm_check_error(hfmi_comm* c);
// make the p2p staging buffer large enough for a collective of `bytes` NOW (a collective: every rank calls it with the same
// size), so that it never regrows while row panels of an application are in flight on the auxiliary stream
int comm_reserve_stage(hfmi_comm* c, size_t bytes);
void comm_forget_ctx(hfmi_comm* c);        // the context is going away first: stop referring to it
void ctx_watch_comm(hfmi_ctx* ctx, hfmi_comm* c);
void ctx_unwatch_comm(hfmi_ctx* ctx, hfmi_comm* c);
int ctx_check_comm(hfmi_ctx* ctx);        // comm_check_error over the watched communicators

// ------------------------------------------------------------------ kernel launchers (hfmi_gemm.hip)
// C (m x k) = scale * A^T B (+ beta * C); A: N x m, B: N x k column-major blocks.
// C is addressed as C[i*rs + j*cs] (device); out_colmajor selects the partial layout that makes
// the final write coalesced when rs == 1.
int launch_tsgemm_tn(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* B, int64_t ldb, int k,
                     int64_t N, double scale, double beta, double* C, int64_t rs, int64_t cs, int nsplit_req);
// skinny x skinny variant (hfmi_skinny.hip): both operands staged through LDS, m, k <= 160 and m + k <= 288 columns
int launch_tsgemm_ss(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* B, int64_t ldb, int k,
                     int64_t N, double scale, double beta, double* C, int64_t rs, int64_t cs, int nsplit_req);
// C[i*rs + j*cs] = scale * sum_sp part[sp][..] + beta * C, fixed summation order (part and C: where the call's slices and result start)
int launch_reduce_partials(hfmi_ctx* ctx, const double* part, const reduce_call& c, double scale, double beta, double* C, int64_t rs,
                           int64_t cs);
// Y (N x r) = alpha * A (N x m) * S (m x r, device row-major, ld = lds, zero padded to 16 cols) + beta * Y
int launch_tsgemm_nn(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* S, int lds, int r,
                     double alpha, double beta, double* Y, int64_t ldy, int64_t N);

// Y (+)= C W with C_ij = sigma^2 phi(|x_i - x_j| / ell) + nugget delta_ij evaluated in registers (hfmi_kcov.hip); x: d arrays of N doubles
int launch_kernel_cov(hfmi_ctx* ctx, const double* x, int64_t N, int d, int family, double sigma, double ell, double nugget,
                      const double* W, int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate, const kcov_nu_ref& nu = kcov_nu_ref());
// Y (M rows) (+)= K W (N rows), K_ij = sigma^2 phi(|t_i - x_j| / ell) + nugget [j == i + diag_offset] (diag_offset < 0: no nugget); t: d
// arrays of M doubles, tstride apart.  Same per-row summation order as launch_kernel_cov.  M = 0: nothing is launched.
int launch_kernel_cross_cov(hfmi_ctx* ctx, const double* x, int64_t N, const double* t, int64_t M, int64_t tstride, int64_t diag_offset,
                            int d, int family, double sigma, double ell, double nugget, const double* W, int64_t ldw, double* Y,
                            int64_t ldy, int nvec, int accumulate, const kcov_nu_ref& nu = kcov_nu_ref());

// The metric of a kernel covariance, r^2 = delta^T G delta / ell^2 with G symmetric positive definite, enters through its lower Cholesky
// factor G = L L^T: |L^T delta|^2 is the same number and cannot round below zero.  Scattered points are uploaded as x' = L^T x, so the
// kernels see an isotropic problem; the grid's column takes L itself (hfmi_fftcov.hip).  kcov_metric_factor (hfmi_op.hip) checks G
// (finite, |G_ij - G_ji| <= 4 eps max |G|, every pivot positive) and writes L row-major d x d, zeros above the diagonal.
int kcov_metric_factor(const double* G, int d, double* L);

// Kernel covariance on a regular grid by FFT (hfmi_fftcov.hip; plans: hfmi_fftcov_plan.h).  create checks the arguments, uploads the
// node map and the twiddles and computes Lambda; apply is Y (+)= C W; destroy deletes the state (the caller synchronised)
// metric_factor: the lower Cholesky factor of the kernel's metric (d x d row-major, kcov_metric_factor), or null for none;
// max_line > 0: the long route (split-line passes, hfmi_fftcov_plan.h) with that longest line, 0: the old route;
// nu: the smoothness of HFMI_KERNEL_MATERN (the state builds and owns its tables), unread otherwise
int fftcov_create(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N, int family, double sigma,
                  double ell, double nugget, const double* metric_factor, fftcov_state** out, int max_line = 0, double nu = 0.0);
// the table words of a general Matern kernel (hfmi_kernel_matern_tables) on the device, and sqrt(2 nu) as the builder rounded it (hfmi_op.hip)
int kcov_nu_upload(hfmi_ctx* ctx, double nu, dev_buf<double>* out, double* ca);
int64_t fftcov_points(const fftcov_state* st);
int fftcov_apply(hfmi_ctx* ctx, fftcov_state* st, const double* W, int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate);
void fftcov_destroy(fftcov_state* st);
// Y (+)= S W (transpose 0: length prod P_c -> N) or S^T W (1: N -> prod P_c), the factor of a sampler's embedding; checks the lengths
int fftcov_factor_apply(hfmi_ctx* ctx, fftcov_state* st, int transpose, const hfmi_block* W, hfmi_block* Y, int accumulate);

// what hfmi_interp.hip needs to know of a grid covariance and of a sampler (hfmi_fftcov.hip)
struct fftcov_grid_desc {
  int d;
  int64_t n[3];
  double h[3];
  double sigma, nugget;
  bool all_nodes;      // no node map: point g is node g
  bool long_route;
};
void fftcov_describe(const fftcov_state* st, fftcov_grid_desc* out);
// grid, node map or none, kernel, metric and smoothness agree (an operator and a sampler made from it)
bool fftcov_same_covariance(const fftcov_state* a, const fftcov_state* b);
// table[(o0 + 3) + 7 ((o1 + 3) + 7 (o2 + 3))] (device, 7^d doubles) = the kernel at the signed lattice offset o, nugget left out, by
// the code that fills the circulant's first column; queued on the context's stream
int fftcov_offset_table(hfmi_ctx* ctx, const fftcov_state* st, double* table);
const fftcov_state* grid_sampler_state(const hfmi_grid_sampler* s);
hfmi_ctx* grid_sampler_ctx(const hfmi_grid_sampler* s);
// what a factor operator takes of a sampler: the root table in its state (made at the first call; `who` heads the message of a failed
// allocation), the state itself to share, and prod P_c, the length of the padded vectors S acts on
int grid_sampler_root(hfmi_grid_sampler* s, const char* who);
std::shared_ptr<fftcov_state> grid_sampler_share(hfmi_grid_sampler* s);
int64_t fftcov_padded_len(const fftcov_state* st);
// Whittle-Matern operators on a box by DCT / FFT (hfmi_boxcov.hip; plans: hfmi_boxcov_plan.h): Y (+)= W^a T_s W^b X with the operator's table
int64_t boxcov_points(const boxcov_state* st);
int boxcov_apply(hfmi_ctx* ctx, boxcov_state* st, const double* table, double a, double b, const double* W, int64_t ldw, double* Y,
                 int64_t ldy, int nvec, int accumulate);
// Interpolation between grid nodes and scattered points (hfmi_interp.hip; rules: hfmi_interp_plan.h).  apply: Y (+)= W X, W^T X
// or K X by the operator's kind; destroy deletes the state (the caller synchronised)
int interp_apply(hfmi_op* op, const hfmi_block* X, hfmi_block* Y, int accumulate);
void interp_destroy(interp_state* st);
int64_t interp_range_len(const hfmi_op* op);   // OP_GRID_INTERP: N for W, prod n for W^T; OP_INTERP_FACTOR: N for F, prod P_c + N for F^T
// Y (+)= F X or F^T X of an OP_INTERP_FACTOR; checks the lengths
int interp_factor_apply(hfmi_op* op, const hfmi_block* X, hfmi_block* Y, int accumulate);

// ------------------------------------------------------------------ QR (hfmi_qr.hip)
// Y = A S, S upper triangular
int launch_nn_upper(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* S, int ld, int r, double* Y, int64_t ldy, int64_t N);
// Pinned home of what a Cholesky-QR pass taken on trust reports, for the caller to judge after the synchronisation it needs anyway
// (ctx->late_pinned, made by ctx_late_pinned).  The single pass parks the status words of its LU solve in the first slot.
struct qr_late_buffer {
  alignas(128) hfmi_status_words st2;   // the second pass's status words
  alignas(128) hfmi_status_words st1;   // the first pass's, when that one was taken on trust as well
  double aux[SM_LD + SM_MAXK];          // SM_AUX: [0, k) original column norms; [SM_LD, SM_LD + k) diag(Rtot)
};
static_assert(sizeof(hfmi_status_words) <= 128 && sizeof(qr_late_buffer) == 256 + sizeof(double) * (SM_LD + SM_MAXK),
              "two sets of status words share the first 256 bytes of the late-check buffer");
int ctx_late_pinned(hfmi_ctx* ctx, qr_late_buffer** out);
// Y = op X in column panels of at most 256 vectors (block views): no operator kind sees a width it was not written for
int op_apply_panels(hfmi_op* op, const hfmi_block* X, hfmi_block* Y);
extern int g_qr_wide_min;      // width from which a checked qr_chol takes the wide route (tuning key "qr_wide_min", 17..257; default 257)
struct qr_result {             // where qr_chol left things
  int passes = 0;
  bool deferred = false;       // the last pass was not applied: Q stands for Q R^-1 with R^-1 in SM_RINV
  bool wide = false;           // the wide arena holds Rtot (WA_RTOT, ld = round_up(k, 32)), not SM_RTOT
  bool late = false;           // the second pass was taken on trust: ctx->late_pinned holds what qr_late_stands judges ...
  bool first_trusted = false;  // ... and the first one too
};
// repeated Cholesky-QR by the rules of hfmi_qr_rules.h; want_r: exact triangular factors in every pass (see borth_qr)
int qr_chol(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, bool want_r, qr_policy policy, qr_result* res);
bool qr_late_stands(const qr_late_buffer* late, int k, bool first_trusted);   // the late verdict (qr_late_verdict) on the buffer
// hfmi_borth_qr with want_r (exact triangular factors in every Cholesky pass) chosen by the caller
int borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, bool want_r, int method, int* passes);

// ------------------------------------------------------------------ kernel launchers (hfmi_misc.hip)
// 2-D elementwise launch geometry: x over row pairs (16 B per lane), y over vectors (grid-stride)
static inline dim3 ew_grid(int64_t N, int nvec) {
  const int64_t pairs = (N + 1) / 2;
  int64_t gx = (pairs + 255) / 256;
  if (gx > 4096) gx = 4096;
  int gy = nvec < 1024 ? nvec : 1024;
  return dim3((unsigned)gx, (unsigned)gy);
}
int launch_fill(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld, double value, bool include_pad);
int launch_zero_pad(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld);
int launch_row_scale(hfmi_ctx* ctx, double* G, int ld, int m, int k, const double* w);
int launch_matern32(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld, int nx, int ny, double sigma, double ell);
int launch_copy(hfmi_ctx* ctx, double* dst, int64_t ldd, const double* src, int64_t lds, int64_t N, int nvec);
int launch_scale(hfmi_ctx* ctx, double* p, int64_t ld, int64_t N, int nvec, double alpha);
int launch_axpy(hfmi_ctx* ctx, double* y, int64_t ldy, double alpha, const double* x, int64_t ldx, int64_t N, int nvec);
int launch_randn(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld, uint64_t seed, uint32_t stream, double sigma);
int launch_philox_raw(hfmi_ctx* ctx, uint32_t* out, int64_t N, int nvec, uint64_t seed, uint32_t stream);
// dense (N x nvec row-major, contiguous) <-> block
int launch_dense_to_block(hfmi_ctx* ctx, const double* dense, double* p, int64_t ld, int64_t N, int nvec);
int launch_block_to_dense(hfmi_ctx* ctx, const double* p, int64_t ld, double* dense, int64_t N, int nvec);
int launch_block_to_dense_ld(hfmi_ctx* ctx, const double* p, int64_t ld, double* dense, int64_t ldd, int64_t N, int nvec);
// out[j] = the sum of the nchunks partials of column j, fixed order (device out)
int launch_dots_final(hfmi_ctx* ctx, const double* part, int nchunks, int nvec, double* out);
// out[j] = <A_j, B_j> for j < nvec (device out)
int launch_col_dots(hfmi_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t N, int nvec,
                    double* out);
// small q x q (row-major) applied to each sample's q x k slab of G in place: G_i <- Gamma G_i
int launch_gamma_apply(hfmi_ctx* ctx, double* G, int ldg, int ndata, int q, int k, const double* gamma, int ldgam);
int launch_gamma_apply_cm(hfmi_ctx* ctx, const double* Gc, double* out, int64_t ld, int ndata, int q, int k, const double* gamma,
                          int ldgam);

// ------------------------------------------------------------------ Chebyshev iteration and reductions on row-major (nrows x k) arrays (hfmi_cheb.hip)
unsigned rm_grid(hfmi_ctx* ctx, int64_t nrows, int k, int per_cu);   // a workgroup per group of rows (hfmi_rm_dev.h), at most per_cu a CU
int launch_cheb_first(hfmi_ctx* ctx, const double* B, double* X1, double* X0, const double* inv_diag, int64_t nrows, int k, double inv_theta);
int launch_cheb_step(hfmi_ctx* ctx, const hfmi_csr* M, const double* B, const double* Xc, double* Xp, int k, double c1, double c2, bool resid);
// per-column reductions, fixed summation order; part: k * RM_CHUNKS doubles of the caller's, or null for the context's workspace
constexpr int RM_CHUNKS = 1024;
int launch_rm_colsq(hfmi_ctx* ctx, const double* A, int64_t nrows, int k, double* part, double* out);                      // <A_j, A_j>
int launch_rm_coldots(hfmi_ctx* ctx, const double* A, const double* B, int64_t nrows, int k, double* part, double* out);   // <A_j, B_j>
// alpha_j = rz_j / pap_j (0 unless pap_j > 0 and alpha_j finite): X += alpha P, R -= alpha AP, rr_j = <R_j, R_j>
int launch_rm_cg_update(hfmi_ctx* ctx, int64_t nrows, int k, double* X, double* R, const double* P, const double* AP, const double* rz,
                        const double* pap, double* part, double* rr);

// ------------------------------------------------------------------ sparse products and the kernels of the block CG (hfmi_sparse.hip)
int launch_csr_spmm(hfmi_ctx* ctx, const hfmi_csr* M, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec,
                    bool accumulate);
// Y = M X fused with the per-column dots dots[j] = <X_j, Y_j> (PCG: p . A p); needs the ELL image
int launch_ell_spmm_dot(hfmi_ctx* ctx, const hfmi_csr* M, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec,
                        double* dots);
// One fused PCG update per column j (alpha_j = rz_j / pap_j): y += alpha p, r -= alpha ap, then
// rz_new_j = <r, D^-1 r> and rr_j = <r, r> (device outputs, fixed summation order)
int launch_pcg_update(hfmi_ctx* ctx, double* y, int64_t ldy, double* r, int64_t ldr, const double* p, int64_t ldp,
                      const double* ap, int64_t ldap, const double* inv_diag, int64_t N, int nvec, const double* rz,
                      const double* pap, double* rz_new, double* rr);
// p_j = D^-1 r_j + (rz_new_j / rz_j) p_j
int launch_pcg_direction(hfmi_ctx* ctx, double* p, int64_t ldp, const double* r, int64_t ldr, const double* inv_diag,
                         int64_t N, int nvec, const double* rz_new, const double* rz);
// per-column updates used by PCG / MGS (coefficients on device)
// y_j += sign * (num_j / den_j) * x_j   (den may be null -> coefficient num_j)
int launch_col_axpy_dev(hfmi_ctx* ctx, double* y, int64_t ldy, const double* x, int64_t ldx, int64_t N, int nvec,
                        const double* num, const double* den, double sign);
// p_j = z_j + (num_j/den_j) * p_j
int launch_col_xpby_dev(hfmi_ctx* ctx, double* p, int64_t ldp, const double* z, int64_t ldz, int64_t N, int nvec,
                        const double* num, const double* den);
// z_j = inv_diag .* r_j
int launch_diag_scale(hfmi_ctx* ctx, double* z, int64_t ldz, const double* r, int64_t ldr, const double* inv_diag,
                      int64_t N, int nvec);

// ------------------------------------------------------------------ the one-workgroup k x k stage (plans: hfmi_small_plan.h)
// the dynamic-LDS attribute of a kernel, raised where its plan says so
static inline int small_raise_lds(const void* kern, const small_launch& L) {
  if (L.raise) HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
  return HFMI_OK;
}
// hfmi_chol_col.hip (column-at-a-time kernels) and hfmi_chol.hip (blocked MFMA kernel, the default):
// G (k x k, SM slot) = R^T R; writes R (upper), Rinv (upper); if rtot_accumulate, Rtot <- R * Rtot.
// Status words (min pivot ratio, defect, shifted/failed) land in ctx->status_dev.
int launch_chol_inv(hfmi_ctx* ctx, int k, int slot_gram, int slot_r, int slot_rinv, int slot_rtot, int rtot_mode,
                    int full_r, double shift_rel, double pivot_tol);
// hfmi_jacobi.hip: T (k x k) -> eigenvalues (sorted descending) into dvals (device, k), eigenvectors into slot_v (columns).
int launch_jacobi_eig(hfmi_ctx* ctx, int k, int slot_t, int slot_v, double* dvals, int sort_by_abs);
// the same contract by Householder tridiagonalisation + divide and conquer (hfmi_eig_dc.hip): LAPACK dsyevd's algorithm
// family, i.e. what the reference's np.linalg.eigh runs; absolute accuracy eps ||T||
int launch_dc_eig(hfmi_ctx* ctx, int k, int slot_t, int slot_v, double* dvals, int sort_by_abs);
// dispatcher (sym_eig_route): method 0 = default (divide and conquer unless tuning "eig" = 1), 1 = Jacobi (high relative accuracy)
int launch_sym_eig(hfmi_ctx* ctx, int k, int slot_t, int slot_v, double* dvals, int sort_by_abs, int method);
int launch_chol_mfma(hfmi_ctx* ctx, int k, int slot_gram, int slot_r, int slot_rinv, int slot_rtot, int rtot_mode, int full_r,
                     double shift_rel, double pivot_tol);   // hfmi_chol.hip
// ------------------------------------------------------------------ wide Cholesky + inverse (hfmi_chol_wide.hip)
static inline double* wa_ptr(hfmi_ctx* c, int slot) { return c->wide.get() + (size_t)slot * c->wide_cap * c->wide_cap; }
static inline double* wa_aux(hfmi_ctx* c) { return wa_ptr(c, WA_NSLOTS); }   // [0, k): original column norms; [ld, ld + k): diag(Rtot)
int ctx_wide(hfmi_ctx* ctx, int k);      // make the arena hold k x k matrices (allocates / regrows; zero filled)
// The contract of launch_chol_inv on the wide arena with ld = round_up(k, 32): G = WA_GRAM -> R (WA_R), R^-1 (WA_RINV), both upper
// with zero strict lower triangles; rtot_mode 1: Rtot (WA_RTOT) <- R, 2: Rtot <- R Rtot; the AUX table (wa_aux) and the status
// words, which it also returns on the host (it synchronises the stream: the restart with the shifted diagonal is the host's decision)
int launch_chol_wide(hfmi_ctx* ctx, int k, int rtot_mode, double shift_rel, double pivot_tol, hfmi_status_words* host_st);
int pchol_tuning_set(const char* key, int value); // "pchol_grid": cap on the workgroups of the pivoted Cholesky launches (hfmi_pchol.hip)
int api_tuning_set(const char* key, int value);   // 1 = key handled ("comm_panels", "prof_level", "qr_trust_first", "qr_wide_min"; hfmi_ctx.hip, as hfmi_tuning_set)
extern int g_comm_panels;      // row panels of an overlapped rank reduction (hfmi_op.hip reads HFMI_COMM_PANELS when -1)
extern int g_qr_trust_first;   // first Cholesky-QR pass taken on trust (hfmi_qr.hip reads HFMI_QR_TRUST_FIRST when -1)
int launch_small_set_identity(hfmi_ctx* ctx, int k, int slot);   // hfmi_small.hip, as the product below
// slot_c (k x r, zero padded to 16 columns) = slot_a (k x k) * slot_b[:, :r]
int launch_small_matmul(hfmi_ctx* ctx, int k, int r, int slot_a, int slot_b, int slot_c);
// hfmi_jacobi.hip: R (k x k, slot_r) = U diag(s) V^T: singular values descending in svals (device), U -> slot_u, V -> slot_v (columns)
int launch_jacobi_svd(hfmi_ctx* ctx, int k, int slot_r, int slot_u, int slot_v, double* svals);
// hfmi_lu.hip: X (m x m, slot_x) = W^-1 Z by LU with partial pivoting (slot_a: working copy of W), and when slot_t >= 0 also
// T = (X + X^T) / 2 into slot_t.  Status words: min / max |pivot|, failed = 1 non-finite input, 2 singular W.
int launch_lu_solve(hfmi_ctx* ctx, int m, int slot_w, int slot_z, int slot_a, int slot_x, int slot_t);

constexpr int HFMI_EIG_MAXN = 16384;     // largest symmetric eigenproblem (hfmi_sym_eig_small / _leading, hfmi_block_gram_eig)
// symmetric eigensolve for 256 < n <= HFMI_EIG_MAXN: host in, host out.  hfmi_eig_blocked.hip (panel tridiagonalisation on the MFMA, divide
// and conquer, block-reflector back-transformation); HFMI_EIG_LARGE=jacobi selects the two-sided Jacobi of hfmi_eig_large.hip
// nvec < 0 or > n: all eigenvectors; otherwise host_V is n x nvec (the leading eigenvectors in output order)
// dev_T: the matrix in device memory (n x n row-major) instead of host_T
int sym_eig_large(hfmi_ctx* ctx, const double* host_T, int n, int sort_by_abs, double* host_d, double* host_V, int nvec = -1,
                  const double* dev_T = nullptr);

int eig_dgemm_bench(hfmi_ctx* ctx, int M, int N, int K, int ta, int tb, int reps, const double* host_A, const double* host_B,
                    double* host_C, double* avg_ms);
