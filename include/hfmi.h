/*
 * hfmi.h -- C ABI of libhfmi.so, the MI355X (gfx950) device layer under the
 * hippyflow model-based projectors' randomized double-pass eigensolve.
 *
 * The reference (hippyflow, /root/reference) has no FFI of its own: its boundary
 * is a set of duck-typed Python protocols over the
 * third-party hippylib package, whose only native pieces are a C++ MultiVector
 * and a C++ mt19937 "parRandom" compiled by dolfin.  Each entry point below
 * names the reference call site / hippylib symbol it stands in for.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns 0 on
 *     success or a negative hfmi_status; hfmi_last_error() gives the text.
 *   - all arithmetic is IEEE fp64.
 *   - one hfmi_ctx per GPU; a context (and the objects made from it) is not
 *     thread-safe; independent contexts may be used from different threads or
 *     processes.  All work is enqueued on the context's HIP stream.
 *   - a BLOCK is hippylib's MultiVector: nvec vectors of length N, each vector
 *     contiguous in HBM (column-major N x nvec with leading dimension ld,
 *     ld % 32 == 0, 256-byte aligned columns, rows N..ld-1 kept at zero).
 *     Snapshot matrices (n snapshots of length N; PODProjector.py:340-357) and
 *     stacked Jacobians ((ndata*q) rows of length N; operatorWrappers.py:62-64)
 *     are blocks too: one vector per snapshot / per Jacobian row.
 *   - host arrays are caller-owned, dense, C-ordered fp64.
 */
#ifndef HFMI_H
#define HFMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFMI_VERSION 100

/* Entry points are the only symbols libhfmi.so exports (it is built with -fvisibility=hidden).  Define HFMI_API before
 * including this header to override the attribute. */
#ifndef HFMI_API
#if defined(__GNUC__)
#define HFMI_API __attribute__((visibility("default")))
#else
#define HFMI_API
#endif
#endif

typedef enum {
  HFMI_OK = 0,
  HFMI_ERR_INVALID = -1,      /* bad argument / shape mismatch (the reference asserts) */
  HFMI_ERR_HIP = -2,          /* a HIP runtime call failed */
  HFMI_ERR_NO_DEVICE = -3,    /* no usable gfx950 device */
  HFMI_ERR_NUMERIC = -4,      /* breakdown (e.g. Gram matrix not SPD after shifting) */
  HFMI_ERR_CALLBACK = -5,     /* a host callback operator returned non-zero */
  HFMI_ERR_NOT_CONVERGED = -6,/* iterative kernel hit its iteration cap */
  HFMI_ERR_COMM = -7          /* communicator failure (RCCL error, peer rank missing, time-out) */
} hfmi_status;

/* host <-> block layouts */
#define HFMI_LAYOUT_VECTORS 0 /* host (nvec, N): one vector per row  -- u_data / q_data / J (PODProjector.py:224-225) */
#define HFMI_LAYOUT_DENSE 1   /* host (N, nvec): mv_to_dense layout  -- utilities/mv_utilities.py:31-41 */

typedef struct hfmi_ctx hfmi_ctx;
typedef struct hfmi_block hfmi_block;
typedef struct hfmi_csr hfmi_csr;
typedef struct hfmi_op hfmi_op;
typedef struct hfmi_comm hfmi_comm;
typedef struct hfmi_amg hfmi_amg;
typedef struct hfmi_pchol hfmi_pchol;
typedef struct hfmi_grid_sampler hfmi_grid_sampler;
typedef struct hfmi_box hfmi_box;

/* ---------------------------------------------------------------- context */
HFMI_API const char* hfmi_last_error(void);
HFMI_API int hfmi_version(void);
HFMI_API const char* hfmi_build_tag(void);   /* identity of the kernel sources (hash); keys the PMC records bench.py may use */
HFMI_API int hfmi_device_count(int* count);
HFMI_API int hfmi_ctx_create(int device, hfmi_ctx** out);
HFMI_API int hfmi_ctx_destroy(hfmi_ctx* ctx);
/* adopt an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
HFMI_API int hfmi_ctx_set_stream(hfmi_ctx* ctx, void* hip_stream);
HFMI_API int hfmi_ctx_get_stream(hfmi_ctx* ctx, void** hip_stream);
HFMI_API int hfmi_ctx_synchronize(hfmi_ctx* ctx);
HFMI_API int hfmi_ctx_device_info(hfmi_ctx* ctx, char* name, int name_len, int* compute_units, int64_t* hbm_bytes);
HFMI_API int hfmi_ctx_pci_bus_id(hfmi_ctx* ctx, char* buf, int len);   /* "0000:5d:00.0": keys the sysfs clock / power files bench.py reads */
/* HIP-event timer on the context's stream (bench.py measures kernels with it) */
HFMI_API int hfmi_timer_start(hfmi_ctx* ctx);
HFMI_API int hfmi_timer_stop(hfmi_ctx* ctx, double* milliseconds); /* synchronises */

/* ---------------------------------------------------------------- blocks
 * hippylib MultiVector(vector, nvec) and its copy constructor. */
HFMI_API int hfmi_block_create(hfmi_ctx* ctx, int64_t N, int nvec, hfmi_block** out); /* zero-filled */
/* wrap device memory owned by the caller (e.g. a torch tensor): ld % 32 == 0, ld >= N,
 * dptr 128-byte aligned; rows N..ld-1 are zeroed by the call. */
HFMI_API int hfmi_block_wrap(hfmi_ctx* ctx, double* dptr, int64_t N, int nvec, int64_t ld, hfmi_block** out);
/* view of vectors [first, first+count) of a block (MultiVector.__getitem__) */
HFMI_API int hfmi_block_view(hfmi_block* parent, int first, int count, hfmi_block** out);
HFMI_API int hfmi_block_destroy(hfmi_block* b);
HFMI_API int hfmi_block_info(const hfmi_block* b, int64_t* N, int* nvec, int64_t* ld, double** dptr);
HFMI_API int hfmi_block_upload(hfmi_block* b, const double* host, int layout);
HFMI_API int hfmi_block_download(const hfmi_block* b, double* host, int layout);
/* streaming ingest: the reference fills its snapshot / Jacobian blocks sample by sample from host PDE solves
 * (PODProjector.py:343-357; activeSubspaceProjector.py:178-221).  hfmi_block_upload_async copies from PINNED host memory
 * (hfmi_host_alloc_pinned) on the context's ingest stream and returns at once; *ticket names the upload.
 * hfmi_ingest_wait(ticket): the pinned buffer of that upload may be overwritten (host wait).  hfmi_ingest_fence: work
 * enqueued afterwards on the compute stream sees every upload made so far (device-side wait, the host is not blocked).
 * b is normally a view (hfmi_block_view) of the vectors of one sample. */
HFMI_API int hfmi_host_alloc_pinned(size_t bytes, void** out);
HFMI_API int hfmi_host_free_pinned(void* p);
HFMI_API int hfmi_block_upload_async(hfmi_block* b, const double* host_pinned, int layout, int64_t* ticket);
HFMI_API int hfmi_ingest_wait(hfmi_ctx* ctx, int64_t ticket);
HFMI_API int hfmi_ingest_fence(hfmi_ctx* ctx);
HFMI_API int hfmi_block_zero(hfmi_block* b);                                 /* MultiVector.zero */
HFMI_API int hfmi_block_copy(hfmi_block* dst, const hfmi_block* src);        /* copy constructor */
HFMI_API int hfmi_block_scale(hfmi_block* b, double alpha);                  /* vector *= alpha */
HFMI_API int hfmi_block_axpy(hfmi_block* y, double alpha, const hfmi_block* x); /* vector.axpy, all vectors */
HFMI_API int hfmi_block_norms(const hfmi_block* b, double* host_norms);      /* MultiVector.norm("l2") */

/* a1: the probe draw -- hp.parRandom.normal(sigma, Omega)
 * (activeSubspaceProjector.py:433-443,536-551; PODProjector.py:365-374;
 * KLEProjector.py:151-160).  Counter-based Philox4x32-10 + Box-Muller: every GPU
 * regenerates the same Omega from (seed, stream), replacing collective.bcast.
 * Rows 4g .. 4g+3 of vector j come from the counter (g, j, stream) under the key
 * seed: four 32-bit uniforms -> two radius/angle pairs (oracle/philox.py). */
HFMI_API int hfmi_randn_fill(hfmi_block* b, uint64_t seed, uint32_t stream, double sigma);
/* the raw 32-bit stream behind it (bit-exact parity test): out[nvec][ceil(N/4)][4] */
HFMI_API int hfmi_philox_raw(hfmi_block* shape_of, uint64_t seed, uint32_t stream, uint32_t* host_out);

/* synthetic config-2 input: C (N x N block) = Matern-3/2 covariance
 * sigma^2 (1 + a) exp(-a), a = sqrt(3) d_ij / ell, over the first N nodes of an nx x ny grid on the unit square */
HFMI_API int hfmi_block_fill_matern32(hfmi_block* C, int nx, int ny, double sigma, double ell);

/* MultiVector.dot_mv / dot_v: out[i*nvecB + j] = <A_i, B_j>  (row-major nvecA x nvecB) */
HFMI_API int hfmi_block_dot(const hfmi_block* A, const hfmi_block* B, double* host_out);
/* MvDSmatMult / MultiVector.reduce: Y = alpha * A * S + beta * Y, S host (nvecA x nvecY) row-major */
HFMI_API int hfmi_block_gemm_small(const hfmi_block* A, const double* host_S, double alpha, double beta, hfmi_block* Y);

/* ---------------------------------------------------------------- sparse
 * CSR matrix (prior.M, prior.R; PODProjectorFromData.M_csr, PODProjector.py:695-697). */
HFMI_API int hfmi_csr_create(hfmi_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* indptr,
                    const int32_t* indices, const double* data, hfmi_csr** out);
HFMI_API int hfmi_csr_destroy(hfmi_csr* m);

/* ---------------------------------------------------------------- operators
 * The reference's linear-operator protocol (mult / matMvMult / init_vector;
 * SURVEY.md section 8b) as a tagged object.  apply = hp.MatMvMult(A, W, Y). */

/* a2: hp.LowRankOperator(ones/n, snapshots)  -> Y = scale * X (X^T W)
 *     (PODProjector.py:359-361).  X: block, one vector per snapshot. */
HFMI_API int hfmi_op_snapshot_gram(hfmi_ctx* ctx, const hfmi_block* X, double scale, hfmi_op** out);
/*     general diagonal: hp.LowRankOperator(d, U) -> Y = U diag(d) (U^T W)  (prior.Hlr as B / B^-1,
 *     activeSubspaceProjector.py:455-459; priorPreconditionedProjector.py:48-55).  host_d: one weight per vector of U. */
HFMI_API int hfmi_op_low_rank(hfmi_ctx* ctx, const hfmi_block* U, const double* host_d, hfmi_op** out);
/* a3: sample-averaged Jacobian Gram  Y = scale * sum_i J_i^T Gamma^{-1} J_i W
 *     (MeanJTJfromDataOperator.mult, operatorWrappers.py:95-114; JTJ summed by
 *     SummedListOperator / SeriallySampledJacobianOperator,
 *     activeSubspaceProjector.py:82-95,163-248).  J: block of ndata*q vectors
 *     (row o of sample i is vector i*q+o); gamma_inv host q x q or NULL. */
HFMI_API int hfmi_op_jtj(hfmi_ctx* ctx, const hfmi_block* J, int ndata, int q, const double* host_gamma_inv,
                double scale, hfmi_op** out);
/*     output-space counterpart  Y = scale * sum_i J_i J_i^T W  (JJT, jacobian.py:169-193;
 *     activeSubspaceProjector.py:625-673); acts on blocks of length q. */
HFMI_API int hfmi_op_jjt(hfmi_ctx* ctx, const hfmi_block* J, int ndata, int q, double scale, hfmi_op** out);
/* a4: explicit dense symmetric operator (config 2 covariance; npToDolfinOperator,
 *     operatorWrappers.py:19-52).  C: block of N vectors of length N (symmetric). */
HFMI_API int hfmi_op_dense_sym(hfmi_ctx* ctx, const hfmi_block* C, hfmi_op** out);
/*     the same covariance without the N x N block: C_ij = sigma^2 phi(|x_i - x_j| / ell) + nugget delta_ij over N points with
 *     d = 1, 2 or 3 coordinates each (host_points: N x d row-major, copied to the device), entries evaluated inside the apply
 *     (hfmi_kcov.hip) -- 16 N k bytes move per apply instead of 8 N^2, so N is not capped by HBM.  With r = |x_i - x_j| / ell:
 *       HFMI_KERNEL_MATERN12  exp(-a), a = r              HFMI_KERNEL_MATERN32  (1 + a) exp(-a), a = sqrt(3) r
 *       HFMI_KERNEL_MATERN52  (1 + a + a^2/3) exp(-a), a = sqrt(5) r              HFMI_KERNEL_SQEXP  exp(-r^2 / 2)
 *     HFMI_ERR_INVALID: d outside 1..3, ell <= 0, nugget < 0, unknown family, N < 1; at apply, blocks of another length.
 *     The summation order is fixed: two applies of the same input are bit-identical. */
#define HFMI_KERNEL_MATERN12 0
#define HFMI_KERNEL_MATERN32 1
#define HFMI_KERNEL_MATERN52 2
#define HFMI_KERNEL_SQEXP 3
#define HFMI_KERNEL_MATERN1 4 /* a K_1(a), a = sqrt(2) r: only through a hfmi_kernel_spec (below); the creators with a bare family refuse it */
#define HFMI_KERNEL_MATERN 5  /* Matern of any smoothness nu: only through a hfmi_kernel_spec2 (below); every other creator refuses it */
HFMI_API int hfmi_op_kernel_cov(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, int family, double sigma, double ell,
                       double nugget, hfmi_op** out);
/*     the rectangular cross-covariance between two point sets, by the same kernel: K_ij = sigma^2 phi(|t_i - s_j| / ell)
 *     + nugget [j == i + diag_offset] over M targets t and N sources s (both row-major x d on the host, copied to the device).  It acts
 *     on blocks of length N and gives blocks of length M: the Nystrom extension of a KLE, or of a pivoted Cholesky factor, to other
 *     points.  The nugget sits on the point INDEX: target i is source i + diag_offset; HFMI_KERNEL_NO_DIAGONAL says that no target is a
 *     source, and then the nugget must be 0.  Coincident points with different indices get no nugget.
 *     HFMI_ERR_INVALID: as hfmi_op_kernel_cov, M < 1, a diag_offset other than HFMI_KERNEL_NO_DIAGONAL that is negative or has
 *     diag_offset + M > N, a non-zero nugget without a diagonal; at apply, blocks of other lengths.
 *     Every row is summed over the sources in the order hfmi_op_kernel_cov uses: two applies are bit-identical. */
#define HFMI_KERNEL_NO_DIAGONAL (-1)
HFMI_API int hfmi_op_kernel_cross_cov(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d,
                       int family, double sigma, double ell, double nugget, int64_t diag_offset, hfmi_op** out);
/*     a row slab of hfmi_op_kernel_cov's matrix as an operator on blocks of length N: rows row0 .. row0 + nrows - 1 of Y = C W, computed as
 *     the cross-covariance with targets s[row0 : row0 + nrows] (read in place, no second copy) and diag_offset = row0.  An overwriting
 *     apply writes +0.0 to the other rows below N, an accumulating one leaves them alone; nrows = 0 is valid (all zeros / a no-op).
 *     With one slab per rank and hfmi_op_set_collective(op, comm, HFMI_REDUCE_SUM) every rank holds C W after 2 N^2 k / P flops.
 *     HFMI_ERR_INVALID: as hfmi_op_kernel_cov, row0 < 0, nrows < 0, row0 + nrows > N; at apply, blocks of another length.
 *     A slab's rows are the same bits as those rows of hfmi_op_kernel_cov's apply, and adding zeros is exact: the slabs of a partition
 *     of 0 .. N, summed in any order, reproduce the square apply bit for bit. */
HFMI_API int hfmi_op_kernel_cov_rows(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, int family, double sigma, double ell,
                       double nugget, int64_t row0, int64_t nrows, hfmi_op** out);
/*     the same covariance over nodes of a REGULAR GRID, applied by FFT in O(P log P) per pair of vectors instead of 2 N^2 flops per
 *     vector (hfmi_fftcov.hip).  The grid has n[0] x ... x n[d-1] nodes, d = 1, 2 or 3, spacing h[c] > 0 along axis c, axis 0 fastest:
 *     node g = i0 + n[0] (i1 + n[1] i2) (the numbering of hfmi_block_fill_matern32).  Point i of the operator is grid node host_nodes[i]
 *     (N distinct indices in [0, prod n), any order; copied to the device); NULL = all nodes in order, N = prod n.  The matrix is the
 *     one hfmi_op_kernel_cov has over those points.  For a stationary kernel it is block-Toeplitz with Toeplitz blocks; embedded in a
 *     circulant of P_c = the smallest power of two >= 2 n[c] - 1 (1 when n[c] = 1) entries along axis c, with first column
 *     c[j] = sigma^2 phi(|offset(j)| / ell), offset_c = min(j_c, P_c - j_c) h[c], c[0] += nugget, it is diagonalised by the FFT and the
 *     product is EXACT up to rounding: scatter W into the zero-padded grid, transform, multiply by Lambda = FFT(c) (real, computed once
 *     at creation on the device by the same kernels), transform back, gather the nodes into Y.  Two real columns ride one complex
 *     transform, z = w_j + i w_{j+1}, paired from the first column of the block handed to the apply (a last odd column pairs with
 *     zeros): a column's result depends on its partner in the last bits.  No atomics: two applies of the same block are bit-identical,
 *     whatever the tuning key "fftcov_pairs" says.  Block storage contract as every operator.  The operator owns Lambda, the twiddle
 *     table (built on the host in long double, rounded once) and a work buffer of 16 prod P_c bytes per pair of a chunk.
 *     HFMI_ERR_INVALID: d outside 1..3, n[c] < 1 or > 2048, h[c] <= 0 or not finite, N < 1, a node out of range or repeated, NULL nodes
 *     with N != prod n, unknown family, ell <= 0, nugget < 0; at apply, blocks of another length.  HFMI_ERR_HIP with the sizes in the
 *     message when the work buffer of one pair cannot be allocated.  hfmi_pchol_create refuses this operator. */
HFMI_API int hfmi_op_kernel_cov_grid(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */,
                                     const int64_t* host_nodes_or_null, int64_t N, int family, double sigma, double ell,
                                     double nugget, hfmi_op** out);
/*     The four kernel covariances above from a DESCRIPTOR of the kernel, which adds two things the bare (family, sigma, ell, nugget)
 *     cannot say.  The argument lists are the ones above with the descriptor in place of those four; spec->d must equal d.
 *       HFMI_KERNEL_MATERN1: phi = a K_1(a), a = sqrt(2) r, phi(0) = 1 -- the Matern field of smoothness nu = 1, which is the kernel of
 *     the squared operator (delta - gamma div Theta grad)^2 in two dimensions (the BiLaplacian prior).  K_1 is evaluated on the device
 *     by its power series for a <= 2 and by a Chebyshev interpolant of sqrt(a) e^a K_1(a) in 2 / a beyond (csrc/hfmi_kcov_k1.h), to a few
 *     units of the last place; a = 0 (the diagonal, duplicate points) gives exactly 1, large a underflows to +0.  That evaluation costs
 *     several times the others, so a Matern-1 apply of hfmi_op_kernel_cov is bound by it, not by the matrix cores.
 *       A METRIC: r = sqrt(delta^T G delta) / ell with G symmetric positive definite, d x d row-major in metric[0 .. d*d-1]; all nine
 *     entries zero = the identity, which with one of the four first families is exactly the creator above (same kernels, same bits).
 *     G is factored G = L L^T on the host (hfmi_kernel_metric_factor).  Scattered points -- sources and targets -- are uploaded as
 *     x' = L^T x, so the apply, the row slab and hfmi_pchol_* see an isotropic problem and are the kernels they were.  On a grid the
 *     matrix stays block-Toeplitz but the kernel is even only in the whole offset vector, so the circulant's first column takes signed
 *     offsets: position s_c stands for o_c = s_c below P_c / 2 and s_c - P_c above it, the entry at s_c = P_c / 2 is the mean over both
 *     signs (no apply reads it), r^2 = |L^T diag(h) o|^2 / ell^2.  The column is jointly even, Lambda is real, and everything after
 *     it -- the passes, hfmi_grid_sampler_* with its growth and clipping, hfmi_op_grid_factor -- is unchanged and picks family and metric
 *     up from the operator.
 *     HFMI_ERR_INVALID: what the creator above answers, with family up to HFMI_KERNEL_MATERN1 allowed; spec NULL or spec->d != d; a metric
 *     with an entry that is not finite, with |G_ij - G_ji| > 4 eps max |G|, or with a Cholesky pivot that is not positive. */
typedef struct hfmi_kernel_spec {
  int family; /* HFMI_KERNEL_*, MATERN1 included */
  int d;
  double sigma, ell, nugget;
  double metric[9]; /* row-major d x d; all zeros = identity */
} hfmi_kernel_spec;
HFMI_API int hfmi_op_kernel_cov_spec(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec* spec, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cross_cov_spec(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d,
                                           const hfmi_kernel_spec* spec, int64_t diag_offset, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_rows_spec(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec* spec, int64_t row0,
                                          int64_t nrows, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_grid_spec(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */,
                                          const int64_t* host_nodes_or_null, int64_t N, const hfmi_kernel_spec* spec, hfmi_op** out);
/*     the lower Cholesky factor of a metric, on the host, no context and no device: G (d x d row-major, d = 1, 2 or 3) -> L (d x d
 *     row-major, zeros above the diagonal), unblocked, column by column.  HFMI_ERR_INVALID as listed above. */
HFMI_API int hfmi_kernel_metric_factor(const double* G, int d, double* L);
/*     its launch plan, from the planner the launcher asks (csrc/hfmi_fftcov_plan.h); no context and no device.  nvec vectors, a work
 *     buffer budget in bytes (<= 0: the default, 512 MiB); the tuning key "fftcov_pairs" counts as in an apply.
 *     words[HFMI_FFTCOV_PLAN_WORDS]:  0 d  1-3 P_c  4 prod P_c  5 pairs = ceil(nvec / 2)  6 pairs per chunk  7 chunks  8 passes
 *     9 bytes of work buffer per pair  10 twiddle entries  11 max P_c  12 static LDS of the pass kernel; then 16 words per pass from
 *     word 16:  axis, flags (1 forward, 2 multiply, 4 inverse, 8 scatter fused, 16 gather fused), line length, line stride, lines,
 *     positions loaded, positions stored, lines per workgroup, LDS line stride, threads, dynamic LDS, static + dynamic LDS, grid x
 *     (grid y = the pairs of the chunk), and the line map oe0, os0, os1:  line l starts at entry
 *     (l mod stride) + ((l div stride) mod oe0) os0 + ((l div stride) div oe0) os1. */
#define HFMI_FFTCOV_PLAN_WORDS 96
HFMI_API int hfmi_fftcov_plan_predict(int d, const int64_t* n, int nvec, int64_t budget_bytes, int64_t* words);
/*     EXACT draws m ~ N(0, C) of that covariance at the cost of an apply, by circulant embedding (Dietrich-Newsam, Wood-Chan):
 *       z = IFFT_unnormalised( sqrt(max(Lambda / P, 0)) (xi_1 + i xi_2) ),  xi i.i.d. N(0, 1) on the padded grid;
 *     Re z and Im z on the nodes are two independent draws.  d passes per pair of draws (an apply has 2 d - 1), no operand read but
 *     Lambda: the first pass generates its load from Philox4x32-10 and the probe draw's Box-Muller (the element map, which depends
 *     on (seed, pair, storage position) only, is stated in csrc/hfmi_fftcov_plan.h).  The square root needs Lambda >= 0, which the
 *     operator's minimal embedding often lacks, so the sampler has an embedding of its own: growth g doubles every P_c with n[c] > 1
 *     g times (while every P_c <= 4096).  hfmi_grid_sampler_create copies grid, kernel and node map from the operator (the sampler
 *     does not depend on the operator's lifetime), then tries g = 0 .. max_growth and takes the first whose
 *     lambda_min >= -floor, floor = 16 eps log2(prod P_c) lambda_max: eigenvalues in [-floor, 0) are rounding and become 0 silently.
 *     If none qualifies: clip = 0 is HFMI_ERR_INVALID with lambda_min / lambda_max at the last growth tried in the message; clip = 1
 *     takes that growth, sets every negative eigenvalue to 0 and reports their number and cov_error_bound = sum |lambda^-| / prod P_c:
 *     the clipped part is a positive semidefinite circulant with that constant diagonal, so |Cov(draw) - C|_ij <= cov_error_bound for
 *     all i, j.  hfmi_grid_sampler_info: the growth taken, P_c, the extreme eigenvalues of the embedding, n_clipped and the bound (0, 0
 *     unless clipped); any pointer may be NULL.
 *     hfmi_grid_sampler_draw: column j of Y (+)= draw first_sample + j of the stream `seed`; draws 2 p and 2 p + 1 are Re and Im of pair
 *     p, so first_sample must be even, an odd number of columns drops the last Im, and chunks of a stream (first_sample = 0, 64, ...)
 *     reproduce one large call bit for bit, whatever "fftcov_pairs" says.  Block storage contract as every operator: padding rows
 *     untouched, accumulate != 0 adds.  No atomics.  Y is const as a HANDLE (its pointer, length and leading dimension are read, never
 *     changed); the draw stores into the block's memory, rows below N of its columns.  The contract cases of this writer are in
 *     tests/test_gpu_grid_sampler.py.
 *     HFMI_ERR_INVALID: not a grid covariance operator, max_growth outside 0..3, Y of another length, first_sample odd or negative
 *     or past the 2^33 draws of a seed.  hfmi_fftcov_sample_plan_predict: the draw's launch plan without a device, the words of
 *     hfmi_fftcov_plan_predict (pass flag 32: generated load) with word 13 = growth; HFMI_ERR_INVALID for an infeasible growth. */
HFMI_API int hfmi_grid_sampler_create(hfmi_op* grid_cov_op, int max_growth /* 0..3 */, int clip /* 0 | 1 */, hfmi_grid_sampler** out);
HFMI_API int hfmi_grid_sampler_info(const hfmi_grid_sampler* s, int* growth, int64_t* P /* 3 */, double* lambda_min, double* lambda_max,
                                    int64_t* n_clipped, double* cov_error_bound);
HFMI_API int hfmi_grid_sampler_draw(hfmi_grid_sampler* s, const hfmi_block* Y, uint64_t seed, int64_t first_sample /* even */, int accumulate);
HFMI_API int hfmi_grid_sampler_destroy(hfmi_grid_sampler* s);
HFMI_API int hfmi_fftcov_sample_plan_predict(int d, const int64_t* n, int growth, int nsamples, int64_t budget_bytes, int64_t* words);
/*     the FACTOR C = S S^T of a sampler's embedding as two operators, so that a grid covariance can take the caller's noise
 *     (prior.sample(noise, m): m = mean + S noise) and whiten a Hessian (S^T H S) without any solve.  The embedding circulant Chat has
 *     a non-negative (or clipped) spectrum; its symmetric square root is again a circulant, applied by the passes of an apply with
 *     sqrt(max(Lambda / P, 0) / P) in place of Lambda / P, P = prod P_c:  Chat^(1/2) xi = IFFT_unnormalised( root . FFT(xi) ).  With Rn the
 *     restriction to the operator's points,  S = Rn Chat^(1/2)  (transpose = 0) maps blocks of length P to blocks of length N and
 *     S^T = Chat^(1/2) Rn^T  (transpose = 1) maps length N to length P;  S S^T = C up to rounding, C + E with |E_ij| <= cov_error_bound
 *     for a clipped sampler.  A padded vector is an ordinary block in natural order, entry e = s0 + P0 (s1 + P1 s2): P is 4 to 64 times
 *     N depending on d and the growth, which is what the caller's noise costs against hfmi_grid_sampler_draw's generated one.
 *     Applied through hfmi_op_apply: 2 d - 1 passes per pair of columns, two real columns per complex transform (a last odd column
 *     pairs with zeros), chunked by "fftcov_pairs" with identical bits; no atomics, two applies are bit-identical; block storage
 *     contract as every operator (padding rows untouched, accumulate adds).  The root table is a second table made once per
 *     sampler at its first factor: Lambda and the draws are untouched.  The operator shares the sampler's state: either may be
 *     destroyed first.  HFMI_ERR_INVALID: NULL sampler, transpose outside 0 / 1; at apply, blocks of another length.
 *     hfmi_fftcov_factor_plan_predict: the apply's launch plan without a device, the words of hfmi_fftcov_plan_predict (pass flags
 *     64 / 128: the load / the store addresses the block of padded vectors) with word 13 = growth and word 14 = transpose;
 *     HFMI_ERR_INVALID where hfmi_fftcov_sample_plan_predict says so, and for a transpose outside 0 / 1. */
HFMI_API int hfmi_op_grid_factor(hfmi_grid_sampler* s, int transpose /* 0: S | 1: S^T */, hfmi_op** out);
HFMI_API int hfmi_fftcov_factor_plan_predict(int d, const int64_t* n, int growth, int transpose, int nvec, int64_t budget_bytes,
                                             int64_t* words);
/*     The LONG route: the same operator, sampler and factor with embedding axes longer than one workgroup's line.  An embedding axis
 *     with P_c > max_line is split into P_c = L1 L2 (L2 = max_line) and transformed in two passes, Bailey's four-step without
 *     transposes: L1-point DFTs along the strided sub-axis with the twiddle exp(-2 pi i n2 k1 / P_c) fused into their store, then
 *     L2-point DFTs (the inverse mirrors it, the conjugate twiddle fused into the load).  The spectrum lands in the storage order of the
 *     old route; nothing is permuted.  2 (d + s) - 1 passes per pair of columns with s split axes.  The rules are in
 *     csrc/hfmi_fftcov_plan.h.  max_line is the tuning key "fftcov_max_line" at creation (a power of two in 4 .. 4096, default 4096),
 *     read by this route alone.  Caps: nodes per axis 1 .. 2^23, every P_c <= max_line^2, sampler growth 0 .. 6.  With no axis split
 *     the passes are the old route's: applies, draws and factors are bit-identical to those of hfmi_op_kernel_cov_grid_spec /
 *     hfmi_grid_sampler_create.  Everything else as there: all five families and the metric, block storage contract, no atomics,
 *     bit-identical whatever "fftcov_pairs" says; hfmi_op_grid_factor takes samplers of either route.
 *     HFMI_ERR_INVALID: what hfmi_op_kernel_cov_grid_spec answers with the caps above; hfmi_grid_sampler_create_long: an operator that is
 *     not of hfmi_op_kernel_cov_grid_long, max_growth outside 0..6.  hfmi_grid_sampler_create on such an operator takes the old route
 *     and answers HFMI_ERR_INVALID when an axis has more than 2048 nodes.  A create whose buffers do not fit returns HFMI_ERR_HIP, *out
 *     untouched.
 *     hfmi_fftcov_long_plan_predict: the launch plan of kind 0 (apply, growth 0), 1 (draw), 2 (factor S) or 3 (factor S^T) at longest
 *     line max_line, no context and no device; HFMI_ERR_INVALID for the refusals above, max_line not a power of two in 4 .. 4096, or a
 *     kind outside 0 .. 3.  words[HFMI_FFTCOV_LONG_PLAN_WORDS]: a head of 16 words (0-11 as hfmi_fftcov_plan_predict, 11 the longest
 *     LINE, 12 static LDS of the split kernel, 13 growth, 14 kind, 15 max_line), then 24 per pass from word 16: the 16 words of a pass
 *     of hfmi_fftcov_plan_predict (flags 256 / 512: twiddle fused into the store / the load; static + dynamic LDS of the kernel that
 *     runs the pass), then part (0 whole axis, 1 high sub-axis, 2 low), L1, L2, inner, esub, sub_stride, pm, sm: line l of a
 *     sub-axis pass starts at entry  (l mod inner) + sub sub_stride + (o mod oe0) os0 + (o div oe0) os1  with
 *     sub = (l div inner) mod esub, o = (l div inner) div esub, and line position p is axis position p pm + sub sm. */
#define HFMI_FFTCOV_LONG_PLAN_WORDS 280
HFMI_API int hfmi_op_kernel_cov_grid_long(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */,
                                          const int64_t* host_nodes_or_null, int64_t N, const hfmi_kernel_spec* spec, hfmi_op** out);
HFMI_API int hfmi_grid_sampler_create_long(hfmi_op* grid_cov_long_op, int max_growth /* 0..6 */, int clip /* 0 | 1 */, hfmi_grid_sampler** out);
HFMI_API int hfmi_fftcov_long_plan_predict(int kind, int d, const int64_t* n, int growth, int max_line, int nvec, int64_t budget_bytes,
                                           int64_t* words);
/*     The Matern family of ANY smoothness, HFMI_KERNEL_MATERN, through a second descriptor that carries nu:
 *       phi_nu(a) = 2^(1-nu) / Gamma(nu) a^nu K_nu(a),  a = sqrt(2 nu) r / ell,  phi_nu(0) = 1,  HFMI_MATERN_NU_MIN <= nu <= HFMI_MATERN_NU_MAX
 *     -- the convention of the named families (a = r, sqrt(3) r, sqrt(5) r, sqrt(2) r for nu = 1/2, 3/2, 5/2, 1).  The precision
 *     (delta - gamma div Theta grad)^alpha in d dimensions has this covariance with nu = alpha - d/2.  K_nu is evaluated on the device
 *     (csrc/hfmi_kcov_nu.h): with n = floor(nu + 1/2), mu = nu - n, Temme's series for K_mu, K_(mu+1) up to a = 2 and Chebyshev
 *     interpolants of sqrt(a) e^a K in 2 / a beyond, then the recurrence in the order on scaled quantities.  Everything that depends on
 *     nu is computed once on the host at creation (hfmi_kernel_matern_tables, long double) and kept by the operator on the device.
 *     There is NO silent dispatch: nu = 1.5 through this family runs the general evaluation, 2.3 times the cost of Matern-1 per entry (measured at nu = 1.25),
 *     and agrees with HFMI_KERNEL_MATERN32 to rounding; the named families stay the fast ones.  a = 0 gives exactly 1, a large a +0.
 *       hfmi_kernel_spec2 is hfmi_kernel_spec with nu appended; families 0..5; nu is read only for HFMI_KERNEL_MATERN and must be 0
 *     otherwise.  Each creator below has the argument list of its predecessor with the descriptor type exchanged, and with families 0..4
 *     gives the operator its predecessor gives (same kernels, same bits).  hfmi_pchol_create, hfmi_grid_sampler_create[_long] and
 *     hfmi_op_grid_factor take such operators and pick nu and the tables up from them (the sampler keeps copies of its own).
 *     HFMI_ERR_INVALID: what the predecessor answers, with family up to HFMI_KERNEL_MATERN allowed; nu not finite or outside the range
 *     with HFMI_KERNEL_MATERN, nu != 0 with another family.
 *       hfmi_kernel_matern_tables: the table words of one nu, on the host, no context and no device (layout: csrc/hfmi_matern_tables.hip).
 *     HFMI_ERR_INVALID for a null pointer and for nu not finite or outside the range. */
#define HFMI_MATERN_NU_MIN 0.125
#define HFMI_MATERN_NU_MAX 8.0
#define HFMI_MATERN_TABLE_WORDS 162
typedef struct hfmi_kernel_spec2 {
  int family; /* HFMI_KERNEL_*, MATERN included */
  int d;
  double sigma, ell, nugget;
  double metric[9]; /* row-major d x d; all zeros = identity */
  double nu;        /* the smoothness of HFMI_KERNEL_MATERN; 0 with every other family */
} hfmi_kernel_spec2;
HFMI_API int hfmi_op_kernel_cov_spec2(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec2* spec, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cross_cov_spec2(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d,
                                            const hfmi_kernel_spec2* spec, int64_t diag_offset, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_rows_spec2(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec2* spec, int64_t row0,
                                           int64_t nrows, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_grid_spec2(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */,
                                           const int64_t* host_nodes_or_null, int64_t N, const hfmi_kernel_spec2* spec, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_grid_long_spec2(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */,
                                                const int64_t* host_nodes_or_null, int64_t N, const hfmi_kernel_spec2* spec, hfmi_op** out);
HFMI_API int hfmi_kernel_matern_tables(double nu, double* words /* HFMI_MATERN_TABLE_WORDS */);
/*     SCATTERED points on the FFT route, by structured kernel interpolation:  K = W Cg W^T + diag(delta).  Cg is the matrix of a grid
 *     covariance above over ALL nodes of its grid with nugget 0, W (N x prod n) a sparse cubic interpolation from the grid's nodes to N
 *     points.  K is symmetric positive semidefinite whatever the interpolation error, an apply costs O(4^d N + P log P), a draw is
 *     W z + sqrt(delta) eta with z an exact grid draw.  K is an APPROXIMATION of the covariance C over the points, unlike every other
 *     operator of this family; the library is held to K as defined here at rounding level, and K - C is a property of the kernel and of
 *     ell / h (figures: docs/measurements.md; rough kernels such as HFMI_KERNEL_MATERN12 stay the domain of the exact routes).
 *       Grid: d = 1, 2 or 3 axes of n[c] >= 4 nodes, spacing h[c] > 0, origin[c]; axis 0 fastest.  Per axis of a point x:
 *     u = (x - origin) / h in double, 1 <= u <= n - 2 required; c = min(floor(u), n - 3), t = u - c; the weights on nodes c - 1 .. c + 2
 *     are Keys' cubic convolution (a = -1/2),  w0 = ((2 - t) t - 1) t / 2,  w1 = ((3 t - 5) t t + 2) / 2,  w2 = ((4 - 3 t) t + 1) t / 2,
 *     w3 = (t - 1) t t / 2, evaluated in these forms on the HOST at creation (csrc/hfmi_interp_plan.h) and uploaded: the device never
 *     recomputes a weight.  Row i of W holds the 4^d tensor products; its sum is 1, polynomials up to degree 2 are reproduced.
 *       hfmi_grid_interp_weights: those rules without a context or a device.  base[N]: the node of the stencil corner (c_a - 1)_a;
 *     w[N * d * 4]: w[(i d + a) 4 + s]; optionally the cell binning the spread walks: the stencil base cells form an (n0 - 3) x ... array,
 *     linear index axis 0 fastest; cell_start[prod (n - 3) + 1] and perm[N] list the points of cell q as perm[cell_start[q] ..
 *     cell_start[q + 1] - 1], ascending in point index.  Either of the two may be NULL.
 *       hfmi_op_grid_interp: W (transpose = 0: blocks of length prod n -> blocks of length N, a gather) or W^T (transpose = 1, a
 *     spread) through hfmi_op_apply.  Stencil order of the gather: s2 outermost, s0 innermost, weight (w2 w1) w0, one fused multiply-add
 *     per node.  The spread has NO atomics: a grid node receives from the at most 4^d cells q with q_a in g_a - 3 .. g_a, visited in
 *     ascending linear index, the points of a cell in ascending index; that order is part of the contract, so the result depends on no
 *     launch shape and two applies are bit-identical.  The device keeps 4 d doubles and two indices per point (a CSR image of W holds
 *     4^d values and indices per point and orientation).  Heavily clustered points unbalance the spread; that is accepted.
 *       hfmi_op_kernel_cov_interp: K as ONE operator over the grid operator's grid: one spread, the grid operator's apply, one gather
 *     with + delta_i X_ij fused, through an internal work block of prod n rows that takes an even number of columns per chunk (512 MiB,
 *     or 2 "fftcov_pairs" columns): the grid apply pairs the columns as in one call, so no chunking changes a bit.
 *     q_i = (W Cg W^T)_ii = sum over stencil pairs of w_s w_s' c(s - s'), c(.) the kernel at the signed lattice offsets in [-3, 3]^d
 *     evaluated by the code that fills the circulant's first column, summed once at creation on the device through the per-axis
 *     autocorrelations of the weights (csrc/hfmi_interp_plan.h).  delta_i = nugget + max(sigma^2 - q_i, 0) with diag_correction = 1,
 *     delta_i = nugget with 0: with the correction K_ii = sigma^2 + nugget wherever nothing was clipped.  hfmi_op_kernel_cov_interp_info:
 *     the extremes of sigma^2 - q_i and how many were below zero; hfmi_op_kernel_cov_interp_diag: q and delta themselves, N doubles each
 *     in point order (either pointer may be NULL).  LIFETIME as hfmi_op_compose3's parts: the grid operator is referred to, not owned
 *     or copied, and must outlive this operator; the weights, delta and the work block are this operator's own.
 *       hfmi_interp_sampler_draw: column j of Y (+)= draw first_sample + j,  W z + sqrt(delta) eta:  z is that draw of
 *     hfmi_grid_sampler_draw(grid_sampler, ., seed, .) -- the sampler must have been made from the grid operator -- and eta the probe
 *     draw's Philox / Box-Muller (hfmi_randn_fill's element map) with key seed ^ 0x9E3779B97F4A7C15, stream 0 and vector index
 *     first_sample + j (the draw's number, not the column's position).  The key is not the grid noise's, so eta and z are independent.
 *     first_sample even, as for the grid sampler; chunks first_sample = 0, n, 2 n, ... (n even) reproduce one large call bit for bit.
 *     Y is const as a HANDLE, as in hfmi_grid_sampler_draw.  Block storage contract as every operator: padding rows untouched,
 *     accumulate adds, views stay in bounds (tests/test_gpu_grid_interp.py).
 *     HFMI_ERR_INVALID: d outside 1..3, n[c] < 4 or > 2^23, more than 2^40 nodes, h[c] <= 0 or not finite, origin not finite, N < 1, a point
 *     that is not finite or has u outside [1, n - 2] (the message names the point and the axis), transpose or diag_correction outside
 *     0 / 1; a grid operator that is no grid covariance, has a node map or a nugget; a negative nugget; a sampler of another covariance;
 *     first_sample odd, negative or past the 2^32 draws of a seed; at apply, blocks of another length. */
HFMI_API int hfmi_grid_interp_weights(int d, const int64_t* n /* d */, const double* h /* d */, const double* origin /* d */,
                                      const double* host_points /* N x d */, int64_t N, int64_t* base /* N */, double* w /* N d 4 */,
                                      int64_t* cell_start_or_null, int64_t* perm_or_null);
HFMI_API int hfmi_op_grid_interp(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */, const double* origin /* d */,
                                 const double* host_points /* N x d */, int64_t N, int transpose /* 0: W | 1: W^T */, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_interp(hfmi_op* grid_cov_op, const double* origin /* d */, const double* host_points /* N x d */, int64_t N,
                                       double nugget, int diag_correction /* 0 | 1 */, hfmi_op** out);
HFMI_API int hfmi_op_kernel_cov_interp_info(const hfmi_op* op, double* diag_min, double* diag_max, int64_t* n_diag_clipped);
HFMI_API int hfmi_op_kernel_cov_interp_diag(const hfmi_op* op, double* host_q_or_null /* N */, double* host_delta_or_null /* N */);
HFMI_API int hfmi_interp_sampler_draw(hfmi_op* op, hfmi_grid_sampler* grid_sampler, const hfmi_block* Y, uint64_t seed,
                                      int64_t first_sample /* even */, int accumulate);
/*     the FACTOR of that covariance,  K = F F^T  with  F = [ W S | diag(sqrt(delta)) ]  of shape N x (Ptot + N):  S is the factor of the
 *     sampler's embedding as in hfmi_op_grid_factor (Cg = S S^T, Ptot = prod P_c), so F F^T = W S S^T W^T + diag(delta) is K up to rounding
 *     for a definite sampler and K + W E W^T for a clipped one, |E_ij| <= cov_error_bound and hence |W E W^T|_ij <= 1.25^(2 d)
 *     cov_error_bound (the four Keys weights of an axis have 1-norm 1 + t (1 - t) <= 1.25).  What hands the caller's noise to a prior
 *     over scattered points: m = mean + F xi, and the whitened Hessian F^T H F.
 *       NOISE LAYOUT (part of the contract): rows 0 .. Ptot - 1 of a noise vector are the padded-grid noise in hfmi_op_grid_factor's
 *     natural order (entry e = s0 + P0 (s1 + P1 s2)); rows Ptot .. Ptot + N - 1 hold one entry per point in POINT order -- the order of
 *     host_points, not the binned order the device keeps internally.
 *       hfmi_op_interp_factor: transpose = 0 is F (blocks of length Ptot + N -> N), 1 is F^T (N -> Ptot + N).  F: the grid factor from a
 *     view of the first Ptot rows into the interpolated operator's work block, then one gather whose epilogue adds sqrt(delta_i)
 *     Xi[Ptot + i] by one fused multiply-add.  F^T: one spread into the work block, the transposed grid factor into a view of the first
 *     Ptot rows, and the tail Z[Ptot + i] (+)= sqrt(delta_i) X[i] by a streaming kernel of one multiplication per entry (the product is
 *     rounded before an accumulating apply adds it).  Both work chunk by chunk of the work block, an even number of columns (2
 *     "fftcov_pairs" columns when that key is set), so the pairs the grid factor forms are those of one call: no chunking changes a bit,
 *     and two applies are bit-identical.  Block storage contract as every operator; zero columns is a no-op.  Creation makes the
 *     sampler's root table if no factor of the sampler made it before, and sqrt(delta) in point order in the interpolated operator's
 *     state; neither changes a bit of the sampler's draws or of the operator's applies.  Samplers of either route are taken.
 *     LIFETIME: the sampler's state is shared as by hfmi_op_grid_factor (the sampler may be destroyed first); the interpolated operator
 *     is referred to, not owned or copied, and must outlive this operator, as its grid operator must outlive it.
 *     HFMI_ERR_INVALID: an operator that is not one of hfmi_op_kernel_cov_interp, a sampler of another context or not made from that
 *     operator's grid covariance, transpose outside 0 / 1; at apply, blocks of another length (the message names F or F^T and the four
 *     lengths). */
HFMI_API int hfmi_op_interp_factor(hfmi_op* interp_cov_op, hfmi_grid_sampler* grid_sampler, int transpose /* 0: F | 1: F^T */,
                                   hfmi_op** out);
/*     WHITTLE-MATERN PRIORS ON A BOX by DCT and FFT (hfmi_boxcov.hip): the SPDE prior (delta - gamma div Theta grad)^(-alpha) on a regular
 *     grid of d = 1, 2 or 3 axes (axis 0 fastest, node g = i0 + n0 (i1 + n1 i2)) with axis-aligned Theta = diag(theta) and, per axis, a
 *     NEUMANN side (n_c <= 2049; line length P_c = 2 (n_c - 1), 1 for one node; quadrature
 *     weight w = h_c, halved at the two end nodes, 1 for one node; mode k = 0 .. n_c - 1 at the angle t_k = pi k / (n_c - 1)) or a
 *     PERIODIC one (n_c <= 4096; P_c = n_c, w = h_c; mode k at t_k = 2 pi k~ / n_c with the signed k~ = k up to n_c / 2 and
 *     k - n_c above).  THE RULE OF AN AXIS: its line length P_c is a power of two (Neumann 1 or 2^m + 1 nodes, periodic 2^m), or a
 *     multiple of 4 with no prime factor but 2, 3 and 5 (a mixed-radix line: Neumann 7, 11, 13, 25, 49, 97, 101, 193, 201, 385 ... nodes,
 *     periodic 12, 20, 24, 48, 96, 100, 192 ...); every other n_c is refused, a line that is no multiple of 4 included (Neumann 4, 6, 8
 *     nodes; periodic 6, 18).  Cosine and Fourier transforms diagonalise it:  lambda_k = (delta + gamma sum_c theta_c mu_c(k_c))^(-alpha)  with
 *     mu_c = (2 - 2 cos t_k) / h_c^2 (symbol HFMI_BOX_SYMBOL_FD, the two-point stiffness with lumped mass; evaluated as
 *     (2 sin(t_k / 2) / h_c)^2) or (t_k / h_c)^2 (HFMI_BOX_SYMBOL_CONTINUOUS).  With W = diag(prod_c w_c) and
 *       T_s x = restrict( IFFT_unnormalised( (lambda^s / prod P_c) . FFT( extend(x) ) ) ),
 *     extend the even mirror of every Neumann axis (position P - j takes x_j, 1 <= j <= n - 2) and restrict the first n_c positions,
 *     hfmi_op_box(box, s, a, b) is the N x N operator  W^a T_s W^b:  the covariance of the nodal values C = T_1 W^-1 (s, a, b = 1, 0, -1),
 *     the precision R = C^-1 = W T_-1 (-1, 1, 0), the factor S = T_1/2 W^-1/2 with S S^T = C (1/2, 0, -1/2), S^T = W^1/2 T_1/2 W^-1
 *     (1/2, 1/2, -1) and the whitening S^-1 = W^1/2 T_-1/2 (-1/2, 1/2, 0) -- all exact up to rounding, nothing grown, clipped or
 *     iterated.  With the fd symbol R = A W^-1 A, A = delta W + gamma K, K the tensor sum of the 1-D two-point stiffness matrices: on
 *     Neumann sides and alpha = 2 the BiLaplacian prior on a tensor grid with lumped mass.
 *     Applied through hfmi_op_apply: 2 d - 1 passes of k_boxcov_pass (a power-of-two line) or k_boxcov_pass_mr (a mixed-radix line:
 *     radix-3 and radix-5 stages before the radix-4 / radix-2 ones) per pair of columns over a work buffer of N complex entries per
 *     pair (the rules: csrc/hfmi_boxcov_plan.h), two real columns per complex transform (a last odd column pairs with zeros), chunked
 *     by "fftcov_pairs" with identical bits; no atomics, two applies are bit-identical; block storage contract as every operator
 *     (padding rows untouched, accumulate adds).  The table lambda^s / prod P_c is made once per operator.  The operator shares the
 *     box's state: either may be destroyed first.  hfmi_box_spectrum: the N eigenvalues lambda_k in natural mode order,
 *     entry k0 + n0 (k1 + n1 k2), computed on the host.  hfmi_boxcov_plan_predict: the apply's launch plan without a device;
 *     words[HFMI_BOXCOV_PLAN_WORDS]:  0 d  1-3 n_c  4 N  5 pairs  6 pairs per chunk  7 chunks  8 passes  9 bytes of work buffer per pair
 *     10 entries of the power-of-two lines' twiddle table  11 the largest power-of-two P_c (1 when there is none)  12 static LDS of the
 *     pass kernels  13-15 P_c; then 16 words per pass from word 16:  axis, flags (as
 *     hfmi_fftcov_plan_predict), line length, mirror, extent n_axis, line stride, line span, lines, lines per workgroup, LDS line
 *     stride, threads, dynamic LDS, static + dynamic LDS, grid x, radix-3 stages, radix-5 stages (both 0: a power-of-two line); line l
 *     starts at entry (l mod stride) + (l div stride) span.
 *     HFMI_ERR_INVALID: d outside 1..3; an n_c outside the rules above; a boundary or a symbol that is none of the constants; h, gamma,
 *     delta, alpha or a theta that is not positive and finite (theta NULL = all ones); powers that are not finite; a pass that cannot
 *     be launched; at apply, blocks of another length.  A failed create frees everything, *out untouched. */
#define HFMI_BOX_NEUMANN 0
#define HFMI_BOX_PERIODIC 1
#define HFMI_BOX_SYMBOL_FD 0
#define HFMI_BOX_SYMBOL_CONTINUOUS 1
#define HFMI_BOXCOV_PLAN_WORDS 96
HFMI_API int hfmi_box_create(hfmi_ctx* ctx, int d, const int64_t* n /* d */, const double* h /* d */, const int* boundary /* d */, double gamma,
                             double delta, double alpha, const double* theta_or_null /* d */, int symbol, hfmi_box** out);
HFMI_API int hfmi_box_destroy(hfmi_box* box);
HFMI_API int hfmi_box_spectrum(const hfmi_box* box, double* host_lambda /* N */);
HFMI_API int hfmi_op_box(hfmi_box* box, double s, double a, double b, hfmi_op** out);
HFMI_API int hfmi_boxcov_plan_predict(int d, const int64_t* n, const int* boundary, int nvec, int64_t budget_bytes, int64_t* words);
/*     low-rank factor of that covariance WITHOUT any apply: the greedy (diagonally pivoted) partial Cholesky factorisation
 *     C ~= L L^T (hfmi_pchol.hip).  It reads the diagonal of C and the pivot columns only -- N k^2 flops and 4 N k^2 bytes for rank k,
 *     against 2 N^2 k flops per apply -- and returns the trace of the residual C - L L^T after every step; the residual is positive
 *     semidefinite, so trace[rank] bounds the error of every eigenvalue of L L^T.  With d0 = sigma^2 + nugget and kmax = min(max_rank, N):
 *       step j: (p, dp) = the largest remaining diagonal entry, ties to the LOWEST index; stop when trace[j] <= rel_tol * trace[0]
 *       (REL_TOL) or dp <= 4 kmax eps d0 (FLOOR: what is left is rounding); L[:,j] = (C[:,p] - L[:,:j] L[p,:j]^T) / sqrt(dp).
 *     hfmi_pchol_create runs the factorisation (the operator's coordinates are needed only here: the factor does not depend on the
 *     operator's lifetime).  No atomics: two factorisations of the same input are bit-identical in L, pivots and trace.
 *     hfmi_pchol_read: the `rank` pivots and the rank + 1 traces.  hfmi_pchol_factor: the factor as a block of `rank` vectors of
 *     length N, owned by the handle, read-only, valid until hfmi_pchol_destroy; it obeys the block storage contract (allocated like
 *     hfmi_block_create; rows N..ld-1 are +0.0, only rows below N are written); HFMI_ERR_INVALID when rank is 0.
 *     HFMI_ERR_INVALID: not a kernel covariance operator, max_rank < 1 or > 16384 (the largest Gram eigenproblem,
 *     hfmi_block_gram_eig), rel_tol negative or not finite. */
#define HFMI_PCHOL_MAX_RANK 0
#define HFMI_PCHOL_REL_TOL 1
#define HFMI_PCHOL_FLOOR 2
HFMI_API int hfmi_pchol_create(hfmi_op* kernel_cov_op, int max_rank, double rel_tol, hfmi_pchol** out);
HFMI_API int hfmi_pchol_info(const hfmi_pchol* f, int* rank, int* stop_reason, double* trace0);
HFMI_API int hfmi_pchol_read(const hfmi_pchol* f, int64_t* host_pivots, double* host_trace);
HFMI_API int hfmi_pchol_factor(const hfmi_pchol* f, const hfmi_block** L);
HFMI_API int hfmi_pchol_destroy(hfmi_pchol* f);
/* a4/a9: sparse operator  Y = M W  (prior.M.mult, prior.R.mult; hp.MatMvMult(B, decoder, encoder)) */
HFMI_API int hfmi_op_csr(hfmi_ctx* ctx, const hfmi_csr* M, hfmi_op** out);
/*     solver object for an SPD CSR matrix: Y = M^{-1} W to a relative residual rel_tol per vector
 *     (prior.Msolver behind hp.Solver2Operator, KLEProjector.py:163-164).  Jacobi-preconditioned
 *     Chebyshev iteration on a row-major copy of the block (one kernel per step, no inner products;
 *     the spectrum of D^-1 M is bracketed once per matrix: Gershgorin + the Lanczos matrix of one
 *     scalar CG run); Jacobi-preconditioned block CG when that bracket is too wide or does not
 *     deliver the tolerance. */
HFMI_API int hfmi_op_csr_pcg(hfmi_ctx* ctx, const hfmi_csr* M, double rel_tol, int max_iter, hfmi_op** out);
/*     what the last solve of such an operator did: steps taken, method (0 block CG, 1 Chebyshev, 2 AMG-CG),
 *     and the bracket of the spectrum of D^-1 M in use (0, 0: none) */
HFMI_API int hfmi_op_solver_info(const hfmi_op* op, int* iterations, int* method, double* lmin, double* lmax);
/*     algebraic multigrid for an SPD CSR matrix A (hippylib BiLaplacianPrior.Asolver: PETSc CG with amg_method(),
 *     rel_tol 1e-12; prior.Rsolver = A^-1 M A^-1 costs two such solves per apply, activeSubspaceProjector.py:447-453,
 *     KLEProjector.py:163-168).  The smoothed-aggregation hierarchy is built on the host (hippyflow_amd/amg.py) and
 *     handed over level by level; the CSR matrices are NOT copied or owned and must outlive the hierarchy.
 *     create: level 0 = A, smoothed by a Chebyshev polynomial of `degree` on [lmin, lmax] of D^-1 A;
 *     add_level: P (n_fine x n_c) from the new level to the current coarsest one, R = P^T (explicit), A_c = P^T A P and
 *       its own Chebyshev interval (unused when it stays the coarsest level);
 *     set_coarse: host n x n row-major inverse of the coarsest matrix (dense solve there); completes the hierarchy. */
HFMI_API int hfmi_amg_create(hfmi_ctx* ctx, const hfmi_csr* A, double lmin, double lmax, int degree, hfmi_amg** out);
HFMI_API int hfmi_amg_add_level(hfmi_amg* amg, const hfmi_csr* P, const hfmi_csr* R, const hfmi_csr* Ac, double lmin, double lmax);
HFMI_API int hfmi_amg_set_coarse(hfmi_amg* amg, int n, const double* host_inv);
HFMI_API int hfmi_amg_info(const hfmi_amg* amg, int* levels, int64_t* rows, int max_levels);
HFMI_API int hfmi_amg_destroy(hfmi_amg* amg);
/*     X = V B: one symmetric V-cycle on a block (the preconditioner; a test hook) */
HFMI_API int hfmi_amg_vcycle(hfmi_amg* amg, const hfmi_block* B, hfmi_block* X);
/*     solver operator Y = A^-1 W: block CG with the V-cycle as preconditioner, per-vector recurrences, until every
 *     vector's residual (the true one, checked at the end) is at most rel_tol times its right-hand side.  Errors:
 *     HFMI_ERR_NUMERIC (non-finite input, p.Ap <= 0 or r.z <= 0: not SPD), HFMI_ERR_NOT_CONVERGED (max_iter),
 *     HFMI_ERR_INVALID (shapes); Y is zero-filled on error.  hfmi_op_solver_info: method 2, lmin = lmax = 0.
 *     The operator does not own the hierarchy. */
HFMI_API int hfmi_op_amg_pcg(hfmi_ctx* ctx, hfmi_amg* amg, double rel_tol, int max_iter, hfmi_op** out);
/*     Y = c (b (a W))  (MassPreconditionedCovarianceOperator M C M, KLEProjector.py:47-69) */
HFMI_API int hfmi_op_compose3(hfmi_ctx* ctx, hfmi_op* a, hfmi_op* b, hfmi_op* c, hfmi_op** out);
/*     host black box (FEniCS PDE solves, sparse LU ...): W and Y in HFMI_LAYOUT_VECTORS
 *     (k, N) host arrays; return non-zero to abort.  This is how any object with the
 *     reference's mult/matMvMult protocol plugs into the device solve. */
typedef int (*hfmi_host_apply_fn)(void* user, const double* W_host, double* Y_host, int64_t N, int k);
HFMI_API int hfmi_op_host_callback(hfmi_ctx* ctx, hfmi_host_apply_fn fn, void* user, int64_t N, hfmi_op** out);
/*     For a callback that treats the vectors independently (a sparse-LU / Krylov solve per vector: prior.Rsolver,
 *     activeSubspaceProjector.py:447-450; prior.Msolver): invoke it on slabs of `vectors` vectors.  The slabs go
 *     through pinned double buffers and the device->host copy of slab i+1 and the host->device copy of slab i-1
 *     overlap the host work on slab i.  0 (default) = one call with the whole block. */
HFMI_API int hfmi_op_host_set_chunk(hfmi_op* op, int vectors);
/*     average of a device operator over the ranks of a communicator is done by the
 *     caller between applies (CollectiveOperator, collectiveOperator.py:31-38): a
 *     post-apply hook called with the result block, e.g. an RCCL all-reduce. */
typedef int (*hfmi_post_apply_fn)(void* user, hfmi_block* Y);
HFMI_API int hfmi_op_set_post_apply(hfmi_op* op, hfmi_post_apply_fn fn, void* user);
/*     the same average done natively: the result block of every apply (and the k x k Rayleigh quotient of the
 *     Gram-form solves) is all-reduced over `comm` on the context's stream, no host code inside the solve.
 *     reduce_op HFMI_REDUCE_SUM | HFMI_REDUCE_AVG; comm NULL detaches. */
HFMI_API int hfmi_op_set_collective(hfmi_op* op, hfmi_comm* comm, int reduce_op);
HFMI_API int hfmi_op_apply(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, int accumulate);
HFMI_API int hfmi_op_destroy(hfmi_op* op);

/* ---------------------------------------------------------------- communicator
 * The reference's sample-parallel collective (hippyflow/collectives/collective.py): one process per GPU.
 *   _allReduce_array, collective.py:61-71          -> hfmi_allreduce_host
 *   allReduce of a MultiVector, :98-111 (k Allreduce calls of length N, through host copies)
 *                                                   -> hfmi_allreduce: ONE RCCL all-reduce of the N x k block in
 *                                                      HBM on the context's stream, 1/P of 'avg' fused (ncclAvg)
 *   bcast of a MultiVector, :144-152 (k Bcast calls) -> hfmi_bcast
 *   comm.Get_size / Get_rank, :52-58                -> hfmi_comm_info
 * Bootstrap: rank 0 calls hfmi_comm_unique_id and ships the HFMI_UNIQUE_ID_BYTES bytes to the other ranks (any
 * channel: mpi4py bcast, a file -- hfmi_comm_init_from_file does the file exchange itself); every rank then calls
 * hfmi_comm_init_rank with its own context.  Transports (hfmi_comm_info): 1 = RCCL over xGMI (each rank its own
 * GPU), 2 = direct peer access through HIP IPC staging buffers (ranks sharing a GPU, or HFMI_COMM_TRANSPORT=p2p),
 * 0 = host-only (ctx NULL on every rank: host payloads and barriers only).  Ranks of one communicator live on one
 * node unless HFMI_COMM_TRANSPORT=rccl.  A peer that never arrives fails the call after HFMI_COMM_TIMEOUT_S
 * (300 s) with HFMI_ERR_COMM instead of hanging.  The transport is agreed among the ranks: if librccl does not load,
 * ncclCommInitRank fails or the first all-reduce does not give the right sum on ANY rank, ALL ranks use the p2p
 * transport (which works across GPUs through HIP IPC and is stream-ordered: counters in the node segment, written and
 * polled from the GPUs; HFMI_P2P_SYNC=host|stream overrides the choice).  The id file of hfmi_comm_init_from_file is
 * created 0600 with O_EXCL, read only if it is this user's, and removed before any rank returns. */
#define HFMI_UNIQUE_ID_BYTES 256
#define HFMI_REDUCE_SUM 0
#define HFMI_REDUCE_AVG 1
#define HFMI_REDUCE_MAX 2
HFMI_API int hfmi_comm_unique_id(void* id_out);
HFMI_API int hfmi_comm_init_rank(hfmi_ctx* ctx_or_null, const void* id, int nranks, int rank, hfmi_comm** out);
HFMI_API int hfmi_comm_init_from_file(hfmi_ctx* ctx_or_null, const char* path, int nranks, int rank, hfmi_comm** out);
HFMI_API int hfmi_comm_info(const hfmi_comm* comm, int* nranks, int* rank, int* transport);
/* one line of JSON: the transport, WHY it was chosen (e.g. "fell back from rccl: the first ncclAllReduce failed on rank 3;
 * all ranks agreed on p2p"), the RCCL library in use, every rank's PCI bus id, how the p2p path synchronises */
HFMI_API int hfmi_comm_describe(const hfmi_comm* comm, char* buf, int len);
/* the transport decision as a pure function of the table the ranks publish (test hook for the CPU suite): has_device[p],
 * rccl_ok[p], device_ids[p] for p < nranks; *transport = 0 host / 1 rccl / 2 p2p, or -1 for an inconsistent table */
HFMI_API int hfmi_comm_decide_transport(int nranks, const int* has_device, const int* rccl_ok, const char* const* device_ids,
                               int force_p2p, int* transport, char* reason, int reason_len);
HFMI_API int hfmi_comm_barrier(hfmi_comm* comm);               /* drains the context's stream, then meets the other ranks */
HFMI_API int hfmi_allreduce(hfmi_comm* comm, hfmi_block* Y, int reduce_op);           /* in place, stream-ordered */
HFMI_API int hfmi_bcast(hfmi_comm* comm, hfmi_block* Y, int root);
HFMI_API int hfmi_allreduce_host(hfmi_comm* comm, double* v, int64_t count, int reduce_op);   /* in place */
HFMI_API int hfmi_bcast_host(hfmi_comm* comm, void* v, int64_t nbytes, int root);
HFMI_API int hfmi_comm_destroy(hfmi_comm* comm);

/* ---------------------------------------------------------------- QR (a7)
 * MultiVector.orthogonalize() / Borthogonalize(B): thin QR with Q^T B Q = I,
 * R upper triangular with positive diagonal (unique, so Q equals the
 * reference's MGS Q to round-off).  B, BQ, host_R may be NULL.
 * method: HFMI_QR_CHOL = (shifted) Cholesky-QR, repeated until orthonormal;
 *         HFMI_QR_MGS  = column-by-column Gram-Schmidt with the reference's
 *         Rutishauser re-orthogonalisation test (dependent columns zeroed).
 * Cholesky-QR (CHOL, AUTO) takes up to 2048 vectors: up to 256 the k x k factorisation runs on one compute unit, from 257 on
 * (tuning key "qr_wide_min") it is a blocked factorisation over the whole GPU with Q <- Q R^-1 formed out of place in a cached
 * temporary.  MGS has no width limit. */
#define HFMI_QR_CHOL 0
#define HFMI_QR_MGS 1
#define HFMI_QR_AUTO 2 /* CHOL, falling back to MGS on breakdown */
HFMI_API int hfmi_borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, int method, int* passes);

/* ---------------------------------------------------------------- Rayleigh-Ritz (a8)
 * np.linalg.eigh(T) + descending sort: symmetric k x k (host, row-major; the
 * symmetric part is used), eigenvalues descending, eigenvectors in the columns of V
 * (row-major k x k).  sort_by_abs is a flag word: bit 0 = order by |d|; bit 1 = HFMI_EIG_JACOBI.
 * k <= 256, default: Householder tridiagonalisation + divide and conquer on one compute unit
 * (hfmi_eig_dc.hip) -- the algorithm family of the LAPACK routine behind np.linalg.eigh, absolute
 * accuracy eps ||T||.  HFMI_EIG_JACOBI: one-workgroup parallel cyclic Jacobi in LDS (slower; small
 * eigenvalues of graded positive definite matrices to high RELATIVE accuracy).
 * 256 < k <= 16384 (the n x n Gram problem of the deterministic POD, la.eigh at PODProjector.py:821, any number of
 * snapshots): the same algorithm family over the whole GPU (hfmi_eig_blocked.hip) -- panel Householder
 * tridiagonalisation with the trailing update on the fp64 MFMA, divide and conquer with the leaves on one compute unit
 * each and the upper merges on all of them, block-reflector back-transformation.  Non-finite entries: HFMI_ERR_NUMERIC
 * (np.linalg.eigh raises LinAlgError).  HFMI_EIG_LARGE=jacobi in the environment selects the two-sided Jacobi of
 * rounds 2-4 (hfmi_eig_large.hip; up to 4096). */
#define HFMI_EIG_SORT_ABS 1
#define HFMI_EIG_JACOBI 2
HFMI_API int hfmi_sym_eig_small(hfmi_ctx* ctx, const double* host_T, int k, int sort_by_abs, double* host_d,
                       double* host_V);
/* The same with only the nvec leading eigenvectors (in output order) returned; host_V is k x nvec row-major.  What the
 * deterministic POD uses of la.eigh(G): U[:, :u_rank] (PODProjector.py:821-826).  Beyond 256 the back-transformation and
 * the read-back run over nvec columns instead of k. */
HFMI_API int hfmi_sym_eig_leading(hfmi_ctx* ctx, const double* host_T, int k, int sort_by_abs, int nvec, double* host_d,
                         double* host_V);
/* la.eigh(X^T (M X)) of the deterministic POD in one call (PODProjector.py:818-826: UtMU = u_data @ M @ u_data.T, eigh,
 * U[:, :u_rank]): the n x n Gram matrix of two blocks of n vectors is formed on the device and handed to the
 * eigensolver there; host_d receives the n eigenvalues, host_V the nvec leading eigenvectors (n x nvec row-major). */
HFMI_API int hfmi_block_gram_eig(const hfmi_block* A, const hfmi_block* B, int sort_by_abs, int nvec, double* host_d,
                        double* host_V);

/* np.linalg.svd(R) of the small factor inside hp.accuracyEnhancedSVD (activeSubspaceProjector.py:813-834,1026):
 * R (host, k x k row-major) = U diag(sigma) V^T, sigma descending; U, V row-major k x k (columns = vectors).
 * One-workgroup one-sided Jacobi in LDS (full relative accuracy of small singular values), scaled by a power of two on
 * entry: 2^e R returns the same U, V and 2^e sigma.  V is orthogonal always; the column of U of an exactly zero
 * singular value is zero.  HFMI_ERR_NUMERIC for non-finite input. */
HFMI_API int hfmi_svd_small(hfmi_ctx* ctx, const double* host_R, int k, double* host_sigma, double* host_U, double* host_V);

/* ---------------------------------------------------------------- full solves (a5, a6)
 * hp.doublePass(A, Omega, r, s) / hp.doublePassG(A, B, Binv, Omega, r, s):
 * Omega has k >= r vectors and is not modified; on return host_d[r] holds the
 * eigenvalues (descending) and U (r vectors) the (B-)orthonormal eigenvectors.
 * Everything stays on the device between the first apply and the final U.
 * flags: bit 0 = sort by |d|;  bit 1 = use HFMI_QR_MGS;  bit 3 = Jacobi instead of divide and conquer for the
 * k x k Rayleigh-Ritz problem;  bit 2 = form T = (A Q)^T Q literally (by default, for
 * operators of Gram form A = scale X^T Gamma X the same matrix is formed as scale (X Q)^T Gamma (X Q), which skips
 * the second N x k block product and shrinks the rank average of that pass to k x k).
 * k <= 2048.  Beyond 256 probe vectors the operators are applied in column panels of at most 256, T is always the literal
 * (A Q)^T Q (bit 2 is implied) and the Rayleigh-Ritz problem goes to the whole-GPU eigensolver of hfmi_sym_eig_small (bit 3 is
 * ignored). */
HFMI_API int hfmi_double_pass(hfmi_op* A, const hfmi_block* Omega, int r, int s, int flags, double* host_d,
                     hfmi_block* U);
HFMI_API int hfmi_double_pass_g(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s,
                       int flags, double* host_d, hfmi_block* U);

/* hp.singlePass(A, Omega, r, s) / hp.singlePassG(A, B, Binv, Omega, r, s) (hippylib randomizedEigensolver): the same
 * contract as hfmi_double_pass[_g], but the operator is applied s times instead of s + 1.  X_0 = Omega,
 * X_i = (B^-1) A X_{i-1}; with P = X_{s-1}, Y = X_s, Ybar = A X_{s-1} (= Y without B) and Q = (B-)orth(Y):
 * Wt = P^T (B) Q, Zt = Ybar^T Q, T = sym(Wt^-1 Zt) (LU with partial pivoting on the device), eigh(T), U = Q V[:, :r].
 * flags: bit 0 = sort by |d|; bit 1 = HFMI_QR_MGS; bit 3 = Jacobi for the k x k eigenproblem (bit 2 does not apply).
 * A singular or non-finite Wt (rank-deficient sketch, e.g. dependent probe vectors) is HFMI_ERR_NUMERIC, never NaN
 * eigenpairs (hippylib's np.linalg.solve raises LinAlgError there).  A rank average attached to A applies to every
 * application, as in the double pass. */
HFMI_API int hfmi_single_pass(hfmi_op* A, const hfmi_block* Omega, int r, int s, int flags, double* host_d, hfmi_block* U);
HFMI_API int hfmi_single_pass_g(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                       double* host_d, hfmi_block* U);
/* The single-pass core on a sketch the caller already holds (the Wt / Zt / eigh steps of hp.singlePass[G]):
 * P and Y (N x k) as above, none modified; Ybar and B both NULL for the standard problem, both given for the
 * generalized one (Y = B^-1 Ybar).  Used by streamed sketches, where Y = A Omega is summed while the samples arrive. */
HFMI_API int hfmi_sketch_eig(const hfmi_block* P, const hfmi_block* Y, const hfmi_block* Ybar, hfmi_op* B, int r, int flags,
                    double* host_d, hfmi_block* U);
/* np.linalg.solve(W, Z) inside hp.singlePass[G], on the device (kernel tests): W, Z, X host row-major m x m, m <= 256.
 * HFMI_ERR_NUMERIC for a singular W (min |pivot| <= m eps max |pivot|) or non-finite input. */
HFMI_API int hfmi_small_solve(hfmi_ctx* ctx, const double* host_W, const double* host_Z, int m, double* host_X);

/* ---------------------------------------------------------------- instrumentation
 * Kernel-level entry points used by bench.py / the parity tests:
 *   C (nvecA x nvecB, device partial-summed, returned on host) = A^T B with an explicit split count
 *   (0 = library default) and the average kernel time of `reps` back-to-back launches. */
HFMI_API int hfmi_bench_tsgemm_tn(const hfmi_block* A, const hfmi_block* B, int nsplit, int reps, double* host_C,
                         double* avg_ms);
HFMI_API int hfmi_bench_tsgemm_nn(const hfmi_block* A, const double* host_S, hfmi_block* Y, int reps, double* avg_ms);
/* The tn product with its whole argument list, for the instance sweep of the tests: C = scale A^T B + beta C on a device copy of
 * the caller's host array.  colmajor = 0: host_C is nvecA rows of ldc >= nvecB doubles, element (i, j) at [i ldc + j];
 * colmajor = 1: nvecB rows of ldc >= nvecA doubles, element (i, j) at [j ldc + i] (ldc > 1: a result with both strides 1 is
 * row-major).  The WHOLE array goes up (the beta operand and the guard columns behind the fast extent) and comes
 * back, so the caller sees the result and everything the launch wrote next to it.  nsplit: 0 = library default. */
/* The k x k Cholesky factorisation with inverse behind the wide Cholesky-QR (256 < k <= 2048; any 1 <= k <= 2048 is accepted) on
 * a host matrix (tests): G = R^T R with the library's shift / breakdown rule (shift_rel * trace(G) on the diagonal after a pivot
 * below pivot_tol * G_jj; pivot_tol <= 0: 64 k eps).  host_G, host_R, host_Rinv: k x k row-major; host_status[4] =
 * min pivot ratio, || D^-1/2 G D^-1/2 - I ||_F, shifted, failed (R and R^-1 are zero filled when failed). */
HFMI_API int hfmi_test_chol_wide(hfmi_ctx* ctx, int k, const double* host_G, double shift_rel, double pivot_tol, double* host_R,
                                 double* host_Rinv, double* host_status);
/* The LU solve kernel behind hfmi_small_solve and the single pass with everything it leaves behind (tests): host_W, host_Z, host_X,
 * host_LU m x m row-major, m <= 256; host_LU is the factored working copy (L below the diagonal, U on and above it, rows in pivoted
 * order); host_status[3] = min |pivot|, max |pivot|, failed (0, or 1 / 2 / 3 as hfmi_small_solve reports them).  The status is
 * returned, never turned into an error.  want_T != 0: the kernel also writes T = (X + X^T) / 2 into the eigensolver's slot as the
 * single pass has it do, and host_T receives the whole mp x mp (mp = min(round_up(m, 16), 256), row-major) region of that slot,
 * which is filled with NaNs before the launch -- whatever the kernel does not write shows.  host_T may be NULL when want_T == 0. */
HFMI_API int hfmi_test_lu_solve(hfmi_ctx* ctx, const double* host_W, const double* host_Z, int m, int want_T, double* host_X,
                                double* host_LU, double* host_status, double* host_T);
HFMI_API int hfmi_test_tsgemm_tn(const hfmi_block* A, const hfmi_block* B, double scale, double beta, int colmajor, int ldc,
                                 int nsplit, double* host_C);
/* Ownership of device resources (tests).  Every device buffer, pinned buffer, event and stream of the library (the communicator's
 * excepted) is acquired and released in one place, which counts them per kind in that order (4 kinds), process-wide.
 * hfmi_test_own_fail: acquisitions first .. first + count - 1, counted from this call (the next one is number 1), return
 * hipErrorOutOfMemory without calling HIP; first = 0 disarms.  Nothing is launched and nothing faults: the failure is simulated on the
 * host.  hfmi_test_own_counts: live[4] = handles acquired and not yet released, acquired[4] = acquisitions that succeeded so far,
 * *pooled = storage of destroyed blocks the context keeps for reuse (counted in live[0] as well; 0 for a NULL context).  Any output
 * may be NULL. */
HFMI_API int hfmi_test_own_fail(int first, int count);
HFMI_API int hfmi_test_own_counts(hfmi_ctx* ctx_or_null, int64_t* live, int64_t* acquired, int64_t* pooled);
/* Plan record: every launch of a contraction kernel (k_tsgemm_tn, k_tsgemm_nn[_res], k_tsgemm_ss[b]) and of a partial-sum
 * reduction behind one appends HFMI_PLAN_WORDS ints to a ring of HFMI_PLAN_RING records on the context (host side, a few stores
 * per launch).  Word 0 is the kind, the others by kind:
 *   TN      MT, NT, WAVES, TR, R4, grid, nrb, nsplit, direct, tail_nrb, tail_nsplit
 *   NN      TT, NT, WAVES, R4, UPPER (0), msplit, full_tiles, tail_tiles, grid      (streaming kernel)
 *   NN_RES  TT, NT, WAVES (8), R4, UPPER, msplit (1), full_tiles (all), tail_tiles (0), grid
 *   SS      TPW, NQ, PF, swap (0), same, nsplit
 *   SSB     RT, CTL, NQ, PIPE, swap, same (0), nsplit
 *   REDUCE  route (HFMI_REDUCE_*), RY (4 | 16 split lanes; 0 for the vector kernel), nsplit, tr, m, k
 * hfmi_plan_clear empties the ring; hfmi_plan_read copies the records appended since (oldest first, at most max_records and at
 * most the HFMI_PLAN_RING newest) and stores how many launches there were in *total. */
#define HFMI_PLAN_WORDS 16
#define HFMI_PLAN_RING 256
#define HFMI_PLAN_TN 0
#define HFMI_PLAN_NN 1
#define HFMI_PLAN_NN_RES 2
#define HFMI_PLAN_SS 3
#define HFMI_PLAN_SSB 4
#define HFMI_PLAN_REDUCE 5
#define HFMI_REDUCE_VEC_LONG 0    /* k_reduce_vec over the m x ld array as one long row */
#define HFMI_REDUCE_VEC_ROWS 1    /* k_reduce_vec row by row */
#define HFMI_REDUCE_FLAT 2        /* k_reduce_flat<RY> */
#define HFMI_REDUCE_PARTIALS 3    /* k_reduce_partials<RY> */
HFMI_API int hfmi_plan_clear(hfmi_ctx* ctx);
HFMI_API int hfmi_plan_read(hfmi_ctx* ctx, int max_records, int* words /* max_records x HFMI_PLAN_WORDS */, int* nrecords, int* total);
/* The records a contraction of that shape would append, computed on the host by the planners the launchers call: no context and no
 * device.  kind TN: the m x k result of tsgemm_tn over the long axis N (its own kernels, in column panels of 256; the skinny route
 * is kind SS), addressed as C[i rs + j cs], with nsplit_req > 0 forcing the split; NN: Y (N x k) = A (N x m) S, hook_panels = most
 * row panels of an overlapped rank reduction (0: none, at most 8); SS: tsgemm_ss for m, k the shapes it accepts.  flags describe
 * what the dispatchers read off their pointers.  The knobs are the process's (hfmi_tuning_set), num_cus <= 0 stands for 256.
 * hook_rows (optional, 2 x max_records): first row and row count the row-panel hook is called with behind each record (0, 0: no
 * call).  *nrecords is the number of records of the plan; more than max_records is an error. */
#define HFMI_PREDICT_TN 0
#define HFMI_PREDICT_NN 1
#define HFMI_PREDICT_SS 2
#define HFMI_PREDICT_SAME 1        /* SS: one operand against itself */
#define HFMI_PREDICT_ALIASED 2     /* TN: C is one of the operands */
#define HFMI_PREDICT_UNALIGNED 4   /* TN, SS: C or the workspace is not 16-byte aligned */
#define HFMI_PREDICT_UPPER 8       /* NN: the caller marks the small matrix upper triangular (Q R^-1 of the QR) */
HFMI_API int hfmi_plan_predict(int kind, int m, int k, int64_t N, double scale, double beta, int64_t rs, int64_t cs, int nsplit_req,
                               int flags, int num_cus, int hook_panels, int max_records, int* words, int64_t* hook_rows, int* nrecords);
/* The launch plan of the whole-GPU symmetric eigensolver (hfmi_sym_eig_small / _leading, hfmi_block_gram_eig for 256 < n <= 16384) for
 * an n x n matrix of which nvec eigenvectors are wanted, computed on the host by the planner and the launch walk the solver itself
 * runs: no context and no device.  lds_per_block: LDS a workgroup may have on the device (static + dynamic; 163840 on an MI355X);
 * defl1_static_lds: static LDS of the solver's deflation kernel (4108).  The knobs are the process's (the HFMI_EIG_* environment
 * switches, read once).  Every output is zero-filled first.
 * scalars[HFMI_EIG_PLAN_SCALARS]:
 *    0 route: 1 = the blocked solver, 0 = n < 3 or the Jacobi route (nothing else is filled then)
 *    1 nr (rows of a column: n rounded up to 128)    2 ld (leading dimension)    3 npad (n rounded up to WY)
 *    4 WY (columns of a block reflector)    5 nblk (block reflectors)    6 npanels (64-column panels)    7 Lf (merge levels; 2^Lf leaves)
 *    8 vlen (elements of a workspace vector)    9 bytes of the workspace
 *   10 bytes the dynamic-LDS attribute of k_tri_b is raised to (0: not raised)
 *   11 j_unb: first column of the unblocked tail (-1: none)    12 panel columns    13 panel ends (rank-2k updates)
 *   14 mirror launches (k_mirror_lower)    15 rank-2k updates cut to the lower triangle    16 k_tri_tail launches
 *   17 largest ntiles of a k_tri_bs launch    18 largest npvy (partial sums of v . y a column leaves)
 *   19 largest nb (128-row slots of k_tri_bs)    20 largest npn (partial norms a column leaves)
 *   21, 22, 23 the knobs sym_min, unb_max, leaf_max as clamped
 * regions[4 x HFMI_EIG_PLAN_REGIONS], in layout order (the names: HFMI_EIG_REGIONS of csrc/hfmi_eig_plan.h):
 *   element (0 double, 1 int, 2 byte, 3 node record), count, byte offset, bytes
 * levels[4 x HFMI_EIG_PLAN_LEVELS], entry L < Lf = the merge level of 2^L nodes:
 *   cap (poles the deflation kernel is sized for), MODE (0 / 1 / 2), dynamic LDS bytes, 1 = the dynamic-LDS attribute is raised to them
 * walk[4 x HFMI_EIG_PLAN_INSTANCES], one entry per kernel instance of the tridiagonalisation, in the order k_tri_a<false>, <true>,
 * k_tri_b<4,8>, <8,8>, <8,16>, <8,32>, k_tri_bs<8>, <16>, <32>, k_tri_u<4>, <8>, <16>, <20>:
 *   launches, largest npn it is handed (k_tri_b, k_tri_bs), largest npvy it is handed (k_tri_a), largest dynamic LDS bytes */
#define HFMI_EIG_PLAN_SCALARS 24
#define HFMI_EIG_PLAN_REGIONS 47
#define HFMI_EIG_PLAN_LEVELS 7
#define HFMI_EIG_PLAN_INSTANCES 13
HFMI_API int hfmi_eig_plan_predict(int n, int nvec, int64_t lds_per_block, int64_t defl1_static_lds, int64_t* scalars, int64_t* regions,
                                   int64_t* levels, int64_t* walk);
/* The launch plan of one call of the one-compute-unit k x k stage (k <= 256: the Cholesky of every Cholesky-QR pass, the Rayleigh-Ritz
 * eigensolve, the SVD, the LU of the single pass), computed on the host by the planner the launcher itself asks
 * (csrc/hfmi_small_plan.h): no context and no device.  kind: HFMI_SMALL_PLAN_*; method (EIGH only): 1 = the caller asks for Jacobi.
 * knobs: HFMI_SMALL_KNOB_WORDS ints, or NULL for the process's own (environment read once, hfmi_tuning_set "chol" / "eig"):
 *    0 small_threads   1 chol_env (HFMI_CHOL=tile)   2 chol_generic   3 chol_tile   4 jacobi_db   5 jacobi_replay_lds
 *    6 eig_env (HFMI_EIG=jacobi)   7 tri_waves   8 dc_split_top   9 dc_timing   10 tuning key "chol" (-1: never set)   11 tuning key "eig"
 * words[HFMI_SMALL_PLAN_WORDS], zero-filled first:
 *    0 refusal (0: none; 1: k outside 1 .. 256; 2: Jacobi, no instance holds that many blocks per thread)    1 launches
 *    2 bytes of the workspace    3 regions of the workspace
 *    4 route (Cholesky: 1 = column-at-a-time kernels, 0 = blocked MFMA kernel; EIGH: 1 = Jacobi, 0 = divide and conquer)
 *    5 the working matrix is in LDS (column Cholesky, Jacobi, SVD)    6 Jacobi, SVD: k rounded up to even
 *    7 Jacobi: 2 x 2 blocks per thread; LU: panel width; blocked Cholesky: 16-row blocks
 *    8, 9, 10 divide and conquer: leading dimension of its matrices, tree levels, 1 = the last merge's product is k_dc_top's
 *   11 divide and conquer, bit 0: k_dc_top reads the second buffer, bit 1: the eigenvectors end in the second buffer, bit 2: timing
 *   12 ... 4 launches x 9, in launch order: kernel family (enum small_family of the header), four template parameters, threads, grid,
 *      dynamic LDS bytes, 1 = the dynamic-LDS attribute is raised to them
 *   48 ... 12 regions x 2, in layout order (HFMI_DC_REGIONS / HFMI_JACOBI_REGIONS of the header): byte offset, bytes
 *   72 ... the HFMI_SMALL_KNOB_WORDS knobs the plan was made with */
#define HFMI_SMALL_PLAN_CHOL 0
#define HFMI_SMALL_PLAN_EIGH 1
#define HFMI_SMALL_PLAN_SVD 2
#define HFMI_SMALL_PLAN_LU 3
#define HFMI_SMALL_KNOB_WORDS 12
#define HFMI_SMALL_PLAN_WORDS 84
HFMI_API int hfmi_small_plan_predict(int kind, int k, int method, const int* knobs, int64_t* words);
/* The rules of repeated Cholesky-QR (hfmi_borth_qr, the orthogonalisation inside the fused solves; csrc/hfmi_qr_rules.h) for given
 * values, from the functions the loops themselves ask: no context and no device.  policy: what the caller lets the loop leave
 * undone -- CHECKED: every pass's status words are read; DEFERRED: the last pass's R^-1 is left for the caller to fold in; TRUSTED:
 * deferred, and the first two passes' words are judged by the caller after the solve.  has_B: a B inner product (every pass is then
 * a checked one); trust_first: the tuning key "qr_trust_first"; pass: 0-based; first_clean: pass 0 was trusted or reported no shift;
 * failed, shifted, gram_dev: the status words of this pass (not read by the two TRUST issues; a NaN defect is "not yet orthonormal").
 * words[0] = how the pass is issued (HFMI_QR_ISSUE_*), words[1] = what follows from its status words (HFMI_QR_NEXT_*),
 * words[2] = 1 when a call of k vectors under that policy takes the wide arena at tuning key "qr_wide_min" = qr_wide_min. */
#define HFMI_QR_POLICY_CHECKED 0
#define HFMI_QR_POLICY_DEFERRED 1
#define HFMI_QR_POLICY_TRUSTED 2
#define HFMI_QR_ISSUE_TRUST_FIRST 0      /* status words to their own slot, apply R^-1, no read */
#define HFMI_QR_ISSUE_TRUST_SECOND 1     /* words and the R_jj / ||z_j|| table to pinned memory, stop with R^-1 deferred */
#define HFMI_QR_ISSUE_READ_THEN_APPLY 2  /* read the words, apply R^-1 only if another pass follows */
#define HFMI_QR_ISSUE_APPLY_THEN_READ 3  /* snapshot the words, apply R^-1, then read */
#define HFMI_QR_NEXT_FAIL_NOT_PD 0       /* HFMI_ERR_NUMERIC: not positive definite even after shifting */
#define HFMI_QR_NEXT_DONE 1
#define HFMI_QR_NEXT_DONE_DEFERRED 2
#define HFMI_QR_NEXT_AGAIN 3
#define HFMI_QR_NEXT_FAIL_MAX_PASSES 4   /* HFMI_ERR_NUMERIC: no convergence in 6 passes */
HFMI_API int hfmi_qr_rules_predict(int policy, int has_B, int trust_first, int pass, int first_clean, int failed, int shifted, double gram_dev,
                                   int k, int qr_wide_min, int* words /* 3 */);
/* The late verdict on a TRUSTED call of k <= 256 vectors: the second pass's words, the first pass's when first_trusted, and the table
 * norm[j] = ||z_j|| of the input column, rdiag[j] = R_jj of the accumulated factor (a column counts as dependent unless
 * R_jj > 100 eps ||z_j||).  *stands = 1: the result stands, 0: the solve is repeated on the checked path. */
HFMI_API int hfmi_qr_late_verdict_predict(int k, int failed2, int shifted2, double gram_dev2, int first_trusted, int failed1, int shifted1,
                                          const double* norm, const double* rdiag, int* stands);
/* The rules of the sparse SPD solves (hfmi_op_csr_pcg, the smoother of hfmi_amg_*; csrc/hfmi_spsolve_rules.h) for given values, from the
 * functions the drivers themselves ask: no context and no device.  [lmin, lmax]: the bracket of the spectrum of D^-1 A; rel_tol,
 * max_iter: the operator's; a Chebyshev step on nrows x k arrays, resid != 0: the residual launch.  knobs: 3 ints (HFMI_PCG,
 * HFMI_CHEB_THREADMAP as 0 / 1, HFMI_CHEB_UNR as the integer it was set to), or NULL for the process's own (environment read once).
 * coef (may be NULL when nsteps = 0): 2 + 2 nsteps doubles -- 1 / theta of the first step, 1.0 when the interval has a width
 * (lmax - lmin > 1e-12 (lmax + lmin)) else 0.0 (then no (c1, c2) is written), then (c1, c2) of steps 2, 3, ... of the three-term iteration.
 * words[HFMI_CHEB_RULES_WORDS]:
 *    0 planned steps   1 route: 0 = Chebyshev, 1 = this matrix is left to the block CG (planned > max_iter or > 200)
 *    2 rounds (each ends with a look at the true residual)   3 .. 6 steps of round 0 .. 3 (0: not run)
 *    7 step kernel: 1 = k_cheb_step_wave (one wave per row), 0 = k_cheb_step (one thread per entry)   8 rows per wave   9 workgroups
 *   10, 11, 12 the knobs the plan was made with (HFMI_CHEB_UNR: anything but 2 and 4 is 1) */
#define HFMI_CHEB_RULES_WORDS 13
HFMI_API int hfmi_cheb_rules_predict(double lmin, double lmax, double rel_tol, int max_iter, int64_t nrows, int k, int resid, const int* knobs,
                                     int nsteps, double* coef, int64_t* words);
/* The bracket the Chebyshev solve makes of one scalar Jacobi-CG run of m iterations: rz[i] = r.z before iteration i (m + 1 values, the
 * last one after the last iteration), pap[i] = p.Ap of iteration i; gersh_lmax: Gershgorin's bound on D^-1 A (0: none).
 * *refusal: 0 = none, 1 = no Gershgorin bound, 2 = p.Ap <= 0 or a non-finite r.z (not SPD), 3 = fewer than 3 iterations,
 * 4 = smallest Ritz value <= 0, 5 = largest below smallest.  values[4] (refusal 0, 4, 5): the Ritz values tmin, tmax of the Lanczos
 * matrix by Sturm bisection, and (refusal 0) the bracket lmin = 0.9 tmin, lmax = min(gersh_lmax, 1.05 tmax), never below tmax. */
HFMI_API int hfmi_lanczos_bracket_predict(int m, const double* rz, const double* pap, double gersh_lmax, int* refusal, double* values);
/* C (M x N) = op(A) op(B), column-major host operands with their natural leading dimensions (A: ta ? K x M : M x K; B: tb ? N x K : K x N),
 * on the general fp64 MFMA product of the eigensolver: the N x N x N congruence products of the deterministic POD's N-dimensional route
 * (la.eigh of PODProjector.py:812-833 reformulated in the state dimension when the snapshots outnumber it: hippyflow_amd/projectors.py) */
HFMI_API int hfmi_dense_matmul(hfmi_ctx* ctx, int M, int N, int K, int ta, int tb, const double* host_A, const double* host_B, double* host_C);
/* the general fp64 MFMA product inside the whole-GPU eigensolver (trailing rank-2k updates, Q S of the merges, block reflectors of
 * the back-transformation; la.eigh(G), PODProjector.py:812-833): C (M x N) = op(A) op(B), column-major host operands with their
 * natural leading dimensions, average kernel time of `reps` launches; host_C may be null */
HFMI_API int hfmi_bench_dgemm(hfmi_ctx* ctx, int M, int N, int K, int ta, int tb, int reps, const double* host_A, const double* host_B,
                     double* host_C, double* avg_ms);
/* What the general fp64 MFMA product does with a descriptor (csrc/hfmi_dgemm.h: gemm_desc, dgemm_route_make), computed on the host by
 * the function the launcher itself calls: no context and no device.  C (M x N) = alpha (op(A) op(B) + op(A2) op(B2)) + beta C with
 * reduction lengths K, K2, `batch` products with element strides sA, sB, leading dimensions lda, ldb; align_X = byte address of X
 * modulo 16 (0 or 8; A2 / B2 only count when K2 > 0); cut = the three triangular-cut bits; has_skip != 0: a device skip flag is
 * passed; pipelined = the process switch HFMI_EIG_GEMM (1 when unset, 0: the 64 x 64 kernel everywhere).
 * route[HFMI_DGEMM_ROUTE_WORDS]: kernel (HFMI_DGEMM_*), vec (pipelined kernels: 1 = 16-byte loads for interior tiles, else 0),
 * grid x, y, z, error (HFMI_DGEMM_ERR_*: the launcher returns HFMI_ERR_INVALID and launches nothing), two spare words (0).
 * kernel HFMI_DGEMM_NONE with error 0: M <= 0 or N <= 0, a no-op. */
#define HFMI_DGEMM_ROUTE_WORDS 8
#define HFMI_DGEMM_NONE (-1)
#define HFMI_DGEMM_K64 0          /* k_dgemm<TA, TB, false>: 64 x 64 tiles */
#define HFMI_DGEMM_K64_CUT 1      /* k_dgemm<false, TB, true>: triangular cuts and the skip flag */
#define HFMI_DGEMM_P128 2         /* k_dgemm_p<TA, TB, 128>: pipelined, 128 x 128 tiles */
#define HFMI_DGEMM_P64 3          /* k_dgemm_p<TA, TB, 64>: pipelined, 64 x 128 tiles */
#define HFMI_DGEMM_ERR_NONE 0
#define HFMI_DGEMM_ERR_K2_BATCH 1 /* a second product (K2 > 0) with batch > 1 */
#define HFMI_DGEMM_ERR_CUT 2      /* a cut or a skip flag with a transposed A or a second product */
HFMI_API int hfmi_dgemm_route_predict(int M, int N, int K, int K2, int batch, int ta, int tb, int64_t lda, int64_t ldb, int64_t sA, int64_t sB,
                                      int align_A, int align_B, int align_A2, int align_B2, int cut, int has_skip, int pipelined, int* route);
/* launch_dgemm with its whole descriptor, for the descriptor sweep of the tests.  Each host array X of n_X doubles (A, B, C; A2, B2 may
 * be null with n = 0) is uploaded to a 16-byte aligned device base and the descriptor's pointer is base + off_X, so an odd offset
 * makes an operand 8-byte but not 16-byte aligned.  dims[HFMI_TEST_DGEMM_DIMS], in this order:
 *    0 ta  1 tb  2 M  3 N  4 K  5 K2  6 batch  7 lda  8 ldb  9 ldc  10 sA  11 sB  12 sC  13 lower  14 cut
 *   15 skip: 0 = no flag, 1 = a device flag that is down, 2 = a device flag that is up
 *   16 n_A  17 off_A  18 n_B  19 off_B  20 n_A2  21 off_A2  22 n_B2  23 off_B2  24 n_C  25 off_C
 * The descriptor is filled verbatim and launch_dgemm is called once; nothing is validated beyond null pointers and that every operand
 * as described lies inside its array.  *launch_status = what launch_dgemm returned (HFMI_ERR_INVALID for its two refusals: the
 * text is in hfmi_last_error); the WHOLE host_C array comes back in either case -- pad rows of ldc, gaps between batch members, the
 * guard doubles before off_C and behind the last column -- so the caller can compare what must stay untouched bit for bit.
 * route[HFMI_DGEMM_ROUTE_WORDS]: the route of the launch that ran, as hfmi_dgemm_route_predict writes it. */
#define HFMI_TEST_DGEMM_DIMS 26
HFMI_API int hfmi_test_dgemm(hfmi_ctx* ctx, const int64_t* dims, double alpha, double beta, const double* host_A, const double* host_B,
                             const double* host_A2, const double* host_B2, double* host_C, int* route, int* launch_status);
/* fp64 MFMA / fp64 FMA / HBM-copy micro-benchmarks (peak denominators measured in the same job) */
HFMI_API int hfmi_bench_peaks(hfmi_ctx* ctx, double* mfma_f64_tflops, double* fma_f64_tflops, double* hbm_copy_gbs);
/* the same MFMA loop with a copy kernel streaming HBM beside it on a second stream: the ceiling of the power-limited regime the
 * big contractions run in (bench.py: roofline.frac_of_in_job_loaded_peak) */
HFMI_API int hfmi_bench_loaded_peak(hfmi_ctx* ctx, double* mfma_f64_tflops, double* hbm_copy_gbs);
/* the MFMA loop on full-mantissa Gaussian operands rotated through the registers every iteration -- alone, and beside the streaming
 * copy: the ceiling the contractions can reach on the solve's data under the power limit (SURVEY section 8d "fp64 MFMA
 * micro-benchmark run in the same job"; bench.py: roofline.frac_of_in_job_random_operand_peak[_while_streaming]) */
/* read-only 16-byte stream over 2 GiB: the HBM rate a contraction that only reads its big operand can reach (the copy of
 * hfmi_bench_peaks also writes); bench.py: roofline.frac_of_in_job_read_peak for the HBM-bound kernel-point shapes */
HFMI_API int hfmi_bench_hbm_read(hfmi_ctx* ctx, double* hbm_read_gbs);
HFMI_API int hfmi_bench_random_peaks(hfmi_ctx* ctx, double* mfma_f64_tflops, double* mfma_f64_tflops_while_streaming, double* hbm_copy_gbs);
/* per-launch HIP-event timing over a region of ordinary calls (bench.py's roofline numbers come from the
 * timed region itself): between begin and end every tsgemm_tn / tsgemm_nn launch is bracketed by events on
 * the context's stream.  end() synchronises and returns one record per distinct (kernel, shape):
 * kind[g] 0 = k_tsgemm_tn (or k_tsgemm_ss for skinny x skinny shapes), 1 = k_tsgemm_nn; shape[3*g..] = (short-side rows m, columns k, long axis N);
 * total milliseconds, launches, and the ALGORITHMIC flops / bytes of one launch. */
/* kernel tuning knobs for in-process A/B measurements (defaults are the measured winners; scripts/gemm_ab.py,
 * scripts/ss_ab.py, scripts/nn_tt_probe.py, scripts/nn_waves_ab.py): ("waves", 8|4|44) tsgemm_tn workgroup shape (44 = two 4-wave workgroups
 * per CU); ("rem4", 1|0) last column tile of <= 12 columns as 4-column groups on the 4x4x4 MFMA | as a full 16-column tile;
 * ("probe", 0..3) timing-only diagnostic of tsgemm_tn (bit 0: the streamed operand re-reads one address, bit 1: no staging /
 * barriers; results are garbage -- scripts/tn_probe.py); ("nn_waves", 0|4|8) and ("nn_tt", 0..3)
 * tsgemm_nn workgroup / wave-tile height (0 = automatic); ("nn_hybrid", 0|1) split only the tail row tiles; ("nn_res", 1|0) small matrix resident in LDS with persistent
 * workgroups when it fits (short reductions: Q R^-1, U = Q V); ("ss", 0|1) route skinny x skinny contractions to
 * tsgemm_ss; ("ss_percu", 1..4) resident tsgemm_ss workgroups per CU assumed when the grid is sized; ("eig", 0|1) Rayleigh-Ritz
 * eigensolver of every call: divide and conquer | Jacobi; ("chol", 0|1) Cholesky + inverse of the QR passes: blocked MFMA kernel |
 * column-at-a-time kernels; ("nn_res_tt", 0|1|2) tile height of the LDS-resident nn product: by round count | table | one less;
 * ("tn_hybrid", 0|1) tsgemm_tn with more row blocks than CUs: uniform split | whole rounds coarsely split + finely split tail;
 * ("prof_level", 1|2|3) what a profiling region records: 2 = every contraction and every phase (default), 3 = these and every pass of
 * a grid kernel covariance (hfmi_profile_end: kind 2, shape = line length, 4 * flags + part of the axis (0 whole, 1 high, 2 low sub-axis),
 * index of the pass in its plan; bytes = 16 (loaded + stored positions) per existing line and pair, 8 more per entry where the pass multiplies), 1 = contractions of at
 * least 2 Gflop only (each record is a pair of stream events, 2-4 us of idle GPU between dependent kernels: scripts/prof_level_ab.py);
 * ("comm_panels", 0..8) row panels of an operator application whose
 * rank reduction overlaps the rest of the product (0 / 1 = one all-reduce after the product; default 4);
 * ("qr_wide_min", 17..257) width from which hfmi_borth_qr takes the wide Cholesky-QR (default 257; lower values let tests compare
 * the two routes at widths both serve);
 * ("pchol_grid", 0..65535) most workgroups per launch of hfmi_pchol_create (0 = what the device holds, default): a small value makes every
 * workgroup walk several row tiles at small N (tests); L and the pivots do not depend on it, the traces only in their last bits;
 * ("fftcov_pairs", 0..4096) pairs of columns per chunk of the work buffer of hfmi_op_kernel_cov_grid (0 = from the byte budget,
 * default): results do not depend on it, bit for bit; the draws of hfmi_grid_sampler_draw and the applies of hfmi_op_grid_factor are
 * chunked by it in the same way;
 * ("fftcov_min_growth", 0..3) the growth hfmi_grid_sampler_create tries first (default 0; capped by its max_growth): a sampler on a larger
 * embedding than the rule would take (tests, measurements);
 * ("fftcov_max_line", a power of two in 4..4096) the longest transform line of the long route (hfmi_op_kernel_cov_grid_long), read
 * when such an operator is created (default 4096): a small value splits axes at small sizes (tests, measurements). */
HFMI_API int hfmi_tuning_set(const char* key, int value);
/* phases of hfmi_double_pass[_g], accumulated between hfmi_profile_begin and hfmi_profile_end (milliseconds, summed
 * over the solves in the region; device phases by HIP events on the context's stream, the HOST_* legs by the host's
 * wall clock -- they are part of the phase that called the host operator, normally BINV) */
#define HFMI_PHASE_APPLY 0        /* power-iteration applies of A (incl. their all-reduce) */
#define HFMI_PHASE_BINV 1         /* applies of B^-1 */
#define HFMI_PHASE_QR 2           /* (B-)orthogonalisation */
#define HFMI_PHASE_RAYLEIGH 3     /* second pass: T = Q^T A Q */
#define HFMI_PHASE_EIG 4          /* small eigensolve */
#define HFMI_PHASE_BACK 5         /* U = Q V */
#define HFMI_PHASE_ALLREDUCE 6    /* rank reductions enqueued by the solve (inside APPLY / RAYLEIGH) */
#define HFMI_PHASE_HOST_D2H 7     /* host callback: waiting for device -> pinned host copies */
#define HFMI_PHASE_HOST_FN 8      /* host callback: inside the host function */
#define HFMI_PHASE_HOST_H2D 9     /* host callback: issuing / draining pinned host -> device copies */
#define HFMI_PHASE_ALLREDUCE_AUX 10 /* rank reductions of row panels on the auxiliary stream, overlapped with the product that
                                     * makes the next panel; HFMI_PHASE_ALLREDUCE then holds only what the main stream waited */
#define HFMI_PHASE_COUNT 11
HFMI_API int hfmi_profile_phases(hfmi_ctx* ctx, double* ms_out /* HFMI_PHASE_COUNT */);   /* after hfmi_profile_end */
HFMI_API int hfmi_profile_begin(hfmi_ctx* ctx);
HFMI_API int hfmi_profile_end(hfmi_ctx* ctx, int max_groups, int* ngroups, int* kind, int64_t* shape, double* ms,
                     int64_t* launches, double* flops_per_launch, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* HFMI_H */
