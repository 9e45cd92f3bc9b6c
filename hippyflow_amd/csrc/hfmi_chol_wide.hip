// Cholesky factorisation with inverse of a k x k Gram matrix for 256 < k <= HFMI_WIDE_MAXK (2048), spread over the GPU: the
// contract of launch_chol_inv (hfmi_chol_col.hip / hfmi_chol.hip) beyond what one compute unit holds.  Everything lives in the wide
// arena of the context (row-major, ld = round_up(k, 32)):
//   G = R^T R,  R upper -> WA_R,  R^-1 upper -> WA_RINV (strict lower triangles written as zeros),
//   Rtot <- R (first pass) or R Rtot -> WA_RTOT,  AUX: original column norms, then diag(Rtot),
//   status words: min pivot ratio, || D^-1/2 G D^-1/2 - I ||_F of the input, shifted, failed.
// Right-looking with blocks of CW_NB = 64 columns.  Step p:
//   k_cw_diag   one workgroup: the diagonal block S_pp = R_pp^T R_pp and W_pp = R_pp^-1 in LDS (33 KB);
//   cw_gemm     the row panel R_p,c = W_pp^T S_p,c for the columns right of the block (one 64 x 64 tile per workgroup);
//   cw_gemm     the trailing update S_c,c' -= R_p,c^T R_p,c', upper tiles only.
// Then R^-1 by block back-substitution, bottom up: X_p,c = -W_pp (R_p,> X_>,c), two products per block row, the first one cut at the
// diagonal of the triangular factor; and Rtot as a triangular x triangular tile product.  All products are the 64 x 64 tile kernel
// k_dgemm<TA,TB,CUT> of hfmi_dgemm.hip with its triangular cuts (cw_gemm below holds the row-major / column-major transposition).
// A pivot at round-off level (piv <= pivot_tol * (G_jj + shift)) raises a device flag that turns every later launch of the attempt
// into a no-op; the host, which reads the status words of a pass anyway, restarts the factorisation ONCE with the diagonal
// shifted by shift_rel * trace(G) and reports `failed` when that breaks down too.
// No atomics, every sum in a fixed order: two runs give the same bits.
#include <math.h>
#include <string.h>

#include <vector>

#include "hfmi_dgemm.h"
#include "hfmi_internal.h"

namespace {
constexpr int CW_NB = 64;            // block size of the factorisation = tile of the products
constexpr int CW_MAXBLK = HFMI_WIDE_MAXK / CW_NB;
constexpr double CW_EPS = 2.220446049250313e-16;

// tail of the arena behind the WA_NSLOTS matrices (doubles): AUX (2 cap), diag0 (cap), pivot ratio per block (64),
// partial sums of trace / defect per tile (2 * 32 * 32), scalars (8: trace, defect^2), flags (8 ints)
inline size_t wa_tail_doubles(int cap) { return (size_t)3 * cap + 64 + 2 * CW_MAXBLK * CW_MAXBLK + 8 + 4; }
inline double* wa_diag0(hfmi_ctx* c) { return wa_aux(c) + 2 * (size_t)c->wide_cap; }
inline double* wa_ratio(hfmi_ctx* c) { return wa_diag0(c) + c->wide_cap; }
inline double* wa_part(hfmi_ctx* c) { return wa_ratio(c) + 64; }
inline double* wa_scal(hfmi_ctx* c) { return wa_part(c) + 2 * CW_MAXBLK * CW_MAXBLK; }
inline int* wa_flags(hfmi_ctx* c) { return (int*)(wa_scal(c) + 8); }

__device__ __forceinline__ double cw_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 256 threads of a workgroup, fixed order; red: 4 doubles of LDS
__device__ __forceinline__ double cw_block_sum(double v, double* red) {
  v = cw_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------ load
// WORK = upper triangle of (G + G^T) / 2 (+ shift on the diagonal), zeros elsewhere up to ld x ld; R and Rinv zero filled.
// attempt 0 also: diag0, the original column norms (first pass) and per-tile partial sums of the trace and of the squared defect.
__global__ __launch_bounds__(256) void k_cw_prep(const double* __restrict__ G, int ld, int k, double* __restrict__ W,
                                                 double* __restrict__ R, double* __restrict__ Rinv, double* __restrict__ diag0,
                                                 double* __restrict__ colnorm0, double* __restrict__ part, int attempt,
                                                 double shift_rel, const double* __restrict__ scal) {
  __shared__ double red[4];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int j = blockIdx.x * CW_NB + tx;
  const double shift = attempt ? shift_rel * scal[0] : 0.0;
  double dev = 0.0, tr = 0.0;
  const double gjj = (j < k) ? G[(size_t)j * ld + j] : 0.0;
  const double ivj = gjj > 0.0 ? 1.0 / sqrt(gjj) : 0.0;
  for (int u = 0; u < CW_NB / 4; ++u) {
    const int i = blockIdx.y * CW_NB + ty + 4 * u;
    if (i >= ld || j >= ld) continue;
    const bool in = i < k && j < k;
    double g = 0.0;
    if (in) {
      g = 0.5 * (G[(size_t)i * ld + j] + G[(size_t)j * ld + i]);
      if (attempt == 0) {
        const double gii = G[(size_t)i * ld + i];
        const double ivi = gii > 0.0 ? 1.0 / sqrt(gii) : 0.0;
        const double x = g * ivi * ivj - (i == j ? 1.0 : 0.0);
        dev += x * x;
        if (i == j) {
          tr += g;
          diag0[i] = g;
          if (colnorm0) colnorm0[i] = sqrt(fmax(g, 0.0));
        }
      }
    }
    W[(size_t)i * ld + j] = (in && j >= i) ? (i == j ? g + shift : g) : 0.0;
    R[(size_t)i * ld + j] = 0.0;
    Rinv[(size_t)i * ld + j] = 0.0;
  }
  if (attempt == 0) {
    dev = cw_block_sum(dev, red);
    tr = cw_block_sum(tr, red);
    if (threadIdx.x == 0) {
      const int t = blockIdx.y * gridDim.x + blockIdx.x;
      part[2 * t] = tr;
      part[2 * t + 1] = dev;
    }
  }
}
// scal[0] = trace, scal[1] = squared defect (attempt 0); the break flag is cleared for the attempt that follows
__global__ __launch_bounds__(256) void k_cw_sum(const double* __restrict__ part, int ntiles, double* __restrict__ scal,
                                                int* __restrict__ flags, int attempt) {
  __shared__ double red[4];
  if (attempt == 0) {
    double tr = 0.0, dev = 0.0;
    for (int t = threadIdx.x; t < ntiles; t += 256) {
      tr += part[2 * t];
      dev += part[2 * t + 1];
    }
    tr = cw_block_sum(tr, red);
    dev = cw_block_sum(dev, red);
    if (threadIdx.x == 0) {
      scal[0] = tr;
      scal[1] = dev;
    }
  }
  if (threadIdx.x == 0) flags[0] = 0;
}

// ------------------------------------------------------------------------------------------------ diagonal block
// S_pp (n <= 64 rows from j0) = R_pp^T R_pp column by column in LDS, then W_pp = R_pp^-1 row by row, bottom up (x_ic kept in the
// strict lower triangle of the LDS copy: X[i][c] -> M[c][i]; four lanes share a dot product).  Writes the diagonal blocks of R and Rinv.
__global__ __launch_bounds__(256) void k_cw_diag(const double* __restrict__ W, double* __restrict__ R, double* __restrict__ Rinv, int ld,
                                                 int k, int j0, const double* __restrict__ diag0, double shift_rel,
                                                 const double* __restrict__ scal, int attempt, double pivot_tol,
                                                 double* __restrict__ ratio, int* __restrict__ flags) {
  __shared__ double M[CW_NB][CW_NB + 1];
  __shared__ double rd[CW_NB], invd[CW_NB];
  if (flags[0]) return;
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const int n = min(CW_NB, k - j0);
  const double shift = attempt ? shift_rel * scal[0] : 0.0;
  for (int a = ty; a < CW_NB; a += 4) {
    double v = (a == tx) ? 1.0 : 0.0;
    if (a < n && tx < n && tx >= a) v = W[(size_t)(j0 + a) * ld + j0 + tx];
    M[a][tx] = v;
  }
  __syncthreads();
  double ratio_local = 1e300;
  for (int j = 0; j < n; ++j) {
    const double piv = M[j][j];
    const double ref = diag0[j0 + j] + shift;
    if (!(piv > pivot_tol * ref) || !(ref > 0.0)) {   // uniform: every thread reads the same words
      if (tid == 0) flags[0] = 1;
      return;
    }
    const double rjj = sqrt(piv), inv = 1.0 / rjj;
    ratio_local = fmin(ratio_local, piv / ref);
    if (tid == 0) {
      rd[j] = rjj;
      invd[j] = inv;
    }
    if (tid > j && tid < n) M[j][tid] *= inv;
    __syncthreads();
    for (int a = j + 1 + ty; a < n; a += 4)
      if (tx >= a && tx < n) M[a][tx] -= M[j][a] * M[j][tx];
    __syncthreads();
  }
  for (int a = ty; a < n; a += 4)
    if (tx < n) R[(size_t)(j0 + a) * ld + j0 + tx] = tx > a ? M[a][tx] : (tx == a ? rd[a] : 0.0);
  // inverse: x_cc = 1 / r_cc;  x_ic = -(sum_{l = i+1..c} r_il x_lc) / r_ii for c > i
  const int c = tid >> 2, q = tid & 3;
  for (int i = n - 2; i >= 0; --i) {
    double s = 0.0;
    if (c < n && c > i)
      for (int l = i + 1 + q; l <= c; l += 4) s += M[i][l] * (l == c ? invd[c] : M[c][l]);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (c < n && c > i && q == 0) M[c][i] = -s * invd[i];
    __syncthreads();
  }
  for (int a = ty; a < n; a += 4)
    if (tx < n) Rinv[(size_t)(j0 + a) * ld + j0 + tx] = tx > a ? M[tx][a] : (tx == a ? invd[a] : 0.0);
  if (tid == 0) ratio[j0 / CW_NB] = ratio_local;
}

// dst = upper triangle of src (k x k), zeros below the diagonal and in the pad columns k .. ld - 1
__global__ __launch_bounds__(256) void k_cw_copy_upper(double* __restrict__ dst, const double* __restrict__ src, int ld, int k,
                                                       const int* __restrict__ flags) {
  if (flags[0]) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ld) return;
  for (int i = blockIdx.y; i < k; i += gridDim.y) dst[(size_t)i * ld + j] = (j >= i && j < k) ? src[(size_t)i * ld + j] : 0.0;
}

// status words and the diag(Rtot) half of the AUX table.  pad = 1: this attempt broke down (the host restarts after attempt 0)
__global__ __launch_bounds__(256) void k_cw_final(const double* __restrict__ Rtot, int ld, int k, double* __restrict__ rdiag,
                                                  const double* __restrict__ ratio, int nblk, const double* __restrict__ scal,
                                                  const int* __restrict__ flags, int attempt, hfmi_status_words* __restrict__ status) {
  const int broke = flags[0];
  if (!broke)
    for (int i = threadIdx.x; i < k; i += 256) rdiag[i] = Rtot[(size_t)i * ld + i];
  if (threadIdx.x == 0) {
    double mr = 1e300;
    for (int b = 0; b < nblk; ++b) mr = fmin(mr, ratio[b]);
    status->min_pivot_ratio = broke ? 0.0 : mr;
    status->gram_dev = sqrt(scal[1]);
    status->offdiag = 0.0;
    status->shifted = (attempt || broke) ? 1 : 0;
    status->failed = (attempt && broke) ? 1 : 0;
    status->sweeps = 0;
    status->pad = broke;
    for (int t = 0; t < 8; ++t) status->tick[t] = 0;
  }
}

// C (M x N) = alpha op(A) op(B) + beta C, everything row-major with one leading dimension.  op(A)(i, l) = TA ? A[l * ld + i] : A[i * ld + l];
// op(B)(l, j) = TB ? B[j * ld + l] : B[l * ld + j].  mode bit 0: tiles below the diagonal are skipped; bit 1: the reduction stops at
// (tile column + 1) * 64 (op(B) upper triangular); bit 2: it starts at tile row * 64 (op(A) upper triangular).
// Runs as the column-major product C^T = op(B)^T op(A)^T of launch_dgemm: the operands and their transposition flags trade places,
// and the cuts of gemm_desc are these three seen from the other side.  A raised break flag makes the launch a no-op.
template <bool TA, bool TB>
int cw_gemm(hfmi_ctx* ctx, int M, int N, int K, double alpha, const double* A, const double* B, double beta, double* C, int ld, int mode) {
  gemm_desc g;
  g.ta = TB;
  g.tb = TA;
  g.M = N;
  g.N = M;
  g.K = K;
  g.alpha = alpha;
  g.beta = beta;
  g.A = B;
  g.B = A;
  g.C = C;
  g.lda = g.ldb = g.ldc = ld;
  g.cut = mode;
  g.skip = wa_flags(ctx);
  return launch_dgemm(ctx, g);
}
}  // namespace

int ctx_wide(hfmi_ctx* ctx, int k) {
  if (k < 1 || k > HFMI_WIDE_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "wide arena: k=%d out of range [1,%d]", k, HFMI_WIDE_MAXK);
  const int ld = (int)round_up(k, 32);
  const size_t doubles = (size_t)WA_NSLOTS * ld * ld + wa_tail_doubles(ld);      // grows with ld: large enough means laid out for >= ld
  if (ctx->wide.count() >= doubles) return HFMI_OK;
  OWN_TRY(grow(ctx->wide, doubles, [&] { return (int)hipStreamSynchronize(ctx->stream); }));
  ctx->wide_cap = ld;
  HIP_TRY(hipMemsetAsync(ctx->wide, 0, doubles * sizeof(double), ctx->stream));
  return HFMI_OK;
}

// one attempt: everything behind the first diagonal block is a no-op once the break flag is up
static int chol_wide_attempt(hfmi_ctx* ctx, int k, int ld, int rtot_mode, double shift_rel, double pivot_tol, int attempt) {
  double *G = wa_ptr(ctx, WA_GRAM), *W = wa_ptr(ctx, WA_WORK), *R = wa_ptr(ctx, WA_R), *X = wa_ptr(ctx, WA_RINV);
  double *Rtot = wa_ptr(ctx, WA_RTOT), *T = wa_ptr(ctx, WA_TMP);
  double* aux = wa_aux(ctx);
  int* flags = wa_flags(ctx);
  const int nt = (ld + CW_NB - 1) / CW_NB, nblk = (k + CW_NB - 1) / CW_NB;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_cw_prep, dim3(nt, nt), dim3(256), 0, st, G, ld, k, W, R, X, wa_diag0(ctx), rtot_mode == 1 ? aux : (double*)nullptr,
                     wa_part(ctx), attempt, shift_rel, wa_scal(ctx));
  hipLaunchKernelGGL(k_cw_sum, dim3(1), dim3(256), 0, st, wa_part(ctx), nt * nt, wa_scal(ctx), flags, attempt);
  HIP_TRY(hipGetLastError());
  for (int p = 0; p < nblk; ++p) {
    const int j0 = p * CW_NB, j1 = j0 + CW_NB, m = k - j1;
    hipLaunchKernelGGL(k_cw_diag, dim3(1), dim3(256), 0, st, W, R, X, ld, k, j0, wa_diag0(ctx), shift_rel, wa_scal(ctx), attempt, pivot_tol,
                       wa_ratio(ctx), flags);
    HIP_TRY(hipGetLastError());
    if (m <= 0) break;
    // R_p,> = W_pp^T S_p,>   and   S_>,> -= R_p,>^T R_p,>
    HFMI_TRY((cw_gemm<true, false>(ctx, CW_NB, m, CW_NB, 1.0, X + (size_t)j0 * ld + j0, W + (size_t)j0 * ld + j1, 0.0, R + (size_t)j0 * ld + j1, ld, 0)));
    HFMI_TRY((cw_gemm<true, false>(ctx, m, m, CW_NB, -1.0, R + (size_t)j0 * ld + j1, R + (size_t)j0 * ld + j1, 1.0, W + (size_t)j1 * ld + j1, ld, 1)));
  }
  // R^-1, bottom up: X_p,> = -W_pp (R_p,> X_>,>)
  for (int p = nblk - 2; p >= 0; --p) {
    const int j0 = p * CW_NB, j1 = j0 + CW_NB, m = k - j1;
    HFMI_TRY((cw_gemm<false, false>(ctx, CW_NB, m, m, 1.0, R + (size_t)j0 * ld + j1, X + (size_t)j1 * ld + j1, 0.0, T, ld, 2)));
    HFMI_TRY((cw_gemm<false, false>(ctx, CW_NB, m, CW_NB, -1.0, X + (size_t)j0 * ld + j0, T, 0.0, X + (size_t)j0 * ld + j1, ld, 0)));
  }
  const dim3 cgrid((ld + 255) / 256, k < 1024 ? k : 1024);
  if (rtot_mode == 1) {
    hipLaunchKernelGGL(k_cw_copy_upper, cgrid, dim3(256), 0, st, Rtot, R, ld, k, flags);
  } else {
    HFMI_TRY((cw_gemm<false, false>(ctx, k, k, k, 1.0, R, Rtot, 0.0, T, ld, 1 | 2 | 4)));
    hipLaunchKernelGGL(k_cw_copy_upper, cgrid, dim3(256), 0, st, Rtot, T, ld, k, flags);
  }
  hipLaunchKernelGGL(k_cw_final, dim3(1), dim3(256), 0, st, Rtot, ld, k, aux + ld, wa_ratio(ctx), nblk, wa_scal(ctx), flags, attempt, ctx->status_dev);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

int launch_chol_wide(hfmi_ctx* ctx, int k, int rtot_mode, double shift_rel, double pivot_tol, hfmi_status_words* host_st) {
  HFMI_TRY(ctx_wide(ctx, k));
  const int ld = (int)round_up(k, 32);
  if (pivot_tol <= 0.0) pivot_tol = 64.0 * k * CW_EPS;
  hfmi_status_words st;
  HFMI_TRY(chol_wide_attempt(ctx, k, ld, rtot_mode, shift_rel, pivot_tol, 0));
  HFMI_TRY(read_status(ctx, &st));
  if (st.pad) {   // breakdown: once more with the shifted diagonal
    HFMI_TRY(chol_wide_attempt(ctx, k, ld, rtot_mode, shift_rel, pivot_tol, 1));
    HFMI_TRY(read_status(ctx, &st));
  }
  if (host_st) *host_st = st;
  return HFMI_OK;
}

// the kernel family on a host matrix, without a QR around it (tests): host_G, host_R, host_Rinv k x k row-major;
// host_status: min_pivot_ratio, gram_dev, shifted, failed
extern "C" int hfmi_test_chol_wide(hfmi_ctx* ctx, int k, const double* host_G, double shift_rel, double pivot_tol, double* host_R,
                                   double* host_Rinv, double* host_status) {
  if (!ctx || !host_G || !host_R || !host_Rinv || !host_status) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > HFMI_WIDE_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "test_chol_wide: k=%d out of range [1,%d]", k, HFMI_WIDE_MAXK);
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(ctx_wide(ctx, k));
  const int ld = (int)round_up(k, 32);
  HFMI_TRY(upload_small(ctx, host_G, k, k, wa_ptr(ctx, WA_GRAM), ld));
  hfmi_status_words st;
  HFMI_TRY(launch_chol_wide(ctx, k, 1, shift_rel, pivot_tol, &st));
  host_status[0] = st.min_pivot_ratio;
  host_status[1] = st.gram_dev;
  host_status[2] = st.shifted;
  host_status[3] = st.failed;
  std::vector<double> tmp((size_t)k * ld);
  for (int which = 0; which < 2; ++which) {
    double* out = which ? host_Rinv : host_R;
    if (st.failed) {
      memset(out, 0, (size_t)k * k * sizeof(double));
      continue;
    }
    HFMI_TRY(read_back(ctx, wa_ptr(ctx, which ? WA_RINV : WA_R), tmp.size(), tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(out + (size_t)i * k, tmp.data() + (size_t)i * ld, (size_t)k * sizeof(double));
  }
  return HFMI_OK;
}
