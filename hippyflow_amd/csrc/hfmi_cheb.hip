// M^-1 on a block by Jacobi-preconditioned CHEBYSHEV iteration (prior.Msolver behind hp.Solver2Operator in
// hp.doublePassG(KLE_Operator, prior.M, prior.Msolver, ...), KLEProjector.py:163-164; the mass-orthogonal QR applies it
// once per solve to an N x k block).
//
// Why not the block CG at the end of this file (kept: it estimates the spectrum once per matrix and is the fallback): per
// iteration CG needs two global reductions -- five launches, eleven passes over N x k blocks, a host look at the
// residual every fourth iteration -- and its SpMM with one thread per ROW gathers 8 bytes per lane from k different
// vectors (1.5 TB/s on config 2 while the elementwise kernels beside it run at 6 TB/s out of the Infinity Cache).
// Chebyshev needs no inner products at all: ONE kernel per iteration, six passes, nothing for the host to wait for.
//
// Layout: the iteration works on a ROW-MAJOR copy of the block (entry (row, j) at [row * k + j]; two transposes per
// solve): with lanes mapped to the k columns of one row every access is a contiguous run of the row -- the gathers of
// the neighbour rows of a sparse-matrix row included -- and the matrix entries of that row are the same for all its
// lanes (broadcast loads).  Any CSR matrix, no ELL image needed.
//
//   theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma
//   x_0 = 0, x_1 = D^-1 b / theta
//   rho' = 1 / (2 sigma - rho);  x_{n+1} = x_n + rho' rho (x_n - x_{n-1}) + (2 rho' / delta) D^-1 (b - A x_n);  rho = rho'
// -- the three-term form of the iteration: the residual is recomputed from b in every step (no residual or direction
// arrays, no drift), x_{n+1} overwrites x_{n-1} in place, and a step reads b, x_n (with its neighbour rows), x_{n-1} and
// writes x_{n+1}: FOUR passes over three N x k arrays -- 200 MB on config 2, resident in the 256 MB Infinity Cache.
// [lmin, lmax] bracket the spectrum of D^-1 A (cheb_estimate below: Gershgorin from above, Lanczos of a scalar CG run from
// below); the error after n steps is at most 2 c^n / (1 + c^2n), c = (sqrt(kappa) - 1) / (sqrt(kappa) + 1).
#include <algorithm>
#include <cmath>

#include "hfmi_internal.h"

namespace {
// thread t of a 256-thread workgroup: row t / k of the workgroup's current group of rows, column t % k (k <= 256: 256 / k
// rows at a time); k > 256: one row at a time, the threads stride over its columns
struct rm_map {
  int rows_per_pass, rl, j0, jstep;
  bool live;
};
__device__ __forceinline__ rm_map rm_thread(int k) {
  rm_map m;
  if (k <= 256) {
    m.rows_per_pass = 256 / k;
    m.rl = threadIdx.x / k;
    m.j0 = threadIdx.x - m.rl * k;
    m.jstep = k;                       // one column per thread
    m.live = m.rl < m.rows_per_pass;
  } else {
    m.rows_per_pass = 1;
    m.rl = 0;
    m.j0 = threadIdx.x;
    m.jstep = 256;
    m.live = true;
  }
  return m;
}

// x_1 = D^-1 B / theta  (x_0 = 0 is never stored: the first step runs with c1 = 0 ... see launch_cheb_step)
__global__ __launch_bounds__(256) void k_cheb_first(const double* __restrict__ B, double* __restrict__ X1, double* __restrict__ X0,
                                                   const double* __restrict__ inv_diag, int64_t nrows, int k, double inv_theta) {
  const rm_map m = rm_thread(k);
  for (int64_t r0 = (int64_t)blockIdx.x * m.rows_per_pass; r0 < nrows; r0 += (int64_t)gridDim.x * m.rows_per_pass) {
    const int64_t row = r0 + m.rl;
    if (!m.live || row >= nrows) continue;
    const double s = inv_diag[row] * inv_theta;
    for (int j = m.j0; j < k; j += m.jstep) {
      const int64_t e = row * k + j;
      X1[e] = s * B[e];
      X0[e] = 0.0;
    }
  }
}

// One step of the three-term iteration, ONE WAVE PER ROW (k even): lane l holds columns 2l, 2l+1 as one 16-byte access, so the
// gather of a neighbour row is one instruction for up to 128 columns, and the row's (column, value) pairs are wave-uniform:
// scalar loads, no vector-memory traffic for the matrix.  UNR rows per wave for memory-level parallelism.
//   RESID = false:  Xp <- Xc + c1 (Xc - Xp) + c2 D^-1 (B - A Xc)      (Xp holds x_{n-1} on entry, x_{n+1} on exit)
//   RESID = true:   Xp <- B - A Xc                                     (the true residual, for the convergence check)
typedef double d2v __attribute__((ext_vector_type(2)));
template <bool RESID, int UNR>
__global__ __launch_bounds__(256) void k_cheb_step_wave(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                       const double* __restrict__ data, const double* __restrict__ inv_diag,
                                                       int64_t nrows, int k, const double* __restrict__ B, const double* __restrict__ Xc,
                                                       double* __restrict__ Xp, double c1, double c2) {
  // the matrix through the constant address space: with wave-uniform addresses the compiler then issues scalar loads (it will
  // not for plain global pointers once the kernel also stores, restrict or not)
  typedef const int64_t __attribute__((address_space(4)))* cptr64;
  typedef const int32_t __attribute__((address_space(4)))* cptr32;
  typedef const double __attribute__((address_space(4)))* cptrd;
  const cptr64 c_indptr = (cptr64)indptr;
  const cptr32 c_indices = (cptr32)indices;
  const cptrd c_data = (cptrd)data, c_inv_diag = (cptrd)inv_diag;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Workgroup b works on the band of
  // rows that belongs to ITS XCD (b % 8), so that the neighbour rows a sparse row gathers were fetched by the same L2.
  const int64_t per_xcd = gridDim.x / 8;                       // the grid is a multiple of 8
  const int64_t logical = (int64_t)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  const int64_t row0 = (logical * 4 + wave) * UNR;             // this wave's UNR consecutive rows
  if (row0 >= nrows) return;
  const int half = k >> 1;
  for (int l0 = 0; l0 < half; l0 += 64) {                      // k <= 128: one trip
    const int l = l0 + lane;
    const bool on = l < half;
    const int64_t col2 = on ? 2 * l : 0;
    d2v ax[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) ax[u] = d2v{0.0, 0.0};
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t row = row0 + u < nrows ? row0 + u : nrows - 1;
      const int64_t zb = c_indptr[row], ze = c_indptr[row + 1];
      for (int64_t z = zb; z < ze; ++z) {
        const double v = c_data[z];
        const d2v g = *reinterpret_cast<const d2v*>(Xc + (int64_t)c_indices[z] * k + col2);
        ax[u] += v * g;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t row = row0 + u;
      if (row >= nrows || !on) continue;
      const int64_t e = row * k + col2;
      const d2v res = *reinterpret_cast<const d2v*>(B + e) - ax[u];
      if (RESID) {
        *reinterpret_cast<d2v*>(Xp + e) = res;
      } else {
        const d2v xc = *reinterpret_cast<const d2v*>(Xc + e);
        const d2v xp = *reinterpret_cast<const d2v*>(Xp + e);
        *reinterpret_cast<d2v*>(Xp + e) = xc + c1 * (xc - xp) + (c2 * c_inv_diag[row]) * res;
      }
    }
  }
}

// the same step with one thread per (row, column) -- odd k, or k > 128 columns
template <bool RESID>
__global__ __launch_bounds__(256) void k_cheb_step(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                  const double* __restrict__ data, const double* __restrict__ inv_diag,
                                                  int64_t nrows, int k, const double* __restrict__ B, const double* __restrict__ Xc,
                                                  double* __restrict__ Xp, double c1, double c2) {
  const rm_map m = rm_thread(k);
  if (!m.live) return;
  const int64_t per_xcd = gridDim.x / 8;
  const int64_t logical = (int64_t)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  const int64_t row = logical * m.rows_per_pass + m.rl;
  if (row >= nrows) return;
  const int64_t zb = indptr[row], ze = indptr[row + 1];
  const double s = c2 * inv_diag[row];
  for (int j = m.j0; j < k; j += m.jstep) {
    double ax = 0.0;
    for (int64_t z = zb; z < ze; ++z) ax += data[z] * Xc[(int64_t)indices[z] * k + j];
    const int64_t e = row * k + j;
    const double res = B[e] - ax;
    if (RESID) {
      Xp[e] = res;
    } else {
      const double xc = Xc[e];
      Xp[e] = xc + c1 * (xc - Xp[e]) + s * res;
    }
  }
}

// per-column sums of squares of a row-major (nrows x k) array: one partial per (column, workgroup)
__global__ __launch_bounds__(256) void k_rm_colsq(const double* __restrict__ A, int64_t nrows, int k, double* __restrict__ part) {
  extern __shared__ double sh[];       // 256 doubles
  const rm_map m = rm_thread(k);
  for (int jb = 0; jb < k; jb += 256) {                // k <= 256: one trip
    double acc = 0.0;
    const int j = (k <= 256) ? m.j0 : jb + (int)threadIdx.x;
    if (m.live && j < k)
      for (int64_t row = (int64_t)blockIdx.x * m.rows_per_pass + m.rl; row < nrows; row += (int64_t)gridDim.x * m.rows_per_pass) {
        const double v = A[row * k + j];
        acc += v * v;
      }
    sh[threadIdx.x] = (m.live && j < k) ? acc : 0.0;
    __syncthreads();
    if (k <= 256) {
      if ((int)threadIdx.x < k) {                      // fixed order over the row groups of this workgroup
        double s = 0.0;
        for (int g = 0; g < m.rows_per_pass; ++g) s += sh[g * k + threadIdx.x];
        part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
      }
    } else if (j < k) {
      part[(int64_t)j * gridDim.x + blockIdx.x] = sh[threadIdx.x];
    }
    __syncthreads();
  }
}
}  // namespace

static inline unsigned cheb_grid(hfmi_ctx* ctx, int64_t nrows, int k) {
  const int rows_per_pass = k <= 256 ? 256 / k : 1;
  int64_t g = (nrows + rows_per_pass - 1) / rows_per_pass;
  const int64_t cap = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 64;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}
int launch_cheb_first(hfmi_ctx* ctx, const double* B, double* X1, double* X0, const double* inv_diag, int64_t nrows, int k, double inv_theta) {
  hipLaunchKernelGGL(k_cheb_first, dim3(cheb_grid(ctx, nrows, k)), dim3(256), 0, ctx->stream, B, X1, X0, inv_diag, nrows, k, inv_theta);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// one step (resid = false) or the residual B - A Xc into Xp (resid = true)
int launch_cheb_step(hfmi_ctx* ctx, const hfmi_csr* M, const double* B, const double* Xc, double* Xp, int k, double c1, double c2, bool resid) {
  static const bool thread_map = env_flag("HFMI_CHEB_THREADMAP");      // A/B switch
  if ((k & 1) == 0 && k <= 128 && !thread_map) {
    // rows per wave: 1 measured best on config 2 (53.5 us a step; 2: 54.4, 4: 63.0, 8: 104 -- profiles/r04c_cheb_unr.txt)
    static const int unr = getenv("HFMI_CHEB_UNR") ? atoi(getenv("HFMI_CHEB_UNR")) : 1;
    int64_t gw = (M->nrows + 4 * unr - 1) / (4 * unr);          // 4 waves x UNR rows per workgroup
    gw = (gw + 7) / 8 * 8;                                      // whole bands for the 8 XCDs
#define HFMI_CHEB_LAUNCH(RES, U) hipLaunchKernelGGL((k_cheb_step_wave<RES, U>), dim3((unsigned)gw), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->inv_diag, M->nrows, k, B, Xc, Xp, c1, c2)
    if (resid) { gw = ((M->nrows + 3) / 4 + 7) / 8 * 8; HFMI_CHEB_LAUNCH(true, 1); }
    else if (unr == 2) HFMI_CHEB_LAUNCH(false, 2);
    else if (unr == 4) HFMI_CHEB_LAUNCH(false, 4);
    else { gw = ((M->nrows + 3) / 4 + 7) / 8 * 8; HFMI_CHEB_LAUNCH(false, 1); }
#undef HFMI_CHEB_LAUNCH
    HIP_TRY(hipGetLastError());
    return HFMI_OK;
  }
  const int rows_per_pass = k <= 256 ? 256 / k : 1;
  int64_t g = (M->nrows + rows_per_pass - 1) / rows_per_pass;
  g = (g + 7) / 8 * 8;
  if (resid)
    hipLaunchKernelGGL((k_cheb_step<true>), dim3((unsigned)g), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->inv_diag, M->nrows, k, B, Xc, Xp, c1, c2);
  else
    hipLaunchKernelGGL((k_cheb_step<false>), dim3((unsigned)g), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->inv_diag, M->nrows, k, B, Xc, Xp, c1, c2);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// out[j] = sum over rows of A[row][j]^2 (deterministic: fixed partition, fixed order)
int launch_rm_colsq(hfmi_ctx* ctx, const double* A, int64_t nrows, int k, double* out) {
  const int chunks = 1024;
  void* part = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_PART, (size_t)k * chunks * sizeof(double), &part));
  hipLaunchKernelGGL(k_rm_colsq, dim3(chunks), dim3(256), 256 * sizeof(double), ctx->stream, A, nrows, k, (double*)part);
  HIP_TRY(hipGetLastError());
  return launch_dots_final(ctx, (const double*)part, chunks, k, out);
}

// ------------------------------------------------------------------ host side of the sparse SPD solve
// ---- spectrum of D^-1 A for the Chebyshev solve -------------------------------------------------------------------------
// extreme eigenvalues of the symmetric tridiagonal matrix (a, b) by bisection on the Sturm count
static int sturm_count(const std::vector<double>& a, const std::vector<double>& b, double x) {
  int cnt = 0;
  double q = a[0] - x;
  if (q < 0) ++cnt;
  for (size_t i = 1; i < a.size(); ++i) {
    if (q == 0.0) q = 1e-300;
    q = a[i] - x - b[i - 1] * b[i - 1] / q;
    if (q < 0) ++cnt;
  }
  return cnt;
}
static void tridiag_extremes(const std::vector<double>& a, const std::vector<double>& b, double* smallest, double* largest) {
  double lo = a[0], hi = a[0];
  for (size_t i = 0; i < a.size(); ++i) {
    const double rad = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < a.size() ? fabs(b[i]) : 0.0);
    lo = std::min(lo, a[i] - rad);
    hi = std::max(hi, a[i] + rad);
  }
  const int m = (int)a.size();
  double l = lo, h = hi;
  for (int it = 0; it < 200 && h - l > 1e-14 * std::max(fabs(l), fabs(h)); ++it) {   // smallest: first x with count >= 1
    const double mid = 0.5 * (l + h);
    if (sturm_count(a, b, mid) >= 1) h = mid; else l = mid;
  }
  *smallest = 0.5 * (l + h);
  l = lo; h = hi;
  for (int it = 0; it < 200 && h - l > 1e-14 * std::max(fabs(l), fabs(h)); ++it) {   // largest: last x with count < m
    const double mid = 0.5 * (l + h);
    if (sturm_count(a, b, mid) >= m) h = mid; else l = mid;
  }
  *largest = 0.5 * (l + h);
}
// One scalar Jacobi-CG run on a pseudo-random right-hand side, on the device, with its two inner products per iteration read
// back: the CG coefficients are the Lanczos matrix of D^-1 A, whose extreme eigenvalues approach those of D^-1 A from inside.
// Once per matrix (~40 iterations of one-vector kernels).
static int cheb_estimate(hfmi_op* op) {
  hfmi_ctx* ctx = op->ctx;
  hfmi_csr* M = const_cast<hfmi_csr*>(op->csr);
  const int64_t N = M->nrows;
  M->cheb_state = -1;
  if (!(M->gersh_lmax > 0.0)) return HFMI_OK;
  hfmi_block R, Z, P, AP;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_0, N, 1, &R));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_1, N, 1, &Z));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_2, N, 1, &P));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_3, N, 1, &AP));
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, 4 * sizeof(double), &sc));
  double *rz = (double*)sc, *pap = rz + 1, *rz_new = rz + 2;
  HFMI_TRY(launch_randn(ctx, R.p, N, 1, R.ld, 0x5eedc0deull, 77u, 1.0));
  HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->inv_diag, N, 1));
  HFMI_TRY(launch_copy(ctx, P.p, P.ld, Z.p, Z.ld, N, 1));
  HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, 1, rz));
  double h_rz = 0, h_pap = 0, h_new = 0;
  HFMI_TRY(read_back(ctx, rz, 1, &h_rz));
  const double rz0 = h_rz;
  std::vector<double> alpha, beta;
  for (int it = 0; it < 60 && h_rz > 1e-28 * rz0; ++it) {
    HFMI_TRY(launch_csr_spmm(ctx, M, P.p, P.ld, AP.p, AP.ld, 1, false));
    HFMI_TRY(launch_col_dots(ctx, P.p, P.ld, AP.p, AP.ld, N, 1, pap));
    HFMI_TRY(launch_col_axpy_dev(ctx, R.p, R.ld, AP.p, AP.ld, N, 1, rz, pap, -1.0));
    HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->inv_diag, N, 1));
    HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, 1, rz_new));
    HFMI_TRY(launch_col_xpby_dev(ctx, P.p, P.ld, Z.p, Z.ld, N, 1, rz_new, rz));
    double two[3];
    HFMI_TRY(read_back(ctx, rz, 3, two));
    h_pap = two[1];
    h_new = two[2];
    if (!(h_pap > 0.0) || !std::isfinite(h_new)) return HFMI_OK;     // not SPD: leave the Chebyshev route off
    alpha.push_back(h_rz / h_pap);
    beta.push_back(h_new / h_rz);
    HIP_TRY(hipMemcpyAsync(rz, rz_new, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    h_rz = h_new;
  }
  const size_t m = alpha.size();
  if (m < 3) return HFMI_OK;
  std::vector<double> a(m), b(m > 1 ? m - 1 : 0);
  for (size_t i = 0; i < m; ++i) {
    a[i] = 1.0 / alpha[i] + (i > 0 ? beta[i - 1] / alpha[i - 1] : 0.0);
    if (i + 1 < m) b[i] = sqrt(beta[i]) / alpha[i];
  }
  double tmin, tmax;
  tridiag_extremes(a, b, &tmin, &tmax);
  if (!(tmin > 0.0) || !(tmax >= tmin)) return HFMI_OK;
  // Ritz values lie inside the spectrum: widen them; never above Gershgorin's bound
  M->cheb_lmin = 0.9 * tmin;
  M->cheb_lmax = std::min(M->gersh_lmax, 1.05 * tmax);
  if (M->cheb_lmax < tmax) M->cheb_lmax = tmax * (1.0 + 1e-9);
  M->cheb_state = 1;
  return HFMI_OK;
}

// Y = M^-1 W by Chebyshev iteration on row-major copies (hfmi_cheb.hip); *handled = false: the caller runs the block CG
static int cheb_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, bool* handled) {
  hfmi_ctx* ctx = op->ctx;
  hfmi_csr* M = const_cast<hfmi_csr*>(op->csr);
  const int64_t N = W->N;
  const int k = W->nvec;
  *handled = false;
  static const bool off = env_flag("HFMI_PCG");          // A/B switch: always the block CG
  if (off || M->cheb_state < 0) return HFMI_OK;
  if (M->cheb_state == 0) HFMI_TRY(cheb_estimate(op));
  if (M->cheb_state != 1) return HFMI_OK;
  const double lmin = M->cheb_lmin, lmax = M->cheb_lmax;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
  hfmi_block Bb, X0b, X1b;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_0, N, k, &Bb));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_1, N, k, &X0b));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_2, N, k, &X1b));
  double* B = Bb.p;                                                  // used as row-major N x k arrays (ld >= N: large enough)
  double* X[2] = {X0b.p, X1b.p};
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)2 * k * sizeof(double), &sc));
  double* bb = (double*)sc;
  double* rr = bb + k;
  HFMI_TRY(launch_block_to_dense(ctx, W->p, W->ld, B, N, k));
  HFMI_TRY(launch_rm_colsq(ctx, B, N, k, bb));
  HFMI_TRY(launch_cheb_first(ctx, B, X[1], X[0], M->inv_diag, N, k, 1.0 / theta));     // x_0 = 0 in X[0], x_1 in X[1]
  int steps = 1, cur = 1;                                            // X[cur] = x_steps, X[cur ^ 1] = x_{steps-1}
  const bool spread = delta > 1e-12 * theta;                         // else D^-1 A is a multiple of the identity: x_1 is the answer
  double rho = spread ? delta / theta : 0.0;                         // 1 / sigma
  int planned = 1;
  if (spread) {
    const double sk = sqrt(lmax / lmin), c = (sk - 1.0) / (sk + 1.0);
    planned = (int)ceil(log(2.0 / op->rel_tol) / -log(c)) + 1;
  }
  if (planned > op->max_iter || planned > 200) {
    // a spectrum this wide needs more steps than CG's superlinear convergence would: leave this matrix to the block CG
    M->cheb_state = -1;
    return HFMI_OK;
  }
  std::vector<double> h(2 * (size_t)k);
  int budget = planned - 1;
  for (int round = 0; round < 4; ++round) {
    for (int i = 0; i < budget; ++i, ++steps) {
      const double rho_new = 1.0 / (2.0 * theta / delta - rho);
      HFMI_TRY(launch_cheb_step(ctx, M, B, X[cur], X[cur ^ 1], k, rho_new * rho, 2.0 * rho_new / delta, false));
      rho = rho_new;
      cur ^= 1;
    }
    // the true residual b - A x into the spare array, its column norms against those of b
    void* rs = nullptr;
    HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)N * k * sizeof(double), &rs));
    HFMI_TRY(launch_cheb_step(ctx, M, B, X[cur], (double*)rs, k, 0.0, 0.0, true));
    HFMI_TRY(launch_rm_colsq(ctx, (const double*)rs, N, k, rr));
    HFMI_TRY(read_back(ctx, bb, (size_t)2 * k, h.data()));
    bool done = true, diverged = false;
    for (int j = 0; j < k; ++j) {
      if (!std::isfinite(h[j]))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "csr solve: non-finite right-hand side in vector %d", j);
      // a residual that is not finite, or larger than the right-hand side it started from, means the polynomial grew: an
      // eigenvalue of D^-1 A lies outside the bracket (Ritz values of a short CG run from one random vector can miss the top of
      // the spectrum).  That is a failure of the ESTIMATE, not of the matrix: hand the solve to the block CG, which alone
      // reports a matrix that is not SPD (advisor r4)
      if (!std::isfinite(h[k + j]) || h[k + j] > h[j]) diverged = true;
      if (!(h[k + j] <= op->rel_tol * op->rel_tol * h[j])) done = false;
    }
    if (diverged) break;
    if (done) {
      op->last_iters = steps;
      op->last_method = 1;
      HFMI_TRY(launch_dense_to_block(ctx, X[cur], Y->p, Y->ld, N, k));
      *handled = true;
      return HFMI_OK;
    }
    if (!spread) break;
    budget = std::max(2, planned / 3);
    if (steps + budget > op->max_iter) break;
  }
  M->cheb_state = -1;       // the bracket of the spectrum was not good enough: this matrix goes back to the block CG for good
  return HFMI_OK;
}

// Y = M^{-1} W for an SPD CSR matrix: Jacobi-preconditioned CG run on all vectors at once (independent
// recurrences, shared SpMM); per-vector scalars stay on the device, the host only polls convergence.
int csr_pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_ctx* ctx = op->ctx;
  hfmi_csr* M = const_cast<hfmi_csr*>(op->csr);
  const int64_t N = W->N;
  const int k = W->nvec;
  if (M->nrows != N) HFMI_FAIL(HFMI_ERR_INVALID, "csr_pcg: matrix has %lld rows, block vectors have %lld", (long long)M->nrows, (long long)N);
  if (!M->inv_diag) {
    HIP_TRY(hipMalloc((void**)&M->inv_diag, (size_t)N * sizeof(double)));
    HFMI_TRY(launch_csr_diag_inv(ctx, M));
  }
  {
    bool handled = false;
    HFMI_TRY(cheb_solve(op, W, Y, &handled));
    if (handled) return HFMI_OK;
  }
  hfmi_block R, Z, P, AP;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_0, N, k, &R));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_1, N, k, &Z));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_2, N, k, &P));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_3, N, k, &AP));
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)6 * k * sizeof(double), &sc));
  // two (r.z, r.r) pairs: an iteration reads r.z from one and writes the new r.z and r.r into the other (r.r must follow
  // r.z_new: launch_pcg_update fills both with one final pass); the pairs swap roles instead of being copied
  double* rz = (double*)sc;       // r.z
  double* rz_new = rz + 2 * k;
  double* rr = rz_new + k;
  double* pap = rz + 4 * k;
  double* bb = rz + 5 * k;
  std::vector<double> h_rr(k), h_bb(k);
  // x0 = 0, r = b
  HFMI_TRY(launch_fill(ctx, Y->p, N, k, Y->ld, 0.0, false));
  HFMI_TRY(launch_copy(ctx, R.p, R.ld, W->p, W->ld, N, k));
  HFMI_TRY(launch_col_dots(ctx, W->p, W->ld, W->p, W->ld, N, k, bb));
  HFMI_TRY(read_back(ctx, bb, k, h_bb.data()));
  HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->inv_diag, N, k));
  HFMI_TRY(launch_copy(ctx, P.p, P.ld, Z.p, Z.ld, N, k));
  HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, k, rz));
  int it = 0;
  bool done = false;
  for (; it < op->max_iter && !done; ++it) {
    if (M->ell_w > 0) {
      // three passes over the blocks per iteration: A p fused with p . A p; (x, r) update fused with both residual
      // dots; the new direction with z = D^-1 r recomputed on the fly (never stored)
      HFMI_TRY(launch_ell_spmm_dot(ctx, M, P.p, P.ld, AP.p, AP.ld, k, pap));
      HFMI_TRY(launch_pcg_update(ctx, Y->p, Y->ld, R.p, R.ld, P.p, P.ld, AP.p, AP.ld, M->inv_diag, N, k, rz, pap, rz_new, rr));
      HFMI_TRY(launch_pcg_direction(ctx, P.p, P.ld, R.p, R.ld, M->inv_diag, N, k, rz_new, rz));
      double* const rr_done = rr;
      std::swap(rz, rz_new);        // the pair just written becomes "current"
      rr = rz_new + k;
      if ((it & 3) == 3 || it + 1 == op->max_iter) {
        HFMI_TRY(read_back(ctx, rr_done, k, h_rr.data()));
        done = true;
        for (int j = 0; j < k; ++j)
          if (!(h_rr[j] <= op->rel_tol * op->rel_tol * h_bb[j])) done = false;
        for (int j = 0; j < k; ++j)
          if (!std::isfinite(h_rr[j]) || !std::isfinite(h_bb[j]))
            HFMI_FAIL(HFMI_ERR_NUMERIC, "csr_pcg: non-finite residual in vector %d at iteration %d (matrix not SPD, or non-finite input)", j, it + 1);
      }
      continue;
    }
    HFMI_TRY(launch_csr_spmm(ctx, M, P.p, P.ld, AP.p, AP.ld, k, false));
    HFMI_TRY(launch_col_dots(ctx, P.p, P.ld, AP.p, AP.ld, N, k, pap));
    HFMI_TRY(launch_col_axpy_dev(ctx, Y->p, Y->ld, P.p, P.ld, N, k, rz, pap, 1.0));
    HFMI_TRY(launch_col_axpy_dev(ctx, R.p, R.ld, AP.p, AP.ld, N, k, rz, pap, -1.0));
    HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->inv_diag, N, k));
    HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, k, rz_new));
    HFMI_TRY(launch_col_xpby_dev(ctx, P.p, P.ld, Z.p, Z.ld, N, k, rz_new, rz));
    HIP_TRY(hipMemcpyAsync(rz, rz_new, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if ((it & 3) == 3 || it + 1 == op->max_iter) {
      HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, R.p, R.ld, N, k, rr));
      HFMI_TRY(read_back(ctx, rr, k, h_rr.data()));
      done = true;
      for (int j = 0; j < k; ++j)
        if (!(h_rr[j] <= op->rel_tol * op->rel_tol * h_bb[j])) done = false;
      for (int j = 0; j < k; ++j)
        if (!std::isfinite(h_rr[j]) || !std::isfinite(h_bb[j]))
          HFMI_FAIL(HFMI_ERR_NUMERIC, "csr_pcg: non-finite residual in vector %d at iteration %d (matrix not SPD, or non-finite input)", j, it + 1);
    }
  }
  op->last_iters = it;
  op->last_method = 0;
  if (!done) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "csr_pcg: no convergence to %.1e in %d iterations", op->rel_tol, op->max_iter);
  return HFMI_OK;
}
