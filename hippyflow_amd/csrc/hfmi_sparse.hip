// Sparse matrices on column-major blocks: the CSR / ELL products Y (+)= M X (hfmi_op_csr), the Jacobi preconditioner of a matrix,
// and M^-1 W for an SPD matrix (prior.Msolver; hfmi_op_csr_pcg): Chebyshev iteration where the spectrum allows it (hfmi_cheb.hip), else
// the Jacobi-preconditioned block CG below with its fused vector updates.
#include <algorithm>
#include <cmath>

#include "hfmi_internal.h"

typedef double d2 __attribute__((ext_vector_type(2)));

// ELL variant: thread = row, the (index, value) pairs of a slot are contiguous across the rows of a wave, SPMM_EB
// vectors per pass.  DOT: also emit this workgroup's part of <X_j, Y_j> (the p . A p of PCG) -- one partial per
// (vector, workgroup), summed in a fixed order by k_col_dots_final.
constexpr int SPMM_EB = 12;
template <bool DOT>
__global__ __launch_bounds__(256) void k_ell_spmm(const int32_t* __restrict__ eidx, const double* __restrict__ eval,
                                                  int w, int64_t nrows, const double* __restrict__ X, int64_t ldx,
                                                  double* __restrict__ Y, int64_t ldy, int nvec, int accumulate,
                                                  double* __restrict__ part, int gx8, int gy) {
  __shared__ double wsum[4][SPMM_EB];
  // XCD-aware order (1-D grid of gx8 * gy workgroups, gx8 a multiple of 8): workgroups are dealt round-robin to the 8 XCDs;
  // XCD x takes the x-th band of row blocks, for every group of vectors, so that the rows a band gathers from (its own and
  // the neighbouring ones) are fetched into ONE L2.  With the natural order every L2 pulled most of X through the fabric:
  // 453 MB of HBM reads per launch for 143 MB of operands on config 2 (profiles/r04c PMC pass).
  const int per = gx8 >> 3;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int rb = xcd * per + slot % per, yg = slot / per;
  const int64_t row = (int64_t)rb * blockDim.x + threadIdx.x;
  const bool live = row < nrows;
  const int64_t r = live ? row : nrows - 1;
  for (int j0 = yg * SPMM_EB; j0 < nvec; j0 += gy * SPMM_EB) {
    double acc[SPMM_EB];
#pragma unroll
    for (int jj = 0; jj < SPMM_EB; ++jj) acc[jj] = 0.0;
    for (int s = 0; s < w; ++s) {
      const double v = eval[(int64_t)s * nrows + r];
      const double* xr = X + eidx[(int64_t)s * nrows + r];
#pragma unroll
      for (int jj = 0; jj < SPMM_EB; ++jj) {
        const int j = j0 + jj < nvec ? j0 + jj : nvec - 1;
        acc[jj] += v * xr[(int64_t)j * ldx];
      }
    }
#pragma unroll
    for (int jj = 0; jj < SPMM_EB; ++jj)
      if (live && j0 + jj < nvec) {
        double* y = Y + (int64_t)(j0 + jj) * ldy + row;
        *y = accumulate ? *y + acc[jj] : acc[jj];
      }
    if (DOT) {
#pragma unroll
      for (int jj = 0; jj < SPMM_EB; ++jj) {
        const int j = j0 + jj < nvec ? j0 + jj : nvec - 1;
        double d = live ? acc[jj] * X[(int64_t)j * ldx + row] : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_down(d, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][jj] = d;
      }
      __syncthreads();
      if ((int)threadIdx.x < SPMM_EB && j0 + (int)threadIdx.x < nvec)
        part[(int64_t)(j0 + threadIdx.x) * gx8 + rb] =
            (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------ CSR SpMM: Y[:, j] (+)= M X[:, j]
// One lane per matrix row (consecutive lanes -> consecutive rows: coalesced Y stores; the gathers of X hit
// neighbouring rows for FEM matrices), 8 vectors per pass so the row's (index, value) pairs are read once per 8.
constexpr int SPMM_JB = 8;
__global__ void k_csr_spmm(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                           const double* __restrict__ data, int64_t nrows, const double* __restrict__ X, int64_t ldx,
                           double* __restrict__ Y, int64_t ldy, int nvec, int accumulate, int gx8, int gy) {
  // XCD-aware row bands, as in k_ell_spmm: 1-D grid of gx8 * gy workgroups, XCD x (= blockIdx.x % 8) owns the x-th band of rows
  const int per = gx8 >> 3;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int rb = xcd * per + slot % per, yg = slot / per;
  const int64_t row = (int64_t)rb * blockDim.x + threadIdx.x;
  if (row >= nrows) return;
  const int64_t b = indptr[row], e = indptr[row + 1];
  for (int j0 = yg * SPMM_JB; j0 < nvec; j0 += gy * SPMM_JB) {
    double acc[SPMM_JB];
#pragma unroll
    for (int jj = 0; jj < SPMM_JB; ++jj) acc[jj] = 0.0;
    for (int64_t z = b; z < e; ++z) {
      const double v = data[z];
      const double* xr = X + indices[z];
#pragma unroll
      for (int jj = 0; jj < SPMM_JB; ++jj)
        if (j0 + jj < nvec) acc[jj] += v * xr[(int64_t)(j0 + jj) * ldx];
    }
#pragma unroll
    for (int jj = 0; jj < SPMM_JB; ++jj)
      if (j0 + jj < nvec) {
        double* y = Y + (int64_t)(j0 + jj) * ldy + row;
        *y = accumulate ? *y + acc[jj] : acc[jj];
      }
  }
}
int launch_csr_spmm(hfmi_ctx* ctx, const hfmi_csr* M, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec, bool accumulate) {
  if (M->nrows <= 0 || nvec <= 0) return HFMI_OK;
  if (M->ell_w > 0) {
    const int gx8 = (int)(((M->nrows + 255) / 256 + 7) / 8 * 8), gy = (nvec + SPMM_EB - 1) / SPMM_EB;
    hipLaunchKernelGGL((k_ell_spmm<false>), dim3((unsigned)(gx8 * gy)), dim3(256), 0, ctx->stream, M->ell_idx, M->ell_val, M->ell_w, M->nrows, X,
                       ldx, Y, ldy, nvec, accumulate ? 1 : 0, (double*)nullptr, gx8, gy);
    HIP_TRY(hipGetLastError());
    return HFMI_OK;
  }
  const int gy = (nvec + SPMM_JB - 1) / SPMM_JB;
  const int gx8 = (int)(((M->nrows + 255) / 256 + 7) / 8 * 8);
  hipLaunchKernelGGL(k_csr_spmm, dim3((unsigned)(gx8 * gy)), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->nrows, X, ldx, Y, ldy, nvec, accumulate ? 1 : 0, gx8, gy);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
__global__ void k_csr_diag_inv(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                               const double* __restrict__ data, int64_t nrows, double* __restrict__ inv_diag) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrows) return;
  double d = 0.0;
  for (int64_t z = indptr[row]; z < indptr[row + 1]; ++z)
    if (indices[z] == row) d += data[z];
  inv_diag[row] = d != 0.0 ? 1.0 / d : 1.0;
}
int launch_csr_diag_inv(hfmi_ctx* ctx, const hfmi_csr* M) {
  hipLaunchKernelGGL(k_csr_diag_inv, dim3((unsigned)((M->nrows + 255) / 256)), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->nrows, M->solve.inv_diag);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
int csr_prepare_jacobi(hfmi_ctx* ctx, const hfmi_csr* M) {
  if (M->solve.inv_diag) return HFMI_OK;
  OWN_TRY(M->solve.inv_diag.alloc((size_t)M->nrows));
  return launch_csr_diag_inv(ctx, M);
}

// y_j += sign * coef_j * x_j,  coef_j = num_j / den_j (den == null: num_j); a zero denominator gives 0 (converged vector)
__global__ void k_col_axpy_dev(double* __restrict__ y, int64_t ldy, const double* __restrict__ x, int64_t ldx, int64_t N, int nvec,
                               const double* __restrict__ num, const double* __restrict__ den, double sign) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double coef = num[j];
    if (den) coef = den[j] != 0.0 ? coef / den[j] : 0.0;
    coef *= sign;
    double* yc = y + (int64_t)j * ldy;
    const double* xc = x + (int64_t)j * ldx;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        d2 v = *reinterpret_cast<d2*>(yc + t);
        const d2 u = *reinterpret_cast<const d2*>(xc + t);
        v.x += coef * u.x; v.y += coef * u.y;
        *reinterpret_cast<d2*>(yc + t) = v;
      } else yc[t] += coef * xc[t];
    }
  }
}
int launch_col_axpy_dev(hfmi_ctx* ctx, double* y, int64_t ldy, const double* x, int64_t ldx, int64_t N, int nvec, const double* num, const double* den, double sign) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_col_axpy_dev, ew_grid(N, nvec), dim3(256), 0, ctx->stream, y, ldy, x, ldx, N, nvec, num, den, sign);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
__global__ void k_col_xpby_dev(double* __restrict__ p, int64_t ldp, const double* __restrict__ z, int64_t ldz, int64_t N, int nvec,
                               const double* __restrict__ num, const double* __restrict__ den) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    const double coef = den[j] != 0.0 ? num[j] / den[j] : 0.0;
    double* pc = p + (int64_t)j * ldp;
    const double* zc = z + (int64_t)j * ldz;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        d2 v = *reinterpret_cast<d2*>(pc + t);
        const d2 u = *reinterpret_cast<const d2*>(zc + t);
        v.x = u.x + coef * v.x; v.y = u.y + coef * v.y;
        *reinterpret_cast<d2*>(pc + t) = v;
      } else pc[t] = zc[t] + coef * pc[t];
    }
  }
}
int launch_col_xpby_dev(hfmi_ctx* ctx, double* p, int64_t ldp, const double* z, int64_t ldz, int64_t N, int nvec, const double* num, const double* den) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_col_xpby_dev, ew_grid(N, nvec), dim3(256), 0, ctx->stream, p, ldp, z, ldz, N, nvec, num, den);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
__global__ void k_diag_scale(double* __restrict__ z, int64_t ldz, const double* __restrict__ r, int64_t ldr, const double* __restrict__ inv_diag, int64_t N, int nvec) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* zc = z + (int64_t)j * ldz;
    const double* rc = r + (int64_t)j * ldr;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += (int64_t)gridDim.x * blockDim.x) zc[t] = inv_diag[t] * rc[t];
  }
}
int launch_diag_scale(hfmi_ctx* ctx, double* z, int64_t ldz, const double* r, int64_t ldr, const double* inv_diag, int64_t N, int nvec) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_diag_scale, ew_grid(2 * N, nvec), dim3(256), 0, ctx->stream, z, ldz, r, ldr, inv_diag, N, nvec);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

int launch_ell_spmm_dot(hfmi_ctx* ctx, const hfmi_csr* M, const double* X, int64_t ldx, double* Y, int64_t ldy, int nvec,
                        double* dots) {
  if (M->ell_w <= 0) HFMI_FAIL(HFMI_ERR_INVALID, "ell_spmm_dot: matrix has no ELL image");
  const int gx = (int)(((M->nrows + 255) / 256 + 7) / 8 * 8), gy = (nvec + SPMM_EB - 1) / SPMM_EB;
  void* part = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_PART, (size_t)nvec * gx * sizeof(double), &part));
  hipLaunchKernelGGL((k_ell_spmm<true>), dim3((unsigned)(gx * gy)), dim3(256), 0, ctx->stream, M->ell_idx, M->ell_val, M->ell_w, M->nrows, X, ldx,
                     Y, ldy, nvec, 0, (double*)part, gx, gy);
  HIP_TRY(hipGetLastError());
  return launch_dots_final(ctx, (const double*)part, (int)gx, nvec, dots);
}

// Fused PCG update (one pass over y, r, p, ap instead of four kernels): per column j, alpha = rz_j / pap_j,
// y += alpha p, r -= alpha ap, partial sums of <r, D^-1 r> and <r, r>.  z = D^-1 r is never stored.
constexpr int PCG_CHUNKS = 128;
__global__ __launch_bounds__(256) void k_pcg_update(double* __restrict__ y, int64_t ldy, double* __restrict__ r, int64_t ldr,
                                                    const double* __restrict__ p, int64_t ldp,
                                                    const double* __restrict__ ap, int64_t ldap,
                                                    const double* __restrict__ dinv, int64_t N, int nvec,
                                                    const double* __restrict__ rz, const double* __restrict__ pap,
                                                    double* __restrict__ part) {
  __shared__ double wsum[4][2];
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    const double a = pap[j] != 0.0 ? rz[j] / pap[j] : 0.0;
    double* yc = y + (int64_t)j * ldy;
    double* rc = r + (int64_t)j * ldr;
    const double* pc = p + (int64_t)j * ldp;
    const double* ac = ap + (int64_t)j * ldap;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        d2 yv = *reinterpret_cast<d2*>(yc + t), rv = *reinterpret_cast<d2*>(rc + t);
        const d2 pv = *reinterpret_cast<const d2*>(pc + t), av = *reinterpret_cast<const d2*>(ac + t);
        const d2 dv = *reinterpret_cast<const d2*>(dinv + t);
        yv.x += a * pv.x; yv.y += a * pv.y;
        rv.x -= a * av.x; rv.y -= a * av.y;
        *reinterpret_cast<d2*>(yc + t) = yv;
        *reinterpret_cast<d2*>(rc + t) = rv;
        s1 += rv.x * (dv.x * rv.x) + rv.y * (dv.y * rv.y);
        s2 += rv.x * rv.x + rv.y * rv.y;
      } else {
        yc[t] += a * pc[t];
        const double rv = rc[t] - a * ac[t];
        rc[t] = rv;
        s1 += rv * (dinv[t] * rv);
        s2 += rv * rv;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s1 += __shfl_down(s1, off, 64);
      s2 += __shfl_down(s2, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      wsum[threadIdx.x >> 6][0] = s1;
      wsum[threadIdx.x >> 6][1] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 2)
      part[((int64_t)threadIdx.x * nvec + j) * gridDim.x + blockIdx.x] =
          (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
    __syncthreads();
  }
}
int launch_pcg_update(hfmi_ctx* ctx, double* y, int64_t ldy, double* r, int64_t ldr, const double* p, int64_t ldp,
                      const double* ap, int64_t ldap, const double* inv_diag, int64_t N, int nvec, const double* rz,
                      const double* pap, double* rz_new, double* rr) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  if (rr != rz_new + nvec) HFMI_FAIL(HFMI_ERR_INVALID, "pcg_update: rr must follow rz_new in memory");
  void* part = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_PART, (size_t)2 * nvec * PCG_CHUNKS * sizeof(double), &part));
  dim3 grid(PCG_CHUNKS, nvec < 1024 ? nvec : 1024);
  hipLaunchKernelGGL(k_pcg_update, grid, dim3(256), 0, ctx->stream, y, ldy, r, ldr, p, ldp, ap, ldap, inv_diag, N, nvec, rz,
                     pap, (double*)part);
  HIP_TRY(hipGetLastError());
  // the two partial arrays are laid out back to back as 2 * nvec "vectors": one final pass fills rz_new | rr
  return launch_dots_final(ctx, (const double*)part, PCG_CHUNKS, 2 * nvec, rz_new);
}
__global__ void k_pcg_direction(double* __restrict__ p, int64_t ldp, const double* __restrict__ r, int64_t ldr,
                                const double* __restrict__ dinv, int64_t N, int nvec, const double* __restrict__ num,
                                const double* __restrict__ den) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    const double b = den[j] != 0.0 ? num[j] / den[j] : 0.0;
    double* pc = p + (int64_t)j * ldp;
    const double* rc = r + (int64_t)j * ldr;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        d2 pv = *reinterpret_cast<d2*>(pc + t);
        const d2 rv = *reinterpret_cast<const d2*>(rc + t), dv = *reinterpret_cast<const d2*>(dinv + t);
        pv.x = dv.x * rv.x + b * pv.x;
        pv.y = dv.y * rv.y + b * pv.y;
        *reinterpret_cast<d2*>(pc + t) = pv;
      } else pc[t] = dinv[t] * rc[t] + b * pc[t];
    }
  }
}
int launch_pcg_direction(hfmi_ctx* ctx, double* p, int64_t ldp, const double* r, int64_t ldr, const double* inv_diag,
                         int64_t N, int nvec, const double* rz_new, const double* rz) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_pcg_direction, ew_grid(N, nvec), dim3(256), 0, ctx->stream, p, ldp, r, ldr, inv_diag, N, nvec, rz_new, rz);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// ------------------------------------------------------------------ host side of the sparse SPD solve
// Jacobi-preconditioned CG run on all vectors at once (independent recurrences, shared SpMM); per-vector scalars stay on the
// device, the host only polls convergence: every fourth iteration, and at the last one.
static int csr_block_cg(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_ctx* ctx = op->ctx;
  const hfmi_csr* M = op->csr;
  const int64_t N = W->N;
  const int k = W->nvec;
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
  HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->solve.inv_diag, N, k));
  HFMI_TRY(launch_copy(ctx, P.p, P.ld, Z.p, Z.ld, N, k));
  HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, k, rz));
  int it = 0;
  bool done = false;
  for (; it < op->max_iter && !done; ++it) {
    const bool poll = (it & 3) == 3 || it + 1 == op->max_iter;
    double* rr_done = rr;           // where this iteration leaves r.r (the CSR body: only when it is polled)
    if (M->ell_w > 0) {
      // three passes over the blocks per iteration: A p fused with p . A p; (x, r) update fused with both residual
      // dots; the new direction with z = D^-1 r recomputed on the fly (never stored)
      HFMI_TRY(launch_ell_spmm_dot(ctx, M, P.p, P.ld, AP.p, AP.ld, k, pap));
      HFMI_TRY(launch_pcg_update(ctx, Y->p, Y->ld, R.p, R.ld, P.p, P.ld, AP.p, AP.ld, M->solve.inv_diag, N, k, rz, pap, rz_new, rr));
      HFMI_TRY(launch_pcg_direction(ctx, P.p, P.ld, R.p, R.ld, M->solve.inv_diag, N, k, rz_new, rz));
      std::swap(rz, rz_new);        // the pair just written becomes "current"
      rr = rz_new + k;
    } else {
      HFMI_TRY(launch_csr_spmm(ctx, M, P.p, P.ld, AP.p, AP.ld, k, false));
      HFMI_TRY(launch_col_dots(ctx, P.p, P.ld, AP.p, AP.ld, N, k, pap));
      HFMI_TRY(launch_col_axpy_dev(ctx, Y->p, Y->ld, P.p, P.ld, N, k, rz, pap, 1.0));
      HFMI_TRY(launch_col_axpy_dev(ctx, R.p, R.ld, AP.p, AP.ld, N, k, rz, pap, -1.0));
      HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->solve.inv_diag, N, k));
      HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, k, rz_new));
      HFMI_TRY(launch_col_xpby_dev(ctx, P.p, P.ld, Z.p, Z.ld, N, k, rz_new, rz));
      HIP_TRY(hipMemcpyAsync(rz, rz_new, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      if (poll) HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, R.p, R.ld, N, k, rr));
    }
    if (!poll) continue;
    HFMI_TRY(read_back(ctx, rr_done, k, h_rr.data()));
    done = true;
    for (int j = 0; j < k; ++j)
      if (!(h_rr[j] <= op->rel_tol * op->rel_tol * h_bb[j])) done = false;
    for (int j = 0; j < k; ++j)
      if (!std::isfinite(h_rr[j]) || !std::isfinite(h_bb[j]))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "csr_pcg: non-finite residual in vector %d at iteration %d (matrix not SPD, or non-finite input)", j, it + 1);
  }
  op->last_iters = it;
  op->last_method = 0;
  if (!done) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "csr_pcg: no convergence to %.1e in %d iterations", op->rel_tol, op->max_iter);
  return HFMI_OK;
}

// Y = M^{-1} W for an SPD CSR matrix
int csr_pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  const hfmi_csr* M = op->csr;
  if (M->nrows != W->N) HFMI_FAIL(HFMI_ERR_INVALID, "csr_pcg: matrix has %lld rows, block vectors have %lld", (long long)M->nrows, (long long)W->N);
  HFMI_TRY(csr_prepare_jacobi(op->ctx, M));
  bool handled = false;
  HFMI_TRY(cheb_solve(op, W, Y, &handled));
  return handled ? HFMI_OK : csr_block_cg(op, W, Y);
}
