// HBM-bound helper kernels on column-major blocks: fill/copy/scale/axpy, the Philox probe draw, layout conversion,
// per-vector dot products (deterministic) and the noise-precision applies.
#include "hfmi_internal.h"
#include "hfmi_randn_math.h"

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

__global__ void k_fill(double* __restrict__ p, int64_t rows, int nvec, int64_t ld, double value) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* c = p + (int64_t)j * ld;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < rows; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < rows) *reinterpret_cast<d2*>(c + t) = d2{value, value};
      else c[t] = value;
    }
  }
}
__global__ void k_zero_pad(double* __restrict__ p, int64_t N, int nvec, int64_t ld) {
  const int64_t padn = ld - N;
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* c = p + (int64_t)j * ld + N;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < padn; t += (int64_t)gridDim.x * blockDim.x) c[t] = 0.0;
  }
}
// Synthetic config-2 covariance: vector j of the block is column j of the Matern-3/2 kernel matrix
// sigma^2 (1 + a) exp(-a), a = sqrt(3) |x_i - x_j| / ell, over the first N nodes (row-major numbering) of an nx x ny grid
// on the unit square.  Written once per run; 16-byte stores.
__global__ void k_matern32(double* __restrict__ p, int64_t N, int nvec, int64_t ld, int nx, double hx, double hy, double sigma2,
                           double inv_ell) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* c = p + (int64_t)j * ld;
    const double xj = (j % nx) * hx, yj = (j / nx) * hy;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      double v[2];
      for (int e = 0; e < 2; ++e) {
        const int64_t i = t + e;
        const double dx = (i % nx) * hx - xj, dy = (i / nx) * hy - yj;
        const double a = 1.7320508075688772 * sqrt(dx * dx + dy * dy) * inv_ell;
        v[e] = sigma2 * (1.0 + a) * exp(-a);
      }
      if (t + 1 < N) *reinterpret_cast<d2*>(c + t) = d2{v[0], v[1]};
      else c[t] = v[0];
    }
  }
}
int launch_matern32(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld, int nx, int ny, double sigma, double ell) {
  hipLaunchKernelGGL(k_matern32, ew_grid(N, nvec), dim3(256), 0, ctx->stream, p, N, nvec, ld, nx, 1.0 / (nx - 1), 1.0 / (ny - 1),
                     sigma * sigma, 1.0 / ell);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// G (m x k, row-major, ld) <- diag(w) G: the diagonal of hp.LowRankOperator(d, U) between its two contractions
__global__ void k_row_scale(double* __restrict__ G, int ld, int m, int k, const double* __restrict__ w) {
  const int i = blockIdx.x;
  const double wi = w[i];
  for (int j = threadIdx.x; j < k; j += blockDim.x) G[(int64_t)i * ld + j] *= wi;
}
int launch_row_scale(hfmi_ctx* ctx, double* G, int ld, int m, int k, const double* w) {
  if (m <= 0 || k <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_row_scale, dim3(m), dim3(64), 0, ctx->stream, G, ld, m, k, w);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
int launch_fill(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld, double value, bool include_pad) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  const int64_t rows = include_pad ? ld : N;
  hipLaunchKernelGGL(k_fill, ew_grid(rows, nvec), dim3(256), 0, ctx->stream, p, rows, nvec, ld, value);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
int launch_zero_pad(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld) {
  if (ld <= N || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_zero_pad, dim3(1, nvec < 1024 ? nvec : 1024), dim3(64), 0, ctx->stream, p, N, nvec, ld);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

__global__ void k_copy(double* __restrict__ dst, int64_t ldd, const double* __restrict__ src, int64_t lds, int64_t N, int nvec) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* d = dst + (int64_t)j * ldd;
    const double* s = src + (int64_t)j * lds;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) *reinterpret_cast<d2*>(d + t) = *reinterpret_cast<const d2*>(s + t);
      else d[t] = s[t];
    }
  }
}
int launch_copy(hfmi_ctx* ctx, double* dst, int64_t ldd, const double* src, int64_t lds, int64_t N, int nvec) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_copy, ew_grid(N, nvec), dim3(256), 0, ctx->stream, dst, ldd, src, lds, N, nvec);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

__global__ void k_scale(double* __restrict__ p, int64_t ld, int64_t N, int nvec, double alpha) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* c = p + (int64_t)j * ld;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        d2 v = *reinterpret_cast<d2*>(c + t);
        v.x *= alpha; v.y *= alpha;
        *reinterpret_cast<d2*>(c + t) = v;
      } else c[t] *= alpha;
    }
  }
}
int launch_scale(hfmi_ctx* ctx, double* p, int64_t ld, int64_t N, int nvec, double alpha) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_scale, ew_grid(N, nvec), dim3(256), 0, ctx->stream, p, ld, N, nvec, alpha);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

__global__ void k_axpy(double* __restrict__ y, int64_t ldy, double alpha, const double* __restrict__ x, int64_t ldx, int64_t N, int nvec) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* yc = y + (int64_t)j * ldy;
    const double* xc = x + (int64_t)j * ldx;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        d2 v = *reinterpret_cast<d2*>(yc + t);
        const d2 u = *reinterpret_cast<const d2*>(xc + t);
        v.x += alpha * u.x; v.y += alpha * u.y;
        *reinterpret_cast<d2*>(yc + t) = v;
      } else yc[t] += alpha * xc[t];
    }
  }
}
int launch_axpy(hfmi_ctx* ctx, double* y, int64_t ldy, double alpha, const double* x, int64_t ldx, int64_t N, int nvec) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_axpy, ew_grid(N, nvec), dim3(256), 0, ctx->stream, y, ldy, alpha, x, ldx, N, nvec);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// ------------------------------------------------------------------ Philox4x32-10 + Box-Muller
// hfmi_randn_math.h: the integer generator, the range-specific fp64 functions and the element map (four normals per
// Philox output, rows 4g .. 4g+3 of column j from counter (g, j, stream)).  Thread = one row group per step, one 32-byte
// store; a wave writes 2 KiB contiguous.  VEC = false: blocks wrapped around foreign memory whose columns are not
// 32-byte aligned.
using hfmi_rng::philox4x32_10;
template <bool VEC>
__global__ __launch_bounds__(256) void k_randn(double* __restrict__ p, int64_t N, int nvec, int64_t ld, uint32_t k0, uint32_t k1,
                                               uint32_t stream, double sigma) {
  const int64_t nfull = N >> 2, ngroups = (N + 3) >> 2;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const hfmi_rng::normal_consts kc = hfmi_rng::make_consts(sigma);
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    double* c = p + (int64_t)j * ld;
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; g < nfull; g += step) {
      uint32_t x[4];
      double z[4];
      philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)j, stream, k0, k1, x);
      hfmi_rng::box_muller4(x, kc, z);
      if (VEC) *reinterpret_cast<d4*>(c + 4 * g) = d4{z[0], z[1], z[2], z[3]};
      else { c[4 * g] = z[0]; c[4 * g + 1] = z[1]; c[4 * g + 2] = z[2]; c[4 * g + 3] = z[3]; }
    }
    if (g < ngroups) {   // the ragged last group: one thread of the grid
      uint32_t x[4];
      double z[4];
      philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)j, stream, k0, k1, x);
      hfmi_rng::box_muller4(x, kc, z);
      for (int i = 0; i < 3; ++i) if (4 * g + i < N) c[4 * g + i] = z[i];
    }
  }
}
static inline dim3 randn_grid(int64_t N, int nvec) {
  const int64_t ngroups = (N + 3) / 4;
  int64_t gx = (ngroups + 256 * 4 - 1) / (256 * 4);   // ~4 row groups per thread
  if (gx < 1) gx = 1;
  if (gx > 4096) gx = 4096;
  return dim3((unsigned)gx, (unsigned)(nvec < 1024 ? nvec : 1024));
}
int launch_randn(hfmi_ctx* ctx, double* p, int64_t N, int nvec, int64_t ld, uint64_t seed, uint32_t stream, double sigma) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  if (sigma == 0.0) return launch_fill(ctx, p, N, nvec, ld, 0.0, false);
  const bool vec = ((uintptr_t)p % 32 == 0) && (ld % 4 == 0 || nvec == 1);
  if (vec) hipLaunchKernelGGL(k_randn<true>, randn_grid(N, nvec), dim3(256), 0, ctx->stream, p, N, nvec, ld, (uint32_t)seed, (uint32_t)(seed >> 32), stream, sigma);
  else hipLaunchKernelGGL(k_randn<false>, randn_grid(N, nvec), dim3(256), 0, ctx->stream, p, N, nvec, ld, (uint32_t)seed, (uint32_t)(seed >> 32), stream, sigma);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// the raw integer stream behind the draw: out[(j * ngroups + g) * 4 + 0..3], ngroups = ceil(N / 4)
__global__ void k_philox_raw(uint32_t* __restrict__ out, int64_t ngroups, int nvec, uint32_t k0, uint32_t k1, uint32_t stream) {
  for (int j = blockIdx.y; j < nvec; j += gridDim.y)
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
      uint32_t x[4];
      philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)j, stream, k0, k1, x);
      uint32_t* o = out + ((int64_t)j * ngroups + g) * 4;
      o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = x[3];
    }
}
int launch_philox_raw(hfmi_ctx* ctx, uint32_t* out, int64_t N, int nvec, uint64_t seed, uint32_t stream) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  hipLaunchKernelGGL(k_philox_raw, randn_grid(N, nvec), dim3(256), 0, ctx->stream, out, (N + 3) / 4, nvec, (uint32_t)seed, (uint32_t)(seed >> 32), stream);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// ------------------------------------------------------------------ dense (N x nvec, row-major) <-> block
// 32 x 32 tiles through LDS so both sides are read/written in 256-byte runs.
template <bool TO_BLOCK>
__global__ void k_transpose(const double* __restrict__ src, double* __restrict__ dst, int64_t ld, int64_t ldd, int64_t N, int nvec) {
  __shared__ double tile[32][33];
  const int64_t t0 = (int64_t)blockIdx.x * 32;
  const int j0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 32 x 8
  if (TO_BLOCK) {  // src dense[t*nvec + j], dst block[j*ld + t]
    for (int r = ty; r < 32; r += 8) {
      const int64_t t = t0 + r; const int j = j0 + tx;
      if (t < N && j < nvec) tile[r][tx] = src[t * ldd + j];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int j = j0 + r; const int64_t t = t0 + tx;
      if (t < N && j < nvec) dst[(int64_t)j * ld + t] = tile[tx][r];
    }
  } else {  // src block[j*ld + t], dst dense[t*nvec + j]
    for (int r = ty; r < 32; r += 8) {
      const int j = j0 + r; const int64_t t = t0 + tx;
      if (t < N && j < nvec) tile[r][tx] = src[(int64_t)j * ld + t];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
      const int64_t t = t0 + r; const int j = j0 + tx;
      if (t < N && j < nvec) dst[t * ldd + j] = tile[tx][r];
    }
  }
}
int launch_dense_to_block(hfmi_ctx* ctx, const double* dense, double* p, int64_t ld, int64_t N, int nvec) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  dim3 grid((unsigned)((N + 31) / 32), (unsigned)((nvec + 31) / 32));
  hipLaunchKernelGGL(k_transpose<true>, grid, dim3(256), 0, ctx->stream, dense, p, ld, (int64_t)nvec, N, nvec);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
int launch_block_to_dense_ld(hfmi_ctx* ctx, const double* p, int64_t ld, double* dense, int64_t ldd, int64_t N, int nvec) {
  if (N <= 0 || nvec <= 0) return HFMI_OK;
  dim3 grid((unsigned)((N + 31) / 32), (unsigned)((nvec + 31) / 32));
  hipLaunchKernelGGL(k_transpose<false>, grid, dim3(256), 0, ctx->stream, p, dense, ld, ldd, N, nvec);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
int launch_block_to_dense(hfmi_ctx* ctx, const double* p, int64_t ld, double* dense, int64_t N, int nvec) {
  return launch_block_to_dense_ld(ctx, p, ld, dense, nvec, N, nvec);
}

// ------------------------------------------------------------------ per-vector dot products (deterministic)
// grid (chunks, vectors): wave-64 shuffle reduction -> LDS across the 4 waves -> one partial per block;
// a second kernel adds the partials in a fixed order.
constexpr int DOT_CHUNKS = 64;
__global__ void k_col_dots_partial(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                   int64_t N, int nvec, double* __restrict__ part) {
  __shared__ double wsum[4];
  for (int j = blockIdx.y; j < nvec; j += gridDim.y) {
    const double* a = A + (int64_t)j * lda;
    const double* b = B + (int64_t)j * ldb;
    double s = 0.0;
    for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; t < N; t += (int64_t)gridDim.x * blockDim.x * 2) {
      if (t + 1 < N) {
        const d2 u = *reinterpret_cast<const d2*>(a + t), v = *reinterpret_cast<const d2*>(b + t);
        s += u.x * v.x + u.y * v.y;
      } else s += a[t] * b[t];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)j * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}
// one wave per output: lanes stride over the partials, then a fixed-order shuffle tree (deterministic); the serial
// version of this loop cost 50-100 us per call once a fused kernel produced a few hundred partials per vector
__global__ __launch_bounds__(64) void k_col_dots_final(const double* __restrict__ part, int nchunks, int nvec,
                                                       double* __restrict__ out) {
  const int j = blockIdx.x;
  if (j >= nvec) return;
  const double* p = part + (int64_t)j * nchunks;
  double s = 0.0;
  for (int c = threadIdx.x; c < nchunks; c += 64) s += p[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) out[j] = s;
}
int launch_dots_final(hfmi_ctx* ctx, const double* part, int nchunks, int nvec, double* out) {
  hipLaunchKernelGGL(k_col_dots_final, dim3(nvec), dim3(64), 0, ctx->stream, part, nchunks, nvec, out);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
int launch_col_dots(hfmi_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, int64_t N, int nvec, double* out) {
  if (nvec <= 0) return HFMI_OK;
  void* part = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_PART, (size_t)nvec * DOT_CHUNKS * sizeof(double), &part));
  dim3 grid(DOT_CHUNKS, nvec < 1024 ? nvec : 1024);
  hipLaunchKernelGGL(k_col_dots_partial, grid, dim3(256), 0, ctx->stream, A, lda, B, ldb, N, nvec, (double*)part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_col_dots_final, dim3(nvec), dim3(64), 0, ctx->stream, (const double*)part, DOT_CHUNKS, nvec, out);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// G_i <- Gamma G_i for every sample's q x k slab (noise precision, operatorWrappers.py:107-109).  One
// workgroup per sample, slab staged in LDS (q*k*8 bytes: 100 x 74 -> 59 KB).
__global__ void k_gamma_apply(double* __restrict__ G, int ldg, int q, int k, const double* __restrict__ gamma, int ldgam) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* slab = reinterpret_cast<double*>(smem);
  double* Gi = G + (int64_t)blockIdx.x * q * ldg;
  for (int e = threadIdx.x; e < q * k; e += blockDim.x) slab[e] = Gi[(int64_t)(e / k) * ldg + (e % k)];
  __syncthreads();
  for (int e = threadIdx.x; e < q * k; e += blockDim.x) {
    const int o = e / k, j = e % k;
    double s = 0.0;
    for (int p = 0; p < q; ++p) s += gamma[o * ldgam + p] * slab[p * k + j];
    Gi[(int64_t)o * ldg + j] = s;
  }
}
int launch_gamma_apply(hfmi_ctx* ctx, double* G, int ldg, int ndata, int q, int k, const double* gamma, int ldgam) {
  const size_t shmem = (size_t)q * k * sizeof(double);
  if (shmem > 150 * 1024) HFMI_FAIL(HFMI_ERR_INVALID, "gamma_apply: q*k slab (%zu bytes) exceeds LDS", shmem);
  HIP_TRY(hipFuncSetAttribute((const void*)k_gamma_apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(k_gamma_apply, dim3(ndata), dim3(256), shmem, ctx->stream, G, ldg, q, k, gamma, ldgam);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// column-major variant for the Rayleigh-quotient shortcut: Gc is (ndata*q) x k with leading dimension ld (one
// column per probe vector); out[:, j] slab i = Gamma * Gc[:, j] slab i
__global__ void k_gamma_apply_cm(const double* __restrict__ Gc, double* __restrict__ out, int64_t ld, int q, int k,
                                 const double* __restrict__ gamma, int ldgam) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* slab = reinterpret_cast<double*>(smem);     // [k][q]
  const int64_t base = (int64_t)blockIdx.x * q;
  for (int e = threadIdx.x; e < q * k; e += blockDim.x) {
    const int j = e / q, o = e % q;
    slab[e] = Gc[(int64_t)j * ld + base + o];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < q * k; e += blockDim.x) {
    const int j = e / q, o = e % q;
    double s = 0.0;
    for (int p = 0; p < q; ++p) s += gamma[o * ldgam + p] * slab[j * q + p];
    out[(int64_t)j * ld + base + o] = s;
  }
}
int launch_gamma_apply_cm(hfmi_ctx* ctx, const double* Gc, double* out, int64_t ld, int ndata, int q, int k, const double* gamma,
                          int ldgam) {
  const size_t shmem = (size_t)q * k * sizeof(double);
  if (shmem > 150 * 1024) HFMI_FAIL(HFMI_ERR_INVALID, "gamma_apply: q*k slab (%zu bytes) exceeds LDS", shmem);
  HIP_TRY(hipFuncSetAttribute((const void*)k_gamma_apply_cm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  hipLaunchKernelGGL(k_gamma_apply_cm, dim3(ndata), dim3(256), shmem, ctx->stream, Gc, out, ld, q, k, gamma, ldgam);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
