// Device helpers shared by the one-workgroup k x k kernels (hfmi_chol_col.hip, hfmi_chol.hip, hfmi_jacobi.hip, hfmi_lu.hip):
// workgroup reductions through LDS, the reciprocal square root of the serial chains, the folded-triangle index map.
#pragma once
#include <hip/hip_runtime.h>

constexpr double EPS_D = 2.220446049250313e-16;

__device__ __forceinline__ double block_sum(double v, double* scratch /* >= 16 doubles, LDS */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; ++w) s += scratch[w];
  return s;
}
__device__ __forceinline__ double block_min(double v, double* scratch) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = scratch[0];
  const int nw = blockDim.x >> 6;
  for (int w = 1; w < nw; ++w) s = fmin(s, scratch[w]);
  return s;
}

__device__ __forceinline__ double fast_rsqrt(double x) {
  // v_rsq_f64 is good to ~2^-26; ONE third-order step y0 (1 + e/2 + 3 e^2/8), e = 1 - x y0^2, leaves ~e^3 = 2^-78:
  // five dependent fp64 operations (32 cycles each on one CU) instead of the eight of two Newton steps -- this sits
  // on the serial chain of every Cholesky column and every Jacobi round.
  const double y0 = __builtin_amdgcn_rsq(x);
  const double e = fma(-(x * y0), y0, 1.0);
  const double q = e * fma(0.375, e, 0.5);
  return fma(y0, q, y0);
}
// cell e of the folded triangle {(row, col): 0 <= row <= col < n}: ceil(n/2) strips of n+1 cells, strip r holds
// row r (n-r cells) followed by row n-1-r (r+1 cells).  Returns false for the duplicate half of the middle strip.
__device__ __forceinline__ bool tri_cell(int e, int n, float inv_np1, int& row, int& col) {
  int r = (int)((float)e * inv_np1);
  int cc = e - r * (n + 1);
  if (cc < 0) {
    --r;
    cc += n + 1;
  } else if (cc > n) {
    ++r;
    cc -= n + 1;
  }
  if (cc < n - r) {
    row = r;
    col = r + cc;
    return true;
  }
  const int r2 = n - 1 - r;
  row = r2;
  col = r2 + (cc - (n - r));
  return r2 != r;
}
