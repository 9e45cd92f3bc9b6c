// Device helpers of the kernels that work on ROW-MAJOR (nrows x k) arrays, entry (row, j) at [row * k + j]: the Chebyshev step and the
// per-column reductions (hfmi_cheb.hip), the sparse products of the V-cycle (hfmi_amg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// The tail of a per-column reduction: acc is what this thread summed of column j over its rows.  One partial per (column, workgroup)
// into part, summed over the row groups of the workgroup in a fixed order; sh: 256 doubles of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ void rm_col_partial(const rm_map& m, int k, int j, double acc, double* sh, double* part) {
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
