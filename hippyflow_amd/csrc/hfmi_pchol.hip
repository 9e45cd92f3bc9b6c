// Greedy (diagonally pivoted) partial Cholesky factorisation  C ~= L L^T  of a kernel covariance (hfmi_pchol_*, include/hfmi.h).
// It reads the diagonal of C and the k pivot columns only: N k^2 flops and 4 N k^2 bytes for rank k, against 2 N^2 k flops for ONE apply
// of the matrix-free operator (hfmi_kcov.hip).  The trace of the residual C - L L^T (positive semidefinite) comes with it and bounds the
// error of every eigenvalue of L L^T.
//
//   d0 = sigma^2 + nugget;  diag[i] = d0;  trace[0] = sum(diag);  floor = 4 kmax eps d0
//   step j:  (p, dp) = argmax diag, ties to the LOWEST index;  stop when trace[j] <= rel_tol trace[0] (REL_TOL) or dp <= floor (FLOOR)
//            L[i,j] = (C(i,p) - sum_{c<j} L[i,c] L[p,c]) / sqrt(dp)   (one fma chain, c ascending; sqrt(dp) itself for i == p)
//            diag[i] = max(diag[i] - L[i,j]^2, 0),  diag[p] = 0;  trace[j+1] = sum(diag)
//
// Launches of a step: k_pchol_gather_row copies row p of L (j scattered doubles) into a contiguous buffer; k_pchol_column computes the
// column with lanes along i (every column of L is read in 512-byte pieces per wave; a step is HBM-bound at 8 N j bytes), the row of the
// pivot staged through LDS PC_CHUNK columns at a time (all lanes read the same LDS word: a broadcast), and leaves one (max, lowest index,
// sum) of the new diagonal per workgroup; k_pchol_pick reduces those to (next pivot, its diagonal, trace) in ONE workgroup.  The host reads
// these 24 bytes back after every step and decides whether to go on.  No atomics anywhere: every sum and every arg-max has a fixed order
// (per thread over its row tiles in order, a shuffle tree per wave, the waves in order, the workgroups in order), so two factorisations of
// the same input on the same device are bit-identical.  The CPU twin tests/helpers/pchol_twin.py walks the same steps.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <type_traits>

#include "hfmi_kcov_eval.h"

#define PC_CHUNK 256        // columns of the pivot's row per LDS chunk (exported to Python as _lib.PC_CHUNK)
#define PC_THREADS 256      // rows per tile: one row per lane
#define PC_WAVES (PC_THREADS / 64)

struct pc_pick {            // what the host reads back after a step
  double dp;                // largest remaining diagonal entry
  long long p;              // its lowest index
  double trace;             // sum of the remaining diagonal
};

// (bv, bi, bs) of all threads of the workgroup -> thread 0; fixed order
__device__ __forceinline__ void pc_block_reduce(double& bv, long long& bi, double& bs) {
  __shared__ double rv[PC_WAVES], rs[PC_WAVES];
  __shared__ long long ri[PC_WAVES];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(bv, off);
    const long long oi = __shfl_down(bi, off);
    const double os = __shfl_down(bs, off);
    if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    bs += os;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) rv[wave] = bv, ri[wave] = bi, rs[wave] = bs;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < PC_WAVES; ++w) {
      if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) bv = rv[w], bi = ri[w];
      bs += rs[w];
    }
  }
}

// diag[i] = d0 and the workgroup's (max, lowest index, sum)
__global__ __launch_bounds__(PC_THREADS) void k_pchol_init(int64_t N, double d0, double* __restrict__ diag, double* __restrict__ pmax,
                                                           long long* __restrict__ pidx, double* __restrict__ psum) {
  double bv = -1.0, bs = 0.0;
  long long bi = LLONG_MAX;
  const int64_t ntiles = (N + PC_THREADS - 1) / PC_THREADS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i = tile * PC_THREADS + threadIdx.x;
    if (i < N) {
      diag[i] = d0;
      if (d0 > bv) bv = d0, bi = i;
      bs += d0;
    }
  }
  pc_block_reduce(bv, bi, bs);
  if (threadIdx.x == 0) pmax[blockIdx.x] = bv, pidx[blockIdx.x] = bi, psum[blockIdx.x] = bs;
}

// prow[c] = L[p, c] for c < j
__global__ __launch_bounds__(PC_THREADS) void k_pchol_gather_row(const double* __restrict__ L, int64_t ld, int64_t p, int j,
                                                                 double* __restrict__ prow) {
  const int c = blockIdx.x * PC_THREADS + threadIdx.x;
  if (c < j) prow[c] = L[(int64_t)c * ld + p];
}

// column j of L from the pivot (p, dp), the new diagonal and the workgroup's (max, lowest index, sum) of it.  PT: kcov_params, or
// kcov_k1_params for Matern-1, kcov_nu_params for a Matern of any smoothness (the entry behind kcov_entry is what differs)
template <class PT>
__global__ __launch_bounds__(PC_THREADS) void k_pchol_column(PT P, double* __restrict__ L, int64_t ld, int j, int64_t p, double dp,
                                                             const double* __restrict__ prow, double* __restrict__ diag,
                                                             double* __restrict__ pmax, long long* __restrict__ pidx,
                                                             double* __restrict__ psum) {
  __shared__ double pl[PC_CHUNK];
  const int64_t N = P.N;
  const int d = P.d;
  const double root = sqrt(dp);
  const double xp0 = P.x0[p];
  const double xp1 = d > 1 ? P.x1[p] : 0.0;
  const double xp2 = d > 2 ? P.x2[p] : 0.0;
  double* __restrict__ Lj = L + (int64_t)j * ld;
  double bv = -1.0, bs = 0.0;
  long long bi = LLONG_MAX;
  const int64_t ntiles = (N + PC_THREADS - 1) / PC_THREADS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i = tile * PC_THREADS + threadIdx.x;
    const bool valid = i < N;
    const double* Li = L + i;
    double s = 0.0;
    for (int c0 = 0; c0 < j; c0 += PC_CHUNK) {
      const int nc = min(PC_CHUNK, j - c0);
      __syncthreads();          // every wave is done with the previous chunk
      if ((int)threadIdx.x < nc) pl[threadIdx.x] = prow[c0 + threadIdx.x];
      __syncthreads();
      if (valid) {
        const double* Lc = Li + (int64_t)c0 * ld;
#pragma unroll 8
        for (int c = 0; c < nc; ++c) s = fma(Lc[(int64_t)c * ld], pl[c], s);
      }
    }
    if (valid) {
      double v = root, dn = 0.0;
      if (i != p) {
        const double dx = P.x0[i] - xp0;
        double r2 = dx * dx;
        if (d > 1) {
          const double dy = P.x1[i] - xp1;
          r2 = fma(dy, dy, r2);
        }
        if (d > 2) {
          const double dz = P.x2[i] - xp2;
          r2 = fma(dz, dz, r2);
        }
        const double c = kcov_entry(P, r2, false);
        {
#pragma clang fp contract(off)      // the entry is rounded as k_kcov rounds it before s is taken off
          v = (c - s) / root;
        }
        dn = fmax(fma(-v, v, diag[i]), 0.0);
      }
      Lj[i] = v;
      diag[i] = dn;
      if (dn > bv) bv = dn, bi = i;     // i ascends within a thread: strictly greater keeps the lowest index
      bs += dn;
    }
  }
  pc_block_reduce(bv, bi, bs);
  if (threadIdx.x == 0) pmax[blockIdx.x] = bv, pidx[blockIdx.x] = bi, psum[blockIdx.x] = bs;
}

// the nb workgroup results -> out, one workgroup: thread t takes t, t + PC_THREADS, ... in order
__global__ __launch_bounds__(PC_THREADS) void k_pchol_pick(int nb, const double* __restrict__ pmax, const long long* __restrict__ pidx,
                                                           const double* __restrict__ psum, pc_pick* __restrict__ out) {
  double bv = -1.0, bs = 0.0;
  long long bi = LLONG_MAX;
  for (int b = threadIdx.x; b < nb; b += PC_THREADS) {
    if (pmax[b] > bv || (pmax[b] == bv && pidx[b] < bi)) bv = pmax[b], bi = pidx[b];
    bs += psum[b];
  }
  pc_block_reduce(bv, bi, bs);
  if (threadIdx.x == 0) out->dp = bv, out->p = bi, out->trace = bs;
}

// ("pchol_grid", n) of hfmi_tuning_set: at most n workgroups per launch (0 = as many as the device holds).  For tests: a small grid makes
// every workgroup walk several row tiles at sizes where the result can be checked densely.  L and the pivots do not depend on it (a row's
// chain and the arg-max are exact in any grouping); the traces do in their last bits (another grouping of the same sum).
static int g_pchol_grid = 0;
int pchol_tuning_set(const char* key, int value) {
  if (key && !strcmp(key, "pchol_grid") && value >= 0 && value <= 65535) {
    g_pchol_grid = value;
    return 1;
  }
  return 0;
}

struct hfmi_pchol {
  ~hfmi_pchol() {           // the storage goes back where it came from; the pool keeps it in stream order
    if (!p) return;
    (void)hipSetDevice(ctx->device);
    pool_release(ctx, p, bytes);
  }
  hfmi_ctx* ctx = nullptr;
  double* p = nullptr;      // the factor's storage: max_rank columns from the block allocator, padding rows and unused columns +0.0
  size_t bytes = 0;
  hfmi_block L = {};        // the first `rank` columns, by value (a view, not an owner)
  int rank = 0, stop_reason = HFMI_PCHOL_MAX_RANK;
  std::vector<int64_t> pivots;
  std::vector<double> trace;
};

static int pc_read_pick(hfmi_ctx* ctx, const pc_pick* dev, pc_pick* host) {
  double w[3];
  static_assert(sizeof(pc_pick) == sizeof(w), "pc_pick is three 8-byte words");
  HFMI_TRY(read_back(ctx, (const double*)dev, 3, w));
  memcpy(host, w, sizeof(w));
  return HFMI_OK;
}

template <class PT>
static int pchol_run(hfmi_pchol* h, const hfmi_op* op, int kmax, double rel_tol, double* scratch, int grid) {
  hfmi_ctx* ctx = h->ctx;
  const int64_t N = op->kc_N, ld = h->L.ld;
  PT P;
  if constexpr (std::is_same<PT, kcov_nu_params>::value)
    HFMI_TRY(kcov_nu_params_init_as(&P, op->kc_x, N, op->kc_d, op->kc_family, op->kc_sigma, op->kc_ell, op->kc_nugget, op->kc_nu_ref()));
  else
    HFMI_TRY(kcov_params_init_as(&P, op->kc_x, N, op->kc_d, op->kc_family, op->kc_sigma, op->kc_ell, op->kc_nugget));
  // scratch: diag[N] | prow[kmax] | pmax[grid] | psum[grid] | pidx[grid] | pick
  double* diag = scratch;
  double* prow = diag + N;
  double* pmax = prow + kmax;
  double* psum = pmax + grid;
  long long* pidx = (long long*)(psum + grid);
  pc_pick* pick_dev = (pc_pick*)(pidx + grid);
  const double d0 = P.sigma2 + P.nugget;
  const double floor_ = 4.0 * kmax * DBL_EPSILON * d0;
  pc_pick pick;
  hipLaunchKernelGGL(k_pchol_init, dim3(grid), dim3(PC_THREADS), 0, ctx->stream, N, d0, diag, pmax, pidx, psum);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_pchol_pick, dim3(1), dim3(PC_THREADS), 0, ctx->stream, grid, pmax, pidx, psum, pick_dev);
  HIP_TRY(hipGetLastError());
  HFMI_TRY(pc_read_pick(ctx, pick_dev, &pick));
  h->trace.push_back(pick.trace);
  h->stop_reason = HFMI_PCHOL_MAX_RANK;
  int j = 0;
  for (; j < kmax; ++j) {
    if (!(pick.trace > rel_tol * h->trace[0])) {
      h->stop_reason = HFMI_PCHOL_REL_TOL;
      break;
    }
    if (!(pick.dp > floor_)) {
      h->stop_reason = HFMI_PCHOL_FLOOR;
      break;
    }
    if (pick.p < 0 || pick.p >= N) HFMI_FAIL(HFMI_ERR_NUMERIC, "pchol: step %d picked row %lld of %lld", j, pick.p, (long long)N);
    if (j > 0) {
      hipLaunchKernelGGL(k_pchol_gather_row, dim3((j + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, ctx->stream, h->p, ld,
                         (int64_t)pick.p, j, prow);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pchol_column<PT>, dim3(grid), dim3(PC_THREADS), 0, ctx->stream, P, h->p, ld, j, (int64_t)pick.p, pick.dp, prow, diag,
                       pmax, pidx, psum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pchol_pick, dim3(1), dim3(PC_THREADS), 0, ctx->stream, grid, pmax, pidx, psum, pick_dev);
    HIP_TRY(hipGetLastError());
    h->pivots.push_back(pick.p);
    HFMI_TRY(pc_read_pick(ctx, pick_dev, &pick));
    h->trace.push_back(pick.trace);
  }
  h->rank = j;
  h->L.nvec = j;
  return HFMI_OK;
}

extern "C" int hfmi_pchol_create(hfmi_op* op, int max_rank, double rel_tol, hfmi_pchol** out) {
  if (!op || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (op->kind != OP_KERNEL_COV) HFMI_FAIL(HFMI_ERR_INVALID, "pchol: the operator is not a kernel covariance (hfmi_op_kernel_cov)");
  if (max_rank < 1 || max_rank > HFMI_EIG_MAXN)
    HFMI_FAIL(HFMI_ERR_INVALID, "pchol: max_rank = %d outside 1..%d (the largest Gram eigenproblem)", max_rank, HFMI_EIG_MAXN);
  if (!(rel_tol >= 0.0) || !isfinite(rel_tol)) HFMI_FAIL(HFMI_ERR_INVALID, "pchol: rel_tol must be finite and not negative");
  hfmi_ctx* ctx = op->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t N = op->kc_N;
  const int kmax = (int)std::min<int64_t>(max_rank, N);
  int per_cu = 0;
  const bool k1 = op->kc_family == HFMI_KERNEL_MATERN1;
  const bool knu = op->kc_family == HFMI_KERNEL_MATERN;
  if (knu) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pchol_column<kcov_nu_params>, PC_THREADS, 0));
  else if (k1) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pchol_column<kcov_k1_params>, PC_THREADS, 0));
  else HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pchol_column<kcov_params>, PC_THREADS, 0));
  if (per_cu < 1) per_cu = 1;
  const int64_t ntiles = (N + PC_THREADS - 1) / PC_THREADS;
  int grid = (int)std::min<int64_t>(ntiles, (int64_t)per_cu * ctx->num_cus);
  if (g_pchol_grid > 0) grid = std::min(grid, g_pchol_grid);
  std::unique_ptr<hfmi_pchol> h(new (std::nothrow) hfmi_pchol());
  if (!h) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  h->ctx = ctx;
  hfmi_block* b = nullptr;
  HFMI_TRY(block_alloc(ctx, N, kmax, &b));
  h->L = *b;
  h->L.owner = false;
  h->p = b->p;
  h->bytes = (size_t)b->ld * kmax * sizeof(double);
  delete b;
  dev_buf<double> scratch;
  const size_t scratch_doubles = (size_t)N + kmax + 3 * (size_t)grid + sizeof(pc_pick) / sizeof(double);
  int s = HFMI_OK;
  hipError_t e = hipMemsetAsync(h->p, 0, h->bytes, ctx->stream);
  if (e == hipSuccess) e = (hipError_t)scratch.alloc(scratch_doubles);
  if (e != hipSuccess) {
    hfmi_set_error("pchol: %s", hipGetErrorString(e));
    s = HFMI_ERR_HIP;
  } else {
    s = knu ? pchol_run<kcov_nu_params>(h.get(), op, kmax, rel_tol, scratch, grid)
        : k1 ? pchol_run<kcov_k1_params>(h.get(), op, kmax, rel_tol, scratch, grid) : pchol_run<kcov_params>(h.get(), op, kmax, rel_tol, scratch, grid);
  }
  (void)hipStreamSynchronize(ctx->stream);      // before the scratch goes
  if (s != HFMI_OK) return s;
  *out = h.release();
  return HFMI_OK;
}
extern "C" int hfmi_pchol_info(const hfmi_pchol* h, int* rank, int* stop_reason, double* trace0) {
  if (!h) HFMI_FAIL(HFMI_ERR_INVALID, "null factorisation");
  if (rank) *rank = h->rank;
  if (stop_reason) *stop_reason = h->stop_reason;
  if (trace0) *trace0 = h->trace[0];
  return HFMI_OK;
}
extern "C" int hfmi_pchol_read(const hfmi_pchol* h, int64_t* host_pivots, double* host_trace) {
  if (!h) HFMI_FAIL(HFMI_ERR_INVALID, "null factorisation");
  if (host_pivots) std::copy(h->pivots.begin(), h->pivots.end(), host_pivots);
  if (host_trace) std::copy(h->trace.begin(), h->trace.end(), host_trace);
  return HFMI_OK;
}
extern "C" int hfmi_pchol_factor(const hfmi_pchol* h, const hfmi_block** L) {
  if (!h || !L) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (h->rank < 1) HFMI_FAIL(HFMI_ERR_INVALID, "pchol: the factor has rank 0 (no step was taken: stop reason %d)", h->stop_reason);
  *L = &h->L;
  return HFMI_OK;
}
extern "C" int hfmi_pchol_destroy(hfmi_pchol* h) {
  delete h;
  return HFMI_OK;
}
