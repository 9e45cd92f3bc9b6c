// Scattered points on the FFT route: the sparse cubic interpolation W from the nodes of a regular grid to N points
// (hfmi_op_grid_interp), and the interpolated grid covariance  K = W Cg W^T + diag(delta)  as one operator (hfmi_op_kernel_cov_interp)
// with its draws (hfmi_interp_sampler_draw) and its factor K = F F^T (hfmi_op_interp_factor).  Every rule -- the cell of a point, Keys' weights, the stencil order, the cell binning
// and the spread order, the autocorrelation form of the diagonal, the launch shapes -- is in hfmi_interp_plan.h; the weights are
// computed there, on the host, and uploaded.  This unit holds the kernels, the state and the launchers.
//
// Device layout (binned order: position k is point perm[k], the points of a cell contiguous, cells ascending):  base[k] the node of
// the stencil corner, w[(4 a + s) N + k] weight s of axis a, delta[k] / sdelta[k] the diagonal and its square root.  That is 4 d
// doubles and two indices per point against the 4^d (value, index) pairs of a CSR row per orientation; the products are formed in
// registers.
//
// k_interp_gather  Y (+)= W G (+ delta . X, or + sqrt(delta) . eta with eta generated): a thread takes a point in binned order, keeps
//   its weights in registers and walks the columns; neighbouring threads read neighbouring grid lines, each result goes to its own row.
// k_interp_spread  G (+)= W^T X: a thread owns a grid node, visits the cells that reach it and their points in the contract's order
//   and carries INTERP_SPREAD_COLS columns per trip.  No atomics.  Heavily clustered points make the threads of a few nodes long: that
//   imbalance is accepted here, not solved.
// k_interp_diag    q_i from the 7^d table of the kernel and the per-axis autocorrelations of the weights, once at creation.
// k_interp_factor_tail  Z (+)= sqrt(delta) . X in point order, the last N rows of F^T X: a stream, one multiplication per entry.
// The first three are gathers bound by latency, not bandwidth (docs/measurements.md, "Interpolated grid covariance": a few per cent of the HBM
// rate at N = 1e6, 0.47 to 0.82 of the time of the CSR-composed K); none has been tuned beyond its access pattern.
#include <math.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "hfmi_internal.h"
#include "hfmi_interp_plan.h"
#include "hfmi_randn_math.h"

struct interp_state {
  interp_grid g;
  int64_t N = 0;
  dev_buf<int64_t> base, perm, cell_start;
  dev_buf<double> w;
  // hfmi_op_kernel_cov_interp
  dev_buf<double> delta, sdelta;         // binned order
  std::vector<double> host_q, host_delta;   // point order: q_i = (W Cg W^T)_ii and delta_i
  double diag_min = 0.0, diag_max = 0.0;    // extremes of sigma^2 - q_i
  int64_t n_clipped = 0;
  dev_buf<double> work;                  // the internal block of work_ld rows, a chunk of columns
  int64_t work_ld = 0;
  dev_buf<double> sdelta_pt;             // sqrt(delta) in POINT order: the tail of F^T streams over it (made by the first hfmi_op_interp_factor)
};

void interp_destroy(interp_state* st) { delete st; }
int64_t interp_range_len(const hfmi_op* op) {
  if (op->kind == OP_INTERP_FACTOR) return op->ip_grid->ip->N + (op->fac_transpose ? fftcov_padded_len(op->fac.get()) : 0);
  return op->ip_transpose ? op->ip->g.nnodes : op->ip->N;
}

struct interp_args {
  const int64_t* base;
  const int64_t* perm;
  const int64_t* cell_start;
  const double* w;
  int64_t N;
  int64_t n0, n1, n2;       // nodes per axis
  int64_t nc0, nc1, nc2;    // cells per axis
  int64_t nnodes;
  const double* in;         // gather: G (nnodes rows); spread: X (N rows)
  int64_t ldin;
  double* out;
  int64_t ldout;
  int ncols, accumulate;
  const double* diag;       // gather epilogue: delta (EPI_DIAG) or sqrt(delta) (EPI_NOISE), binned order
  const double* X;          // EPI_DIAG: the second block, N rows
  int64_t ldx;
  uint32_t k0, k1;          // EPI_NOISE: the key; column j is vector index first + j of stream 0
  int64_t first;
};

enum { EPI_NONE = 0, EPI_DIAG = 1, EPI_NOISE = 2 };

template <int D, int EPI>
__global__ __launch_bounds__(INTERP_THREADS) void k_interp_gather(interp_args A) {
  const int64_t N = A.N;
  hfmi_rng::normal_consts kc{};
  if constexpr (EPI == EPI_NOISE) kc = hfmi_rng::make_consts(1.0);
  for (int64_t k = (int64_t)blockIdx.x * INTERP_THREADS + threadIdx.x; k < N; k += (int64_t)gridDim.x * INTERP_THREADS) {
    const int64_t b = A.base[k], i = A.perm[k];
    double w0[4], w1[4], w2[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      w0[s] = A.w[(int64_t)s * N + k];
      w1[s] = D > 1 ? A.w[(int64_t)(4 + s) * N + k] : 1.0;
      w2[s] = D > 2 ? A.w[(int64_t)(8 + s) * N + k] : 1.0;
    }
    double dg = 0.0;
    if constexpr (EPI != EPI_NONE) dg = A.diag[k];
    for (int j = blockIdx.y; j < A.ncols; j += gridDim.y) {
      const double* g = A.in + (int64_t)j * A.ldin + b;
      double acc = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < (D > 2 ? 4 : 1); ++s2) {
#pragma unroll
        for (int s1 = 0; s1 < (D > 1 ? 4 : 1); ++s1) {
          const double* row = g + (int64_t)s1 * A.n0 + (int64_t)s2 * A.n0 * A.n1;
#pragma unroll
          for (int s0 = 0; s0 < 4; ++s0) {
            const double wt = D > 2 ? (w2[s2] * w1[s1]) * w0[s0] : D > 1 ? w1[s1] * w0[s0] : w0[s0];
            acc = fma(wt, row[s0], acc);
          }
        }
      }
      if constexpr (EPI == EPI_DIAG) acc = fma(dg, A.X[(int64_t)j * A.ldx + i], acc);
      if constexpr (EPI == EPI_NOISE) {
        // row i of vector first + j in the element map of the probe draw (hfmi_randn_math.h): rows 4 g .. 4 g + 3 from one Philox output
        const int64_t grp = i >> 2;
        uint32_t r[4];
        double z[4];
        hfmi_rng::philox4x32_10((uint32_t)grp, (uint32_t)(grp >> 32), (uint32_t)(A.first + j), 0u, A.k0, A.k1, r);
        hfmi_rng::box_muller4(r, kc, z);
        const int q = (int)(i & 3);
        const double eta = q == 0 ? z[0] : q == 1 ? z[1] : q == 2 ? z[2] : z[3];
        acc = fma(dg, eta, acc);
      }
      double* y = A.out + (int64_t)j * A.ldout + i;
      *y = A.accumulate ? *y + acc : acc;
    }
  }
}

template <int D>
__global__ __launch_bounds__(INTERP_THREADS) void k_interp_spread(interp_args A) {
  constexpr int CT = INTERP_SPREAD_COLS;
  const int64_t N = A.N;
  for (int64_t g = (int64_t)blockIdx.x * INTERP_THREADS + threadIdx.x; g < A.nnodes; g += (int64_t)gridDim.x * INTERP_THREADS) {
    const int64_t g0 = g % A.n0, g1 = D > 1 ? (g / A.n0) % A.n1 : 0, g2 = D > 2 ? g / (A.n0 * A.n1) : 0;
    const int64_t lo0 = g0 > 3 ? g0 - 3 : 0, hi0 = g0 < A.nc0 ? g0 : A.nc0 - 1;
    const int64_t lo1 = D > 1 ? (g1 > 3 ? g1 - 3 : 0) : 0, hi1 = D > 1 ? (g1 < A.nc1 ? g1 : A.nc1 - 1) : 0;
    const int64_t lo2 = D > 2 ? (g2 > 3 ? g2 - 3 : 0) : 0, hi2 = D > 2 ? (g2 < A.nc2 ? g2 : A.nc2 - 1) : 0;
    for (int j0 = (int)blockIdx.y * CT; j0 < A.ncols; j0 += (int)gridDim.y * CT) {
      double acc[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = 0.0;
      for (int64_t q2 = lo2; q2 <= hi2; ++q2)
        for (int64_t q1 = lo1; q1 <= hi1; ++q1)
          for (int64_t q0 = lo0; q0 <= hi0; ++q0) {
            const int64_t cell = q0 + A.nc0 * (q1 + A.nc1 * q2);
            const int64_t kb = A.cell_start[cell], ke = A.cell_start[cell + 1];
            const double* p0 = A.w + (g0 - q0) * N;
            const double* p1 = A.w + (4 + (g1 - q1)) * N;
            const double* p2 = A.w + (8 + (g2 - q2)) * N;
            for (int64_t k = kb; k < ke; ++k) {
              const double wt = D > 2 ? (p2[k] * p1[k]) * p0[k] : D > 1 ? p1[k] * p0[k] : p0[k];
              const double* x = A.in + A.perm[k];
#pragma unroll
              for (int c = 0; c < CT; ++c)
                if (j0 + c < A.ncols) acc[c] = fma(wt, x[(int64_t)(j0 + c) * A.ldin], acc[c]);
            }
          }
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (j0 + c < A.ncols) {
          double* y = A.out + (int64_t)(j0 + c) * A.ldout + g;
          *y = A.accumulate ? *y + acc[c] : acc[c];
        }
    }
  }
}

// The tail of F^T: Z[i, j] (+)= sqrt(delta_i) X[i, j], everything in POINT order.  A stream: x over the points (neighbouring threads
// take neighbouring rows of sd, X and Z), y over the columns, one multiplication per entry, no LDS, no atomics.  The product is rounded
// before an accumulating apply adds it (no contraction), so an accumulated tail is what was there plus the overwriting one.
__global__ __launch_bounds__(INTERP_THREADS) void k_interp_factor_tail(const double* __restrict__ sd, int64_t N, const double* __restrict__ X,
                                                                        int64_t ldx, double* __restrict__ Z, int64_t ldz, int ncols,
                                                                        int accumulate) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * INTERP_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * INTERP_THREADS) {
    const double s = sd[i];
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
      const double t = s * X[(int64_t)j * ldx + i];
      double* z = Z + (int64_t)j * ldz + i;
      *z = accumulate ? *z + t : t;
    }
  }
}

// a_a[o], o = 0 .. 3, of one axis' four weights (hfmi_interp_plan.h)
__device__ __forceinline__ void interp_autocorr(const double (&w)[4], double (&a)[4]) {
  a[0] = fma(w[3], w[3], fma(w[2], w[2], fma(w[1], w[1], w[0] * w[0])));
  a[1] = fma(w[3], w[2], fma(w[2], w[1], w[1] * w[0]));
  a[2] = fma(w[3], w[1], w[2] * w[0]);
  a[3] = w[3] * w[0];
}

template <int D>
__global__ __launch_bounds__(INTERP_THREADS) void k_interp_diag(const double* w, int64_t N, const double* table, double* q) {
  __shared__ double t[INTERP_TABLE];
  constexpr int total = D == 1 ? 7 : D == 2 ? 49 : 343;
  for (int e = threadIdx.x; e < total; e += INTERP_THREADS) t[e] = table[e];
  __syncthreads();
  for (int64_t k = (int64_t)blockIdx.x * INTERP_THREADS + threadIdx.x; k < N; k += (int64_t)gridDim.x * INTERP_THREADS) {
    double w0[4], w1[4], w2[4], a0[4], a1[4] = {1.0, 0.0, 0.0, 0.0}, a2[4] = {1.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      w0[s] = w[(int64_t)s * N + k];
      w1[s] = D > 1 ? w[(int64_t)(4 + s) * N + k] : 0.0;
      w2[s] = D > 2 ? w[(int64_t)(8 + s) * N + k] : 0.0;
    }
    interp_autocorr(w0, a0);
    if (D > 1) interp_autocorr(w1, a1);
    if (D > 2) interp_autocorr(w2, a2);
    double acc = 0.0;
    // the o2 loop stays a loop (a2 picked by selects, no indexed register array): unrolled, the 343 terms spill
#pragma unroll 1
    for (int o2 = (D > 2 ? -3 : 0); o2 <= (D > 2 ? 3 : 0); ++o2) {
      const int m2 = abs(o2);
      const double a2o = m2 == 0 ? a2[0] : m2 == 1 ? a2[1] : m2 == 2 ? a2[2] : a2[3];
#pragma unroll
      for (int o1 = (D > 1 ? -3 : 0); o1 <= (D > 1 ? 3 : 0); ++o1) {
#pragma unroll
        for (int o0 = -3; o0 <= 3; ++o0) {
          const double a = D > 2 ? (a2o * a1[abs(o1)]) * a0[abs(o0)] : D > 1 ? a1[abs(o1)] * a0[abs(o0)] : a0[abs(o0)];
          acc = fma(a, t[(o0 + 3) + 7 * ((D > 1 ? o1 + 3 : 0) + 7 * (D > 2 ? o2 + 3 : 0))], acc);
        }
      }
    }
    q[k] = acc;
  }
}

// ------------------------------------------------------------------ state
static const char* interp_grid_error(int code) {
  switch (code) {
    case INTERP_BAD_D: return "a grid has d = 1, 2 or 3 axes";
    case INTERP_BAD_N: return "an axis has 4 .. 2^23 nodes";
    case INTERP_BAD_H: return "the spacing must be positive and finite";
    case INTERP_BAD_ORIGIN: return "the origin must be finite";
    default: return "the grid has more than 2^40 nodes";
  }
}

// checks, weights and bins on the host (hfmi_interp_plan.h); everything the callers below share
struct interp_host {
  interp_grid g;
  std::vector<int64_t> base, cell, cell_start, perm;
  std::vector<double> w;
};
static int interp_host_make(const char* who, int d, const int64_t* n, const double* h, const double* origin, const double* points, int64_t N,
                            bool bins, interp_host* H) {
  if (!n || !h || !origin || !points) HFMI_FAIL(HFMI_ERR_INVALID, "%s: null argument", who);
  int axis = 0;
  const int gs = interp_grid_check(d, n, h, origin, &H->g, &axis);
  if (gs != INTERP_OK) HFMI_FAIL(HFMI_ERR_INVALID, "%s: %s (d = %d, axis %d)", who, interp_grid_error(gs), d, axis);
  if (N < 1) HFMI_FAIL(HFMI_ERR_INVALID, "%s: needs at least one point (N = %lld)", who, (long long)N);
  try {
    H->base.resize((size_t)N);
    H->cell.resize((size_t)N);
    H->w.resize((size_t)N * d * 4);
    if (bins) {
      H->cell_start.resize((size_t)H->g.ncells + 1);
      H->perm.resize((size_t)N);
    }
  } catch (const std::bad_alloc&) {
    HFMI_FAIL(HFMI_ERR_INVALID, "%s: out of host memory", who);
  }
  int64_t bad = 0;
  if (interp_weights(H->g, points, N, H->base.data(), H->w.data(), H->cell.data(), &bad, &axis) != INTERP_OK)
    HFMI_FAIL(HFMI_ERR_INVALID, "%s: point %lld is not finite or lies outside nodes 1 .. n - 2 = %lld of axis %d (coordinate %.17g, origin %.17g, spacing %.17g)",
              who, (long long)bad, (long long)H->g.n[axis] - 2, axis, points[(size_t)bad * d + axis], H->g.o[axis], H->g.h[axis]);
  if (bins) interp_bin(H->cell.data(), N, H->g.ncells, H->cell_start.data(), H->perm.data());
  return HFMI_OK;
}

extern "C" int hfmi_grid_interp_weights(int d, const int64_t* n, const double* h, const double* origin, const double* host_points, int64_t N,
                                        int64_t* base, double* w, int64_t* cell_start, int64_t* perm) {
  if (!base || !w) HFMI_FAIL(HFMI_ERR_INVALID, "grid_interp_weights: null argument");
  interp_host H;
  HFMI_TRY(interp_host_make("grid_interp_weights", d, n, h, origin, host_points, N, cell_start || perm, &H));
  std::copy(H.base.begin(), H.base.end(), base);
  std::copy(H.w.begin(), H.w.end(), w);
  if (cell_start) std::copy(H.cell_start.begin(), H.cell_start.end(), cell_start);
  if (perm) std::copy(H.perm.begin(), H.perm.end(), perm);
  return HFMI_OK;
}

template <class T>
static int interp_upload(dev_buf<T>* out, const std::vector<T>& host) {
  OWN_TRY(out->alloc(host.size()));
  HIP_TRY(hipMemcpy(out->get(), host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return HFMI_OK;
}

static int interp_state_make(hfmi_ctx* ctx, const char* who, int d, const int64_t* n, const double* h, const double* origin, const double* points,
                             int64_t N, std::unique_ptr<interp_state, void (*)(interp_state*)>& st) {
  interp_host H;
  HFMI_TRY(interp_host_make(who, d, n, h, origin, points, N, true, &H));
  st.reset(new (std::nothrow) interp_state());
  if (!st) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  st->g = H.g;
  st->N = N;
  // binned order on the device
  std::vector<int64_t> base((size_t)N);
  std::vector<double> w((size_t)N * d * 4);
  for (int64_t k = 0; k < N; ++k) {
    const int64_t i = H.perm[(size_t)k];
    base[(size_t)k] = H.base[(size_t)i];
    for (int a = 0; a < d; ++a)
      for (int s = 0; s < 4; ++s) w[(size_t)(4 * a + s) * N + k] = H.w[((size_t)i * d + a) * 4 + s];
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(interp_upload(&st->base, base));
  HFMI_TRY(interp_upload(&st->perm, H.perm));
  HFMI_TRY(interp_upload(&st->cell_start, H.cell_start));
  HFMI_TRY(interp_upload(&st->w, w));
  return HFMI_OK;
}

static interp_args interp_base_args(const interp_state* st) {
  interp_args A{};
  A.base = st->base, A.perm = st->perm, A.cell_start = st->cell_start, A.w = st->w;
  A.N = st->N;
  A.n0 = st->g.n[0], A.n1 = st->g.n[1], A.n2 = st->g.n[2];
  A.nc0 = st->g.nc[0], A.nc1 = st->g.nc[1], A.nc2 = st->g.nc[2];
  A.nnodes = st->g.nnodes;
  return A;
}

template <int EPI>
static int interp_launch_gather(hfmi_ctx* ctx, const interp_state* st, interp_args A) {
  const interp_launch s = interp_launch_shape(st->N, A.ncols, 1, ctx->num_cus);
  const dim3 grid(s.gx, s.gy), block(INTERP_THREADS);
  if (st->g.d == 1) hipLaunchKernelGGL((k_interp_gather<1, EPI>), grid, block, 0, ctx->stream, A);
  else if (st->g.d == 2) hipLaunchKernelGGL((k_interp_gather<2, EPI>), grid, block, 0, ctx->stream, A);
  else hipLaunchKernelGGL((k_interp_gather<3, EPI>), grid, block, 0, ctx->stream, A);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// Y (+)= W G (+ epilogue): G has nnodes rows, Y (and X) N rows
static int interp_gather(hfmi_ctx* ctx, const interp_state* st, const double* G, int64_t ldg, double* Y, int64_t ldy, int ncols, int accumulate,
                         int epi = EPI_NONE, const double* diag = nullptr, const double* X = nullptr, int64_t ldx = 0, uint64_t key = 0,
                         int64_t first = 0) {
  interp_args A = interp_base_args(st);
  A.in = G, A.ldin = ldg, A.out = Y, A.ldout = ldy, A.ncols = ncols, A.accumulate = accumulate;
  A.diag = diag, A.X = X, A.ldx = ldx, A.k0 = (uint32_t)key, A.k1 = (uint32_t)(key >> 32), A.first = first;
  if (epi == EPI_DIAG) return interp_launch_gather<EPI_DIAG>(ctx, st, A);
  if (epi == EPI_NOISE) return interp_launch_gather<EPI_NOISE>(ctx, st, A);
  return interp_launch_gather<EPI_NONE>(ctx, st, A);
}
// G (+)= W^T X
static int interp_spread(hfmi_ctx* ctx, const interp_state* st, const double* X, int64_t ldx, double* G, int64_t ldg, int ncols, int accumulate) {
  interp_args A = interp_base_args(st);
  A.in = X, A.ldin = ldx, A.out = G, A.ldout = ldg, A.ncols = ncols, A.accumulate = accumulate;
  const interp_launch s = interp_launch_shape(st->g.nnodes, ncols, INTERP_SPREAD_COLS, ctx->num_cus);
  const dim3 grid(s.gx, s.gy), block(INTERP_THREADS);
  if (st->g.d == 1) hipLaunchKernelGGL(k_interp_spread<1>, grid, block, 0, ctx->stream, A);
  else if (st->g.d == 2) hipLaunchKernelGGL(k_interp_spread<2>, grid, block, 0, ctx->stream, A);
  else hipLaunchKernelGGL(k_interp_spread<3>, grid, block, 0, ctx->stream, A);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// ------------------------------------------------------------------ operators
extern "C" int hfmi_op_grid_interp(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const double* origin, const double* host_points,
                                   int64_t N, int transpose, hfmi_op** out) {
  if (!ctx || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (transpose != 0 && transpose != 1) HFMI_FAIL(HFMI_ERR_INVALID, "grid_interp: transpose = %d is not 0 (W) or 1 (W^T)", transpose);
  std::unique_ptr<interp_state, void (*)(interp_state*)> st(nullptr, interp_destroy);
  HFMI_TRY(interp_state_make(ctx, "grid_interp", d, n, h, origin, host_points, N, st));
  std::unique_ptr<hfmi_op> op(new (std::nothrow) hfmi_op());
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->ctx = ctx;
  op->kind = OP_GRID_INTERP;
  op->ip = st.release();
  op->ip_transpose = transpose;
  *out = op.release();
  return HFMI_OK;
}

extern "C" int hfmi_op_kernel_cov_interp(hfmi_op* grid_cov_op, const double* origin, const double* host_points, int64_t N, double nugget,
                                         int diag_correction, hfmi_op** out) {
  if (!grid_cov_op || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (grid_cov_op->kind != OP_KERNEL_COV_GRID || !grid_cov_op->fc)
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_interp: the operator is not a kernel covariance on a grid (hfmi_op_kernel_cov_grid)");
  fftcov_grid_desc gd;
  fftcov_describe(grid_cov_op->fc, &gd);
  if (!gd.all_nodes) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_interp: the grid covariance must be over all nodes of its grid (no node map)");
  if (gd.nugget != 0.0) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_interp: the grid covariance must have nugget 0 (got %g): the nugget belongs to this operator", gd.nugget);
  if (!(nugget >= 0.0) || !isfinite(nugget)) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_interp: the nugget must be finite and not negative");
  if (diag_correction != 0 && diag_correction != 1) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_interp: diag_correction = %d is not 0 or 1", diag_correction);
  hfmi_ctx* ctx = grid_cov_op->ctx;
  std::unique_ptr<interp_state, void (*)(interp_state*)> st(nullptr, interp_destroy);
  HFMI_TRY(interp_state_make(ctx, "kernel_cov_interp", gd.d, gd.n, gd.h, origin, host_points, N, st));
  // q_i on the device from the kernel's table, then delta on the host (N doubles each way, once)
  dev_buf<double> table, q;
  OWN_TRY(table.alloc(INTERP_TABLE));
  OWN_TRY(q.alloc((size_t)N));
  int status = fftcov_offset_table(ctx, grid_cov_op->fc, table);
  if (status == HFMI_OK) {
    const interp_launch s = interp_launch_shape(N, 1, 1, ctx->num_cus);
    if (gd.d == 1) hipLaunchKernelGGL(k_interp_diag<1>, dim3(s.gx), dim3(INTERP_THREADS), 0, ctx->stream, st->w.get(), N, table.get(), q.get());
    else if (gd.d == 2) hipLaunchKernelGGL(k_interp_diag<2>, dim3(s.gx), dim3(INTERP_THREADS), 0, ctx->stream, st->w.get(), N, table.get(), q.get());
    else hipLaunchKernelGGL(k_interp_diag<3>, dim3(s.gx), dim3(INTERP_THREADS), 0, ctx->stream, st->w.get(), N, table.get(), q.get());
    if (hipGetLastError() != hipSuccess) status = HFMI_ERR_HIP;
  }
  std::vector<double> qb((size_t)N);
  hipError_t e = hipMemcpyAsync(qb.data(), q.get(), (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t done = hipStreamSynchronize(ctx->stream);   // whatever happened: `table` and `q` must not go while a kernel may use them
  HFMI_TRY(status);
  HIP_TRY(e);
  HIP_TRY(done);
  std::vector<int64_t> perm((size_t)N);
  HIP_TRY(hipMemcpy(perm.data(), st->perm.get(), (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost));
  const double sigma2 = gd.sigma * gd.sigma;
  st->host_q.resize((size_t)N);
  st->host_delta.resize((size_t)N);
  std::vector<double> db((size_t)N), sb((size_t)N);
  st->diag_min = INFINITY, st->diag_max = -INFINITY;
  for (int64_t k = 0; k < N; ++k) {
    const double defect = sigma2 - qb[(size_t)k];
    st->diag_min = std::min(st->diag_min, defect), st->diag_max = std::max(st->diag_max, defect);
    if (defect < 0.0) ++st->n_clipped;
    const double dl = diag_correction ? nugget + std::max(defect, 0.0) : nugget;
    db[(size_t)k] = dl, sb[(size_t)k] = sqrt(dl);
    st->host_q[(size_t)perm[(size_t)k]] = qb[(size_t)k];
    st->host_delta[(size_t)perm[(size_t)k]] = dl;
  }
  HFMI_TRY(interp_upload(&st->delta, db));
  HFMI_TRY(interp_upload(&st->sdelta, sb));
  st->work_ld = round_up(st->g.nnodes, 32);
  std::unique_ptr<hfmi_op> op(new (std::nothrow) hfmi_op());
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->ctx = ctx;
  op->kind = OP_KERNEL_COV_INTERP;
  op->ip = st.release();
  op->ip_grid = grid_cov_op;
  *out = op.release();
  return HFMI_OK;
}

static int interp_cov_op(const hfmi_op* op, const char* who) {
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "%s: null operator", who);
  if (op->kind != OP_KERNEL_COV_INTERP || !op->ip) HFMI_FAIL(HFMI_ERR_INVALID, "%s: the operator is not one of hfmi_op_kernel_cov_interp", who);
  return HFMI_OK;
}
extern "C" int hfmi_op_kernel_cov_interp_info(const hfmi_op* op, double* diag_min, double* diag_max, int64_t* n_diag_clipped) {
  HFMI_TRY(interp_cov_op(op, "kernel_cov_interp_info"));
  if (diag_min) *diag_min = op->ip->diag_min;
  if (diag_max) *diag_max = op->ip->diag_max;
  if (n_diag_clipped) *n_diag_clipped = op->ip->n_clipped;
  return HFMI_OK;
}
extern "C" int hfmi_op_kernel_cov_interp_diag(const hfmi_op* op, double* host_q, double* host_delta) {
  HFMI_TRY(interp_cov_op(op, "kernel_cov_interp_diag"));
  if (host_q) std::copy(op->ip->host_q.begin(), op->ip->host_q.end(), host_q);
  if (host_delta) std::copy(op->ip->host_delta.begin(), op->ip->host_delta.end(), host_delta);
  return HFMI_OK;
}

// the internal block holds `cols` columns
static int interp_fit_work(hfmi_ctx* ctx, interp_state* st, int cols) {
  OWN_TRY(grow(st->work, (size_t)st->work_ld * cols, [&] { return (int)hipStreamSynchronize(ctx->stream); }));
  return HFMI_OK;
}

int interp_apply(hfmi_op* op, const hfmi_block* X, hfmi_block* Y, int accumulate) {
  hfmi_ctx* ctx = op->ctx;
  interp_state* st = op->ip;
  const int k = X->nvec;
  if (op->kind == OP_GRID_INTERP) {
    const int64_t nin = op->ip_transpose ? st->N : st->g.nnodes, nout = op->ip_transpose ? st->g.nnodes : st->N;
    if (X->N != nin || Y->N != nout)
      HFMI_FAIL(HFMI_ERR_INVALID, "grid_interp: %s maps vectors of length %lld to length %lld, got %lld -> %lld", op->ip_transpose ? "W^T" : "W",
                (long long)nin, (long long)nout, (long long)X->N, (long long)Y->N);
    if (k < 1) return HFMI_OK;
    if (op->ip_transpose) return interp_spread(ctx, st, X->p, X->ld, Y->p, Y->ld, k, accumulate);
    return interp_gather(ctx, st, X->p, X->ld, Y->p, Y->ld, k, accumulate);
  }
  if (X->N != st->N || Y->N != st->N)
    HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld -> %lld", (long long)st->N, (long long)X->N, (long long)Y->N);
  if (k < 1) return HFMI_OK;
  // K X chunk by chunk of an even number of columns: spread into the work block, the grid apply IN PLACE (its first pass has read
  // every node of a chunk into the padded array before its last pass stores one), gather with delta . X fused
  const int kc = interp_chunk_cols(st->work_ld, k, fftcov_pairs_knob());
  HFMI_TRY(interp_fit_work(ctx, st, kc));
  double* G = st->work;
  for (int c0 = 0; c0 < k; c0 += kc) {
    const int nc = std::min(kc, k - c0);
    const double* x = X->p + (int64_t)c0 * X->ld;
    HFMI_TRY(interp_spread(ctx, st, x, X->ld, G, st->work_ld, nc, 0));
    HFMI_TRY(fftcov_apply(ctx, op->ip_grid->fc, G, st->work_ld, G, st->work_ld, nc, 0));
    HFMI_TRY(interp_gather(ctx, st, G, st->work_ld, Y->p + (int64_t)c0 * Y->ld, Y->ld, nc, accumulate, EPI_DIAG, st->delta, x, X->ld));
  }
  return HFMI_OK;
}

extern "C" int hfmi_interp_sampler_draw(hfmi_op* op, hfmi_grid_sampler* grid_sampler, const hfmi_block* Y, uint64_t seed, int64_t first_sample,
                                        int accumulate) {
  HFMI_TRY(interp_cov_op(op, "interp_sampler_draw"));
  if (!grid_sampler || !Y) HFMI_FAIL(HFMI_ERR_INVALID, "interp_sampler_draw: null argument");
  hfmi_ctx* ctx = op->ctx;
  interp_state* st = op->ip;
  if (grid_sampler_ctx(grid_sampler) != ctx || !fftcov_same_covariance(grid_sampler_state(grid_sampler), op->ip_grid->fc))
    HFMI_FAIL(HFMI_ERR_INVALID, "interp_sampler_draw: the sampler was not made from this operator's grid covariance");
  if (Y->N != st->N) HFMI_FAIL(HFMI_ERR_INVALID, "interp_sampler_draw: draws have length %lld, the block's vectors %lld", (long long)st->N, (long long)Y->N);
  if (first_sample < 0 || (first_sample & 1))
    HFMI_FAIL(HFMI_ERR_INVALID, "interp_sampler_draw: first_sample = %lld must be even and not negative (draws 2 p and 2 p + 1 are one transform)",
              (long long)first_sample);
  const int k = Y->nvec;
  if (first_sample + k > ((int64_t)1 << 32))
    HFMI_FAIL(HFMI_ERR_INVALID, "interp_sampler_draw: a seed has 2^32 draws, first_sample = %lld with %d columns goes past them", (long long)first_sample, k);
  if (k < 1) return HFMI_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int kc = interp_chunk_cols(st->work_ld, k, fftcov_pairs_knob());
  HFMI_TRY(interp_fit_work(ctx, st, kc));
  const uint64_t key = seed ^ 0x9E3779B97F4A7C15ull;     // not the grid noise's key: eta and z are independent
  for (int c0 = 0; c0 < k; c0 += kc) {
    const int nc = std::min(kc, k - c0);
    const hfmi_block Z{ctx, st->work.get(), st->g.nnodes, nc, st->work_ld, false};
    HFMI_TRY(hfmi_grid_sampler_draw(grid_sampler, &Z, seed, first_sample + c0, 0));
    HFMI_TRY(interp_gather(ctx, st, Z.p, Z.ld, Y->p + (int64_t)c0 * Y->ld, Y->ld, nc, accumulate != 0, EPI_NOISE, st->sdelta, nullptr, 0, key,
                           first_sample + c0));
  }
  return HFMI_OK;
}

// ------------------------------------------------------------------ the factor K = F F^T (hfmi_op_interp_factor)
// F = [ W S | diag(sqrt(delta)) ], N x (Ptot + N), S the factor of the sampler's embedding (hfmi_op_grid_factor) and Ptot = prod P_c.
// NOISE LAYOUT (hfmi_interp_plan.h): rows 0 .. Ptot - 1 the padded-grid noise in the grid factor's natural order, rows Ptot .. Ptot + N - 1
// one entry per point in POINT order.  Both directions go through the interpolated operator's work block chunk by chunk of an even
// number of columns, so the pairs the grid factor forms are those of one call and no "fftcov_pairs" changes a bit.
extern "C" int hfmi_op_interp_factor(hfmi_op* cov, hfmi_grid_sampler* grid_sampler, int transpose, hfmi_op** out) {
  HFMI_TRY(interp_cov_op(cov, "interp_factor"));
  if (!grid_sampler || !out) HFMI_FAIL(HFMI_ERR_INVALID, "interp_factor: null argument");
  if (transpose != 0 && transpose != 1) HFMI_FAIL(HFMI_ERR_INVALID, "interp_factor: transpose = %d is not 0 (F) or 1 (F^T)", transpose);
  hfmi_ctx* ctx = cov->ctx;
  interp_state* st = cov->ip;
  if (grid_sampler_ctx(grid_sampler) != ctx || !fftcov_same_covariance(grid_sampler_state(grid_sampler), cov->ip_grid->fc))
    HFMI_FAIL(HFMI_ERR_INVALID, "interp_factor: the sampler was not made from this operator's grid covariance");
  HFMI_TRY(grid_sampler_root(grid_sampler, "interp_factor"));
  if (!st->sdelta_pt) {
    std::vector<double> sp((size_t)st->N);
    for (int64_t i = 0; i < st->N; ++i) sp[(size_t)i] = sqrt(st->host_delta[(size_t)i]);    // the bits of sdelta, in point order
    HFMI_TRY(interp_upload(&st->sdelta_pt, sp));
  }
  std::unique_ptr<hfmi_op> op(new (std::nothrow) hfmi_op());
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->ctx = ctx;
  op->kind = OP_INTERP_FACTOR;
  op->fac = grid_sampler_share(grid_sampler);
  op->fac_transpose = transpose;
  op->ip_grid = cov;
  *out = op.release();
  return HFMI_OK;
}

int interp_factor_apply(hfmi_op* op, const hfmi_block* X, hfmi_block* Y, int accumulate) {
  hfmi_ctx* ctx = op->ctx;
  interp_state* st = op->ip_grid->ip;
  fftcov_state* fs = op->fac.get();
  const int transpose = op->fac_transpose;
  const int64_t N = st->N, Ptot = fftcov_padded_len(fs);
  const int64_t nin = transpose ? N : Ptot + N, nout = transpose ? Ptot + N : N;
  if (X->N != nin || Y->N != nout)
    HFMI_FAIL(HFMI_ERR_INVALID, "interp_factor: %s maps vectors of length %lld to length %lld, got %lld -> %lld", transpose ? "F^T" : "F",
              (long long)nin, (long long)nout, (long long)X->N, (long long)Y->N);
  const int k = X->nvec;
  if (k < 1) return HFMI_OK;
  const int kc = interp_chunk_cols(st->work_ld, k, fftcov_pairs_knob());
  HFMI_TRY(interp_fit_work(ctx, st, kc));
  for (int c0 = 0; c0 < k; c0 += kc) {
    const int nc = std::min(kc, k - c0);
    double* x = X->p + (int64_t)c0 * X->ld;
    double* y = Y->p + (int64_t)c0 * Y->ld;
    hfmi_block G{ctx, st->work.get(), st->g.nnodes, nc, st->work_ld, false};
    if (!transpose) {
      // the grid factor from a VIEW of the first Ptot rows into the work block, then one gather with + sqrt(delta_i) Xi[Ptot + i] fused
      const hfmi_block top{ctx, x, Ptot, nc, X->ld, false};
      HFMI_TRY(fftcov_factor_apply(ctx, fs, 0, &top, &G, 0));
      HFMI_TRY(interp_gather(ctx, st, G.p, G.ld, y, Y->ld, nc, accumulate, EPI_DIAG, st->sdelta, x + Ptot, X->ld));
    } else {
      // spread into the work block, the transposed grid factor into a view of the first Ptot rows, the tail by its own kernel
      HFMI_TRY(interp_spread(ctx, st, x, X->ld, G.p, G.ld, nc, 0));
      hfmi_block top{ctx, y, Ptot, nc, Y->ld, false};
      HFMI_TRY(fftcov_factor_apply(ctx, fs, 1, &G, &top, accumulate));
      const interp_launch s = interp_launch_shape(N, nc, 1, ctx->num_cus);
      hipLaunchKernelGGL(k_interp_factor_tail, dim3(s.gx, s.gy), dim3(INTERP_THREADS), 0, ctx->stream, st->sdelta_pt.get(), N, x, X->ld, y + Ptot,
                         Y->ld, nc, accumulate);
      HIP_TRY(hipGetLastError());
    }
  }
  return HFMI_OK;
}
