// Kernel covariance on the nodes of a regular grid, applied by FFT (hfmi_op_kernel_cov_grid):  Y (+)= C W with the matrix of
// hfmi_op_kernel_cov, C_ij = sigma^2 phi(|x_i - x_j| / ell) + nugget delta_ij.  On a regular grid a stationary kernel gives a
// block-Toeplitz matrix with Toeplitz blocks; embedded in a circulant (P_c >= 2 n_c - 1 entries along axis c) it is diagonalised by
// the FFT, so C W = gather( IFFT( Lambda . FFT( scatter(W) ) ) ) exactly, up to rounding.  What is planned where, and the pass list,
// is in hfmi_fftcov_plan.h; this unit holds the kernels, the operator's state and the launcher.
//
// k_fftcov_pass: complex fp64 power-of-two transforms of `lpw` lines along one axis of the padded array, one workgroup, the lines in
// LDS.  A pass is  load (from the work buffer, or W's columns through the node map: the scatter)  ->  forward stages  ->  multiply by
// Lambda / P  ->  inverse stages  ->  store (to the work buffer, or into Y through the node map: the gather), every part optional.
// The forward transform is decimation in frequency, in place: natural order in, digit-reversed order out.  The inverse is decimation
// in time and takes that order.  Lambda is made by the forward passes and lives in the same order, so no pass permutes anything.
// Two radix-2 stages are done per trip through LDS (four entries per thread, a radix-4 step written as its two radix-2 stages); an odd
// log2 L adds one radix-2 stage.  Twiddles: exp(-2 pi i k / L) for k < L / 4 staged in LDS from the operator's table, the second
// quarter by w(k + L / 4) = -i w(k).
//
// Two real columns ride one transform, z = w_j + i w_{j+1}: Lambda is real, so the result is y_j + i y_{j+1}.  The pair index is the
// y coordinate of the launch grid; a chunk of pairs shares the launches.  Every entry of Y is written by exactly one thread and there
// are no atomics: two applies are bit-identical, and the pairs per chunk change nothing but the number of launches.
//
// LDS: lpw * (L + pad) entries of 16 bytes and the twiddles, dynamic; two tables of 256 line bases, static (4 KiB).  The plan keeps
// static + dynamic below the 160 KiB of a workgroup.  The bank layout (hfmi_fftcov_plan.h: pad) has not been measured.
#include <math.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "hfmi_kcov_eval.h"

struct fftcov_state {
  int d = 0;
  int64_t n[3] = {1, 1, 1};
  double h[3] = {1.0, 1.0, 1.0};
  int64_t N = 0;           // points of the operator
  int64_t nnodes = 0;      // prod n
  int family = 0;
  double sigma = 0.0, ell = 0.0, nugget = 0.0;
  dev_buf<int64_t> inv;    // nnodes entries: the point that is grid node g, or -1; empty: point g is node g
  dev_buf<double2> tw;     // exp(-2 pi i k / Pmax), k < max(Pmax / 4, 1)
  dev_buf<double> lambda;  // prod P_c doubles: FFT(first column) / prod P_c, in the order the forward passes leave
  dev_buf<double2> work;   // work_pairs() arrays of prod P_c entries
  fftcov_plan plan;        // the passes of an apply
  int work_pairs() const { return (int)(work.bytes() / (size_t)plan.pair_bytes); }
};

struct fftcov_pass_args {
  double2* buf;
  int64_t pair_stride;     // entries between the arrays of consecutive pairs
  const double2* tw;
  int tw_step;             // Pmax / L
  const double* lambda;
  int flags, L, logL, lpw, loglpw, ls, nload, nstore;
  int64_t stride;
  int logstride;
  int64_t nlines, oe0, os0, os1;
  const int64_t* inv;      // scatter / gather: node -> point
  int64_t n0;
  const double* W;
  int64_t ldw;
  double* Y;
  int64_t ldy;
  int ncols, col0, accumulate;
};

__device__ __forceinline__ double2 fc_add(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double2 fc_sub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ double2 fc_mul(double2 a, double2 b) { return double2{fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)}; }
// a * conj(b)
__device__ __forceinline__ double2 fc_mulc(double2 a, double2 b) { return double2{fma(a.x, b.x, a.y * b.y), fma(a.y, b.x, -a.x * b.y)}; }
// exp(-2 pi i k / L) for k < L / 2 from the quarter table (qm = max(L / 4, 1) entries)
__device__ __forceinline__ double2 fc_twiddle(const double2* ltw, int k, int qm) {
  const double2 t = ltw[k & (qm - 1)];
  return k >= qm ? double2{t.y, -t.x} : t;
}

__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_fftcov_pass(fftcov_pass_args A) {
  extern __shared__ double2 fc_lds[];
  __shared__ int64_t lbase[FFTCOV_MAX_LINES];    // first entry of the line in the pair's array, -1: no such line
  __shared__ int64_t gbase[FFTCOV_MAX_LINES];    // axis-0 lines: grid node of position 0
  const int tid = threadIdx.x, nt = blockDim.x;
  const int L = A.L, logL = A.logL, lpw = A.lpw, ls = A.ls;
  double2* x = fc_lds;
  double2* ltw = fc_lds + lpw * ls;
  const int qm = L / 4 > 1 ? L / 4 : 1;
  const int64_t line0 = (int64_t)blockIdx.x * lpw;
  const int pair = blockIdx.y;
  double2* buf = A.buf + (int64_t)pair * A.pair_stride;
  for (int j = tid; j < lpw; j += nt) {
    const int64_t line = line0 + j;
    int64_t b = -1, g = -1;
    if (line < A.nlines) {
      const int64_t inner = line & (A.stride - 1), o = line >> A.logstride;
      b = inner + (o % A.oe0) * A.os0 + (o / A.oe0) * A.os1;
      g = o * A.n0;
    }
    lbase[j] = b;
    gbase[j] = g;
  }
  for (int i = tid; i < qm; i += nt) ltw[i] = A.tw[(int64_t)i * A.tw_step];
  __syncthreads();

  // entry e of the workgroup's lines -> (line j, position p): along the line on the contiguous axis, across adjacent lines on a strided one
  const int total = lpw << logL;
  const bool strided = A.stride > 1;
  const int c0 = A.col0 + 2 * pair;
  const bool has1 = c0 + 1 < A.ncols;
  for (int e = tid; e < total; e += nt) {
    const int j = strided ? (e & (lpw - 1)) : (e >> logL);
    const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
    double2 v = double2{0.0, 0.0};
    const int64_t b = lbase[j];
    if (b >= 0 && p < A.nload) {
      if (A.flags & FFTCOV_SCATTER) {
        const int64_t g = gbase[j] + p;
        const int64_t pt = A.inv ? A.inv[g] : g;
        if (pt >= 0) {
          v.x = A.W[(int64_t)c0 * A.ldw + pt];
          if (has1) v.y = A.W[(int64_t)(c0 + 1) * A.ldw + pt];
        }
      } else {
        v = buf[b + (int64_t)p * A.stride];
      }
    }
    x[j * ls + p] = v;
  }
  __syncthreads();

  if (A.flags & FFTCOV_FWD) {
    int lh = logL - 1;
    if (logL & 1) {          // one radix-2 stage, h = L / 2
      const int h = 1 << lh, items = total >> 1;
      for (int idx = tid; idx < items; idx += nt) {
        const int j = idx >> (logL - 1), off = idx & (h - 1);
        double2* xi = x + j * ls + off;
        const double2 a = xi[0], b = xi[h];
        xi[0] = fc_add(a, b);
        xi[h] = fc_mul(fc_sub(a, b), fc_twiddle(ltw, off, qm));
      }
      --lh;
      __syncthreads();
    }
    for (; lh >= 1; lh -= 2) {   // stages h = 2^lh and q = h / 2
      const int lq = lh - 1, q = 1 << lq, items = total >> 2;
      for (int idx = tid; idx < items; idx += nt) {
        const int j = idx >> (logL - 2), r = idx & ((L >> 2) - 1);
        const int off = r & (q - 1);
        double2* xi = x + j * ls + ((r >> lq) << (lq + 2)) + off;
        const int k1 = off << (logL - 2 - lq);
        const double2 w1 = ltw[k1], w1q = double2{w1.y, -w1.x}, w2 = fc_twiddle(ltw, 2 * k1, qm);
        const double2 x0 = xi[0], x1 = xi[q], x2 = xi[2 * q], x3 = xi[3 * q];
        const double2 a = fc_add(x0, x2), b = fc_mul(fc_sub(x0, x2), w1);
        const double2 c = fc_add(x1, x3), d = fc_mul(fc_sub(x1, x3), w1q);
        xi[0] = fc_add(a, c);
        xi[q] = fc_mul(fc_sub(a, c), w2);
        xi[2 * q] = fc_add(b, d);
        xi[3 * q] = fc_mul(fc_sub(b, d), w2);
      }
      __syncthreads();
    }
  }

  if (A.flags & FFTCOV_MUL) {
    for (int e = tid; e < total; e += nt) {
      const int j = strided ? (e & (lpw - 1)) : (e >> logL);
      const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
      const int64_t b = lbase[j];
      if (b >= 0) {
        const double lam = A.lambda[b + (int64_t)p * A.stride];
        double2 v = x[j * ls + p];
        v.x *= lam;
        v.y *= lam;
        x[j * ls + p] = v;
      }
    }
    __syncthreads();
  }

  if (A.flags & FFTCOV_INV) {
    for (int lq = 0; lq + 1 < logL; lq += 2) {   // stages q = 2^lq and 2 q
      const int q = 1 << lq, items = total >> 2;
      for (int idx = tid; idx < items; idx += nt) {
        const int j = idx >> (logL - 2), r = idx & ((L >> 2) - 1);
        const int off = r & (q - 1);
        double2* xi = x + j * ls + ((r >> lq) << (lq + 2)) + off;
        const int k1 = off << (logL - 2 - lq);
        const double2 w1 = ltw[k1], w1q = double2{w1.y, -w1.x}, w2 = fc_twiddle(ltw, 2 * k1, qm);
        const double2 y0 = xi[0], y1 = xi[q], y2 = xi[2 * q], y3 = xi[3 * q];
        double2 t = fc_mulc(y1, w2);
        const double2 a = fc_add(y0, t), c = fc_sub(y0, t);
        t = fc_mulc(y3, w2);
        const double2 b = fc_add(y2, t), d = fc_sub(y2, t);
        t = fc_mulc(b, w1);
        xi[0] = fc_add(a, t);
        xi[2 * q] = fc_sub(a, t);
        t = fc_mulc(d, w1q);
        xi[q] = fc_add(c, t);
        xi[3 * q] = fc_sub(c, t);
      }
      __syncthreads();
    }
    if (logL & 1) {          // the radix-2 stage h = L / 2
      const int h = 1 << (logL - 1), items = total >> 1;
      for (int idx = tid; idx < items; idx += nt) {
        const int j = idx >> (logL - 1), off = idx & (h - 1);
        double2* xi = x + j * ls + off;
        const double2 a = xi[0], t = fc_mulc(xi[h], fc_twiddle(ltw, off, qm));
        xi[0] = fc_add(a, t);
        xi[h] = fc_sub(a, t);
      }
      __syncthreads();
    }
  }

  for (int e = tid; e < total; e += nt) {
    const int j = strided ? (e & (lpw - 1)) : (e >> logL);
    const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
    const int64_t b = lbase[j];
    if (b >= 0 && p < A.nstore) {
      const double2 v = x[j * ls + p];
      if (A.flags & FFTCOV_GATHER) {
        const int64_t g = gbase[j] + p;
        const int64_t pt = A.inv ? A.inv[g] : g;
        if (pt >= 0) {
          double* y0 = A.Y + (int64_t)c0 * A.ldy + pt;
          *y0 = A.accumulate ? *y0 + v.x : v.x;
          if (has1) {
            double* y1 = y0 + A.ldy;
            *y1 = A.accumulate ? *y1 + v.y : v.y;
          }
        }
      } else {
        buf[b + (int64_t)p * A.stride] = v;
      }
    }
  }
}

// the circulant's first column: entry (j0, j1, j2) is the kernel at the offsets min(j_c, P_c - j_c) h_c, the nugget on entry 0
__global__ __launch_bounds__(256) void k_fftcov_column(kcov_params K, double2* buf, int64_t total, int l0, int l1, int P0, int P1, int P2,
                                                       double h0, double h1, double h2) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j0 = (int)(e & (P0 - 1)), j1 = (int)((e >> l0) & (P1 - 1)), j2 = (int)(e >> (l0 + l1));
    const double dx = (double)min(j0, P0 - j0) * h0;
    double r2 = dx * dx;
    if (K.d > 1) {
      const double dy = (double)min(j1, P1 - j1) * h1;
      r2 = fma(dy, dy, r2);
    }
    if (K.d > 2) {
      const double dz = (double)min(j2, P2 - j2) * h2;
      r2 = fma(dz, dz, r2);
    }
    buf[e] = double2{kcov_entry(K, r2, e == 0), 0.0};
  }
}
// Lambda / P: the transform of a real symmetric column is real, what the imaginary parts hold is rounding
__global__ __launch_bounds__(256) void k_fftcov_spectrum(const double2* buf, double* lambda, int64_t total, double scale) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    lambda[e] = buf[e].x * scale;
}

static int fftcov_launch_pass(hfmi_ctx* ctx, const fftcov_state* st, const fftcov_plan& p, const fftcov_pass& q, int pairs, int col0,
                              const double* W, int64_t ldw, double* Y, int64_t ldy, int ncols, int accumulate) {
  fftcov_pass_args A;
  A.buf = st->work;
  A.pair_stride = p.Ptot;
  A.tw = st->tw;
  A.tw_step = p.Pmax / q.L;
  A.lambda = st->lambda;
  A.flags = q.flags, A.L = q.L, A.logL = q.logL, A.lpw = q.lpw, A.loglpw = q.loglpw, A.ls = q.ls, A.nload = q.nload, A.nstore = q.nstore;
  A.stride = q.stride;
  A.logstride = fftcov_log2(q.stride);
  A.nlines = q.nlines, A.oe0 = q.oe0, A.os0 = q.os0, A.os1 = q.os1;
  A.inv = st->inv;
  A.n0 = st->n[0];
  A.W = W, A.ldw = ldw, A.Y = Y, A.ldy = ldy, A.ncols = ncols, A.col0 = col0, A.accumulate = accumulate;
  if (q.lds + FFTCOV_STATIC_LDS > FFTCOV_LDS_BYTES || q.lpw > FFTCOV_MAX_LINES || q.grid_x > 0x7fffffff || pairs > 65535)
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: a pass of %d lines x %d entries (%d bytes of LDS, grid %lld x %d) cannot be launched", q.lpw,
              q.L, q.lds, (long long)q.grid_x, pairs);
  hipLaunchKernelGGL(k_fftcov_pass, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

int64_t fftcov_points(const fftcov_state* st) { return st->N; }

void fftcov_destroy(fftcov_state* st) { delete st; }

static int fftcov_create_device(hfmi_ctx* ctx, fftcov_state* st, const int64_t* host_inv) {
  const fftcov_plan& p = st->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipFuncSetAttribute((const void*)k_fftcov_pass, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - FFTCOV_STATIC_LDS));
  // the work buffer of one pair and Lambda: what decides whether the padded grid fits at all
  hipError_t e = (hipError_t)st->work.alloc((size_t)p.pair_bytes / sizeof(double2));
  if (e == hipSuccess) e = (hipError_t)st->lambda.alloc((size_t)p.Ptot);
  if (e != hipSuccess) {
    HFMI_FAIL(HFMI_ERR_HIP, "kernel_cov_grid: the padded grid %d x %d x %d needs %lld bytes of work buffer per pair of vectors and %lld bytes of spectrum: %s",
              p.P[0], p.P[1], p.P[2], (long long)p.pair_bytes, (long long)(p.Ptot * 8), hipGetErrorString(e));
  }
  if (host_inv) {
    OWN_TRY(st->inv.alloc((size_t)st->nnodes));
    HIP_TRY(hipMemcpy(st->inv, host_inv, (size_t)st->nnodes * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  // twiddles: long double on the host, rounded once
  std::vector<double2> tw((size_t)p.twiddles);
  const long double two_pi = 2.0L * acosl(-1.0L);
  for (int k = 0; k < p.twiddles; ++k) {
    const long double a = -two_pi * (long double)k / (long double)p.Pmax;
    tw[k] = double2{(double)cosl(a), (double)sinl(a)};
  }
  OWN_TRY(st->tw.alloc(tw.size()));
  HIP_TRY(hipMemcpy(st->tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
  // Lambda = FFT(first column) / P by the forward passes over the whole padded array
  kcov_params K;
  HFMI_TRY(kcov_params_init(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, st->nugget));   // no coordinates are read
  const int64_t blocks = std::min<int64_t>((p.Ptot + 255) / 256, (int64_t)ctx->num_cus * 8);
  hipLaunchKernelGGL(k_fftcov_column, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, K, st->work, p.Ptot, fftcov_log2(p.P[0]),
                     fftcov_log2(p.P[1]), p.P[0], p.P[1], p.P[2], st->h[0], st->h[1], st->h[2]);
  HIP_TRY(hipGetLastError());
  const fftcov_plan sp = fftcov_plan_passes(st->d, st->n, true);
  for (int i = 0; i < sp.npasses; ++i) HFMI_TRY(fftcov_launch_pass(ctx, st, sp, sp.pass[i], 1, 0, nullptr, 0, nullptr, 0, 0, 0));
  hipLaunchKernelGGL(k_fftcov_spectrum, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, st->work, st->lambda, p.Ptot, 1.0 / (double)p.Ptot);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return HFMI_OK;
}

int fftcov_create(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N, int family, double sigma,
                  double ell, double nugget, fftcov_state** out) {
  int64_t nnodes = 1;
  for (int c = 0; c < d; ++c) {
    if (n[c] < 1 || n[c] > FFTCOV_MAXN)
      HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: n[%d] = %lld is not in 1 .. %d", c, (long long)n[c], FFTCOV_MAXN);
    if (!(h[c] > 0.0) || !isfinite(h[c])) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: spacing h[%d] must be positive and finite", c);
    nnodes *= n[c];
  }
  if (N > nnodes || (!host_nodes && N != nnodes))
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: N = %lld points on a grid of %lld nodes%s", (long long)N, (long long)nnodes,
              host_nodes ? "" : " (no node map: N must be the number of nodes)");
  std::vector<int64_t> inv;
  if (host_nodes) {
    inv.assign((size_t)nnodes, -1);
    for (int64_t i = 0; i < N; ++i) {
      const int64_t g = host_nodes[i];
      if (g < 0 || g >= nnodes) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: node %lld of point %lld is not in 0 .. %lld", (long long)g, (long long)i, (long long)nnodes - 1);
      if (inv[g] >= 0) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: points %lld and %lld are the same node %lld", (long long)inv[g], (long long)i, (long long)g);
      inv[g] = i;
    }
  }
  std::unique_ptr<fftcov_state, void (*)(fftcov_state*)> st(new (std::nothrow) fftcov_state(), fftcov_destroy);
  if (!st) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  st->d = d;
  for (int c = 0; c < 3; ++c) st->n[c] = c < d ? n[c] : 1, st->h[c] = c < d ? h[c] : 1.0;
  st->N = N;
  st->nnodes = nnodes;
  st->family = family, st->sigma = sigma, st->ell = ell, st->nugget = nugget;
  st->plan = fftcov_plan_passes(d, st->n, false);
  const int s = fftcov_create_device(ctx, st.get(), host_nodes ? inv.data() : nullptr);
  if (s != HFMI_OK) {
    (void)hipStreamSynchronize(ctx->stream);      // before the buffers go: the kernels queued so far use them
    return s;
  }
  *out = st.release();
  return HFMI_OK;
}

int fftcov_apply(hfmi_ctx* ctx, fftcov_state* st, const double* W, int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate) {
  if (nvec < 1) return HFMI_OK;
  fftcov_plan p = st->plan;
  fftcov_plan_chunks(p, nvec, 0, fftcov_pairs_knob());
  if (p.chunk_pairs > st->work_pairs()) {
    // grow the work buffer to the chunk: the larger one first, so that when the device has no room for it the apply runs in the
    // chunks the buffer at hand holds (same results)
    dev_buf<double2> bigger;
    if (bigger.alloc((size_t)p.chunk_pairs * ((size_t)p.pair_bytes / sizeof(double2))) == 0) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      st->work = std::move(bigger);
    } else {
      fftcov_plan_chunks(p, nvec, 0, st->work_pairs());
    }
  }
  for (int c = 0; c < p.nchunks; ++c) {
    const int pair0 = c * p.chunk_pairs, pairs = std::min(p.chunk_pairs, p.pairs - pair0);
    for (int i = 0; i < p.npasses; ++i) HFMI_TRY(fftcov_launch_pass(ctx, st, p, p.pass[i], pairs, 2 * pair0, W, ldw, Y, ldy, nvec, accumulate));
  }
  return HFMI_OK;
}
