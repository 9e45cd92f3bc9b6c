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
// quarter by w(k + L / 4) = -i w(k).  The stages, the twiddle lookup and the host loop that makes the table are in hfmi_fft_lds.h, shared
// with the box priors (hfmi_boxcov.hip); this unit's pass body holds the ends and calls them.
//
// Two real columns ride one transform, z = w_j + i w_{j+1}: Lambda is real, so the result is y_j + i y_{j+1}.  The pair index is the
// y coordinate of the launch grid; a chunk of pairs shares the launches.  Every entry of Y is written by exactly one thread and there
// are no atomics: two applies are bit-identical, and the pairs per chunk change nothing but the number of launches.
//
// LDS: lpw * (L + pad) entries of 16 bytes and the twiddles, dynamic; two tables of 256 line bases, static (4 KiB).  The plan keeps
// static + dynamic below the 160 KiB of a workgroup.  The bank layout (hfmi_fftcov_plan.h: pad) has not been measured.
//
// The same passes draw m ~ N(0, C) (hfmi_grid_sampler_*, the second half of this unit): k_fftcov_draw is the pass whose load is
// generated -- sqrt(max(Lambda / P, 0)) times complex Philox / Box-Muller noise, hfmi_randn_math.h -- followed by the inverse passes of an
// apply, on an embedding of the sampler's own.  Both kernels are one body (fftcov_pass_body<GEN>); the apply's instance has the
// registers (44 VGPRs) and the LDS it had before the draw existed, the draw's takes 49 VGPRs and no scratch.
//
// And they apply the factor C = S S^T of a sampler's embedding (hfmi_op_grid_factor, the last part of this unit; the rules are in
// hfmi_fftcov_plan.h): S = Rn Chat^(1/2) and S^T are the passes of an apply with the root table sqrt(max(Lambda / P, 0) / P) in place
// of Lambda / P and the block of padded vectors on one side.  fftcov_pass_body serves that as it stands: its scatter and gather with no
// node map, n0 = P_0 and all P_0 positions loaded / stored ARE the direct load and store of a block of length prod P_c, so every pass
// of a factor in 2 or 3 dimensions is a launch of k_fftcov_pass.  Only the single fused pass of d = 1 needs the node map on one side
// and none on the other; k_fftcov_factor (FAC) is the body with that choice read from the pass flags.  k_fftcov_root makes the table.
//
// The long route (hfmi_op_kernel_cov_grid_long and its samplers; rules: "split-line passes" in hfmi_fftcov_plan.h) splits an embedding
// axis longer than max_line into two sub-axes; a pass along a sub-axis is k_fftcov_split / k_fftcov_split_draw, the body with SPLIT: its
// own line map, the axis position p pm + sub sm as the limit of loads and stores, and the four-step twiddle fused into the store of a
// forward high pass or the load of an inverse one.  Passes along whole axes stay launches of the kernels above.
#include <math.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "hfmi_fft_lds.h"
#include "hfmi_kcov_eval.h"
#include "hfmi_randn_math.h"

struct fftcov_state {
  int d = 0;
  int64_t n[3] = {1, 1, 1};
  double h[3] = {1.0, 1.0, 1.0};
  int64_t N = 0;           // points of the operator
  int64_t nnodes = 0;      // prod n
  int family = 0;
  double sigma = 0.0, ell = 0.0, nugget = 0.0;
  bool has_metric = false; // r^2 = |L^T diag(h) o|^2 / ell^2 with the factor below (k_fftcov_column_signed); false: the even column
  double mL[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};   // lower Cholesky factor of the metric, row-major 3 x 3
  double nu = 0.0, nuca = 0.0;   // HFMI_KERNEL_MATERN: the smoothness and sqrt(2 nu); the table words below are this state's own copy
  dev_buf<double> nutab;
  dev_buf<int64_t> inv;    // nnodes entries: the point that is grid node g, or -1; empty: point g is node g
  dev_buf<double2> tw;     // exp(-2 pi i k / Pmax), k < max(Pmax / 4, 1)
  dev_buf<double> lambda;  // prod P_c doubles: FFT(first column) / prod P_c, in the order the forward passes leave
  dev_buf<double> root;    // a sampler's, made at its first factor: sqrt(max(lambda, 0) / prod P_c), the order of lambda
  dev_buf<double2> work;   // arrays of prod P_c entries, one per pair of a chunk (fft_fit_work)
  int growth = 0;          // the embedding's: 0 for an operator, a sampler may double every P_c up to three times (six: long route)
  fftcov_plan plan;        // the passes of an apply, or of a draw (a sampler's state); long route: the embedding only, no passes
  bool long_route = false; // hfmi_op_kernel_cov_grid_long and its samplers: the passes are lplan's
  int max_line = FFTCOV_LONG_MAX_LINE;
  fftcov_long_plan lplan;
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

// what the generated load of a draw's first pass adds (hfmi_fftcov_plan.h: the noise's element map).  A type of its own, so that the apply's
// kernel takes the argument block it always took.
struct fftcov_gen_args {
  uint32_t k0, k1;         // the seed
  int64_t pair0;           // pair index of blockIdx.y = 0 in the stream of draws
};

// storage entries e0 (even) and e0 + 1 of pair `gp`: sqrt(max(lambda, 0)) (z_a + i z_b), four normals of one Philox output
__device__ __forceinline__ void fc_coloured_noise(const fftcov_gen_args& G, uint32_t gp, int64_t e0, const double* lambda,
                                                  const hfmi_rng::normal_consts& kc, double2& v0, double2& v1) {
  const int64_t q = e0 >> 1;
  uint32_t r[4];
  double z[4];
  hfmi_rng::philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), gp, FFTCOV_GEN_STREAM, G.k0, G.k1, r);
  hfmi_rng::box_muller4(r, kc, z);
  const double s0 = sqrt(fmax(lambda[e0], 0.0)), s1 = sqrt(fmax(lambda[e0 + 1], 0.0));
  v0 = double2{s0 * z[0], s0 * z[1]};
  v1 = double2{s1 * z[2], s1 * z[3]};
}

// what a pass along a sub-axis of a split embedding axis adds (hfmi_fftcov_plan.h: split-line passes).  A type of its own, so that the
// apply's kernel takes the argument block it always took.
struct fftcov_split_args {
  int64_t inner, esub, sub_stride;   // a line number is  inner-part + inner (sub + esub o)
  int loginner, pm, sm, logP;        // axis position of (p, sub) = p pm + sub sm; twiddles exp(-2 pi i n2 k1 / 2^logP)
};

// the table of k_fftcov_split: per line of the workgroup, sub sm (the axis position of line position 0, less the lines above)
template <bool SPLIT>
__device__ __forceinline__ int* fc_line_offsets() {
  __shared__ int loff[FFTCOV_MAX_LINES];
  return loff;
}
// the inter-step twiddle of a split axis: exp(-2 pi i n2 k1 / P), k1 = bitrev(p) of the high sub-axis' L = 2^logL points
__device__ __forceinline__ double2 fc_split_twiddle(int n2, int p, int logL, int logP) {
  const int k1 = (int)(__brev((unsigned)p) >> (32 - logL));
  double s, c;
  sincospi(-ldexp((double)(n2 * k1), 1 - logP), &s, &c);
  return double2{c, s};
}

// GEN: the load is generated (the first pass of a draw); otherwise the pass of an apply, compiled to the code it always was.
// FAC: the fused pass of a factor in one dimension: FFTCOV_LOAD_FULL / FFTCOV_STORE_FULL drop the node map on that side
// SPLIT: a pass along a sub-axis (k_fftcov_split, k_fftcov_split_draw): the line map, the position limits and the fused twiddles of
// fftcov_split_args; every other instance compiles to the code it was
template <bool GEN, bool FAC = false, bool SPLIT = false>
__device__ __forceinline__ void fftcov_pass_body(const fftcov_pass_args& A, const fftcov_gen_args& G, const fftcov_split_args& S = fftcov_split_args{}) {
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
  if constexpr (SPLIT) {
    int* loff = fc_line_offsets<SPLIT>();
    for (int j = tid; j < lpw; j += nt) {
      const int64_t line = line0 + j;
      int64_t b = -1, g = -1;
      int off = 0;
      if (line < A.nlines) {
        const int64_t inner = line & (S.inner - 1), r = line >> S.loginner;
        const int64_t sub = r % S.esub, o = r / S.esub;
        b = inner + sub * S.sub_stride + (o % A.oe0) * A.os0 + (o / A.oe0) * A.os1;
        g = o * A.n0;
        off = (int)sub * S.sm;
      }
      lbase[j] = b;
      gbase[j] = g;
      loff[j] = off;
    }
  } else {
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
  }
  for (int i = tid; i < qm; i += nt) ltw[i] = A.tw[(int64_t)i * A.tw_step];
  __syncthreads();

  // entry e of the workgroup's lines -> (line j, position p): along the line on the contiguous axis, across adjacent lines on a strided one
  const int total = lpw << logL;
  const bool strided = A.stride > 1;
  const int c0 = A.col0 + 2 * pair;
  const bool has1 = c0 + 1 < A.ncols;
  if constexpr (GEN) {
    // one thread per two adjacent storage entries: positions p, p + 1 of a line on the contiguous axis, lines j, j + 1 (j even, so the
    // first entry is even: line0 and every stride above the axis are) at one position on a strided one.  No operand but Lambda is
    // read; the VALU work of the normals is what this part costs.  The bank layout of these LDS stores has not been measured either.
    const hfmi_rng::normal_consts kc = hfmi_rng::make_consts(1.0);
    const uint32_t gp = (uint32_t)(G.pair0 + pair);
    if (total == 1) {      // prod P_c = 1: the single entry 0
      if (tid == 0) {
        uint32_t r[4];
        double z[4];
        hfmi_rng::philox4x32_10(0u, 0u, gp, FFTCOV_GEN_STREAM, G.k0, G.k1, r);
        hfmi_rng::box_muller4(r, kc, z);
        const double s0 = sqrt(fmax(A.lambda[0], 0.0));
        x[0] = double2{s0 * z[0], s0 * z[1]};
      }
    }
    for (int u = tid; u < (total >> 1); u += nt) {
      const int j = strided ? 2 * (u & ((lpw >> 1) - 1)) : (u >> (logL - 1));
      const int p = strided ? (u >> (A.loglpw - 1)) : 2 * (u & ((L >> 1) - 1));
      double2 v0 = double2{0.0, 0.0}, v1 = v0;
      const int64_t b = lbase[j];
      if (b >= 0) fc_coloured_noise(G, gp, b + (int64_t)p * A.stride, A.lambda, kc, v0, v1);
      x[j * ls + p] = v0;
      x[strided ? (j + 1) * ls + p : j * ls + p + 1] = v1;
    }
  } else if constexpr (SPLIT) {
    // as below, with the axis position p pm + sub sm in place of p; a high inverse pass multiplies the conjugate twiddle in
    const int* loff = fc_line_offsets<SPLIT>();
    for (int e = tid; e < total; e += nt) {
      const int j = strided ? (e & (lpw - 1)) : (e >> logL);
      const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
      double2 v = double2{0.0, 0.0};
      const int64_t b = lbase[j];
      const int64_t pos = (int64_t)p * S.pm + loff[j];
      if (b >= 0 && pos < A.nload) {
        if (A.flags & FFTCOV_SCATTER) {
          const int64_t g = gbase[j] + pos;
          const int64_t pt = A.inv ? A.inv[g] : g;
          if (pt >= 0) {
            v.x = A.W[(int64_t)c0 * A.ldw + pt];
            if (has1) v.y = A.W[(int64_t)(c0 + 1) * A.ldw + pt];
          }
        } else {
          v = buf[b + (int64_t)p * A.stride];
        }
        if (A.flags & FFTCOV_TW_LOAD) v = fft_mulc(v, fc_split_twiddle(loff[j], p, logL, S.logP));
      }
      x[j * ls + p] = v;
    }
  } else {
    for (int e = tid; e < total; e += nt) {
      const int j = strided ? (e & (lpw - 1)) : (e >> logL);
      const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
      double2 v = double2{0.0, 0.0};
      const int64_t b = lbase[j];
      if (b >= 0 && p < A.nload) {
        if (A.flags & FFTCOV_SCATTER) {
          const int64_t g = gbase[j] + p;
          const int64_t pt = (A.inv && !(FAC && (A.flags & FFTCOV_LOAD_FULL))) ? A.inv[g] : g;
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
  }
  __syncthreads();

  if (A.flags & FFTCOV_FWD) fft_pow2_forward<false>(x, ltw, qm, L, logL, lpw, ls, tid, nt);

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

  if (A.flags & FFTCOV_INV) fft_pow2_inverse<false>(x, ltw, qm, L, logL, lpw, ls, tid, nt);

  if constexpr (SPLIT) {
    // as below, with the axis position p pm + sub sm; a high forward pass multiplies the twiddle in
    const int* loff = fc_line_offsets<SPLIT>();
    for (int e = tid; e < total; e += nt) {
      const int j = strided ? (e & (lpw - 1)) : (e >> logL);
      const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
      const int64_t b = lbase[j];
      const int64_t pos = (int64_t)p * S.pm + loff[j];
      if (b >= 0 && pos < A.nstore) {
        double2 v = x[j * ls + p];
        if (A.flags & FFTCOV_TW_STORE) v = fft_mul(v, fc_split_twiddle(loff[j], p, logL, S.logP));
        if (A.flags & FFTCOV_GATHER) {
          const int64_t g = gbase[j] + pos;
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
    return;
  }
  for (int e = tid; e < total; e += nt) {
    const int j = strided ? (e & (lpw - 1)) : (e >> logL);
    const int p = strided ? (e >> A.loglpw) : (e & (L - 1));
    const int64_t b = lbase[j];
    if (b >= 0 && p < A.nstore) {
      const double2 v = x[j * ls + p];
      if (A.flags & FFTCOV_GATHER) {
        const int64_t g = gbase[j] + p;
        const int64_t pt = (A.inv && !(FAC && (A.flags & FFTCOV_STORE_FULL))) ? A.inv[g] : g;
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

__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_fftcov_pass(fftcov_pass_args A) { fftcov_pass_body<false>(A, fftcov_gen_args{}); }
// the first pass of a draw (hfmi_grid_sampler_draw): generated load, inverse stages, store or gather
__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_fftcov_draw(fftcov_pass_args A, fftcov_gen_args G) { fftcov_pass_body<true>(A, G); }
// the one pass of a factor in one dimension (hfmi_op_grid_factor): node map on one side, the block of padded vectors on the other
__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_fftcov_factor(fftcov_pass_args A) { fftcov_pass_body<false, true>(A, fftcov_gen_args{}); }
// a pass along a sub-axis of a split embedding axis (the long route): apply, spectrum and factor passes; and the generated first pass
// of a draw when the last axis is split
__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_fftcov_split(fftcov_pass_args A, fftcov_split_args S) {
  fftcov_pass_body<false, false, true>(A, fftcov_gen_args{}, S);
}
__global__ __launch_bounds__(FFTCOV_MAX_THREADS) void k_fftcov_split_draw(fftcov_pass_args A, fftcov_gen_args G, fftcov_split_args S) {
  fftcov_pass_body<true, false, true>(A, G, S);
}

// |offset|^2 of an isotropic kernel without a metric from the per-axis distances, for the stencil table (k_fftcov_offsets): the
// arithmetic of the even column below, statement for statement (that kernel keeps its own text, and with it its device code)
__device__ __forceinline__ double fc_even_r2(int d, double dx, double dy, double dz) {
  double r2 = dx * dx;
  if (d > 1) r2 = fma(dy, dy, r2);
  if (d > 2) r2 = fma(dz, dz, r2);
  return r2;
}
// the circulant's first column of an isotropic kernel of the four first families: entry (j0, j1, j2) is the kernel at the offsets
// min(j_c, P_c - j_c) h_c, the nugget on entry 0
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
// The column of a kernel with a metric, r^2 = o^T diag(h) G diag(h) o / ell^2, of Matern-1 (PT = kcov_k1_params) and of a Matern of any
// smoothness (PT = kcov_nu_params): such a kernel is
// even in the offset vector only, not in each axis, so the column takes SIGNED offsets.  Storage position s_c stands for o_c = s_c below
// P_c / 2 and s_c - P_c above it; at s_c = P_c / 2 (P_c >= 2) the entry is the mean over both signs of that offset, taken over every
// axis at its half in the fixed order b = 0 .. 7 (bit c of b: the + sign on axis c).  An apply never reads a half position (P_c >= 2 n_c
// wherever n_c > 1); the mean keeps the column jointly even, so its transform is real and k_fftcov_spectrum and every pass after it are
// what they were.  With G = L L^T:  u = diag(h) o,  w = L^T u (w_c = sum_{e >= c} L_ec u_e, e ascending),  r^2 = w_0^2 + w_1^2 + w_2^2 in
// that order -- the arithmetic the scattered operator does on its uploaded x' = L^T x.  tests/helpers/grid_metric_twin.py states the same.
struct fftcov_metric_args {
  double l00, l10, l11, l20, l21, l22;   // the lower factor, identity when there is no metric
};
// r^2 = |L^T u|^2 of the signed offset u = diag(h) o for the stencil table (k_fftcov_offsets): the arithmetic stated above and written
// out in the signed column below, statement for statement (that kernel keeps its own text, and with it its device code)
__device__ __forceinline__ double fc_metric_r2(int d, const fftcov_metric_args& G, double u0, double u1, double u2) {
  double w0 = G.l00 * u0, w1 = 0.0, w2 = 0.0;
  if (d > 1) {
    w0 = fma(G.l10, u1, w0);
    w1 = G.l11 * u1;
  }
  if (d > 2) {
    w0 = fma(G.l20, u2, w0);
    w1 = fma(G.l21, u2, w1);
    w2 = G.l22 * u2;
  }
  double r2 = w0 * w0;
  if (d > 1) r2 = fma(w1, w1, r2);
  if (d > 2) r2 = fma(w2, w2, r2);
  return r2;
}
template <class PT>
__global__ __launch_bounds__(256) void k_fftcov_column_signed(PT K, fftcov_metric_args G, double2* buf, int64_t total, int l0, int l1, int P0,
                                                              int P1, int P2, double h0, double h1, double h2) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int s0 = (int)(e & (P0 - 1)), s1 = (int)((e >> l0) & (P1 - 1)), s2 = (int)(e >> (l0 + l1));
    const bool m0 = P0 > 1 && 2 * s0 == P0, m1 = K.d > 1 && P1 > 1 && 2 * s1 == P1, m2 = K.d > 2 && P2 > 1 && 2 * s2 == P2;
    const double o0 = (double)(2 * s0 < P0 ? s0 : s0 - P0) * h0;     // at the half: -P_c / 2, the + sign comes from b
    const double o1 = (double)(2 * s1 < P1 ? s1 : s1 - P1) * h1;
    const double o2 = (double)(2 * s2 < P2 ? s2 : s2 - P2) * h2;
    double sum = 0.0;
    int cnt = 0;
#pragma unroll 1
    for (int b = 0; b < 8; ++b) {
      if (((b & 1) && !m0) || ((b & 2) && !m1) || ((b & 4) && !m2)) continue;
      const double u0 = (b & 1) ? -o0 : o0, u1 = (b & 2) ? -o1 : o1, u2 = (b & 4) ? -o2 : o2;
      double w0 = G.l00 * u0, w1 = 0.0, w2 = 0.0;
      if (K.d > 1) {
        w0 = fma(G.l10, u1, w0);
        w1 = G.l11 * u1;
      }
      if (K.d > 2) {
        w0 = fma(G.l20, u2, w0);
        w1 = fma(G.l21, u2, w1);
        w2 = G.l22 * u2;
      }
      double r2 = w0 * w0;
      if (K.d > 1) r2 = fma(w1, w1, r2);
      if (K.d > 2) r2 = fma(w2, w2, r2);
      sum += kcov_entry(K, r2, false);
      ++cnt;
    }
    double v = sum / (double)cnt;      // cnt is 1, 2, 4 or 8
    if (e == 0) v += K.nugget;
    buf[e] = double2{v, 0.0};
  }
}
// Lambda / P: the transform of a real symmetric column is real, what the imaginary parts hold is rounding
__global__ __launch_bounds__(256) void k_fftcov_spectrum(const double2* buf, double* lambda, int64_t total, double scale) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    lambda[e] = buf[e].x * scale;
}

// the root table of a factor from the stored spectrum: negative entries (rounding, or the clipped ones) count as 0
__global__ __launch_bounds__(256) void k_fftcov_root(const double* lambda, double* root, int64_t total, double P) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    root[e] = sqrt(fmax(lambda[e], 0.0) / P);
}

// The kernel at the signed lattice offsets o in [-3, 3]^d (hfmi_op_kernel_cov_interp's diagonal): entry (o0 + 3) + 7 ((o1 + 3) + 7 (o2 + 3))
// is what the first column holds for that offset -- the column kernels' distance arithmetic (fc_even_r2 of |o_c| h_c, SIGNED = false: the
// even column's families without a metric; fc_metric_r2 of o_c h_c otherwise) and the same kcov_entry -- and no nugget.
template <class PT, bool SIGNED>
__global__ __launch_bounds__(256) void k_fftcov_offsets(PT K, fftcov_metric_args G, double* table, int total, double h0, double h1, double h2) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int o0 = e % 7 - 3, o1 = K.d > 1 ? (e / 7) % 7 - 3 : 0, o2 = K.d > 2 ? e / 49 - 3 : 0;
  const double r2 = SIGNED ? fc_metric_r2(K.d, G, (double)o0 * h0, (double)o1 * h1, (double)o2 * h2)
                           : fc_even_r2(K.d, (double)abs(o0) * h0, (double)abs(o1) * h1, (double)abs(o2) * h2);
  table[e] = kcov_entry(K, r2, false);
}

// gen: the pass's load is generated (FFTCOV_GEN, the first pass of a draw); null for every pass that loads.  table: what the fused
// multiply reads, null = Lambda / P (a factor's passes hand over the root table)
static int fftcov_launch_pass(hfmi_ctx* ctx, const fftcov_state* st, const fftcov_plan& p, const fftcov_pass& q, int pairs, int col0,
                              const double* W, int64_t ldw, double* Y, int64_t ldy, int ncols, int accumulate,
                              const fftcov_gen_args* gen = nullptr, const double* table = nullptr, const fftcov_sub* sub = nullptr,
                              int index = -1) {
  fftcov_pass_args A;
  A.buf = st->work;
  A.pair_stride = p.Ptot;
  A.tw = st->tw;
  A.tw_step = p.Pmax / q.L;
  A.lambda = table ? table : st->lambda.get();
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
  if (((q.flags & FFTCOV_GEN) != 0) != (gen != nullptr)) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: a generated load and its seed go together");
  // a factor's pass that touches the block of padded vectors on one side only: that side's scatter / gather without a node map and
  // with n0 = P_0 is the direct load / store; touching it on one side and the nodes on the other (d = 1) is k_fftcov_factor's
  const int full = q.flags & (FFTCOV_LOAD_FULL | FFTCOV_STORE_FULL);
  const bool both = (q.flags & FFTCOV_SCATTER) && (q.flags & FFTCOV_GATHER);
  if (full && !both) A.inv = nullptr, A.n0 = p.P[0];
  // tuning key "prof_level" 3 inside a profiling region: this launch between two events, with the bytes it moves
  const int part = sub ? sub->part : FFTCOV_WHOLE;
  // (nload and nstore count AXIS positions; a line of a high sub-axis holds every pm-th of them, to within one per line)
  const int pm = part == FFTCOV_HI ? sub->pm : 1;
  const int loads = std::min(q.L, (q.nload + pm - 1) / pm), stores = std::min(q.L, (q.nstore + pm - 1) / pm);
  const int pidx = prof_start_pass(ctx, q.L, 4 * (int64_t)q.flags + part, index,
                                   (double)pairs * (double)q.nlines * (16.0 * (loads + stores) + ((q.flags & FFTCOV_MUL) ? 8.0 * q.L : 0.0)));
  if (sub && sub->part != FFTCOV_WHOLE) {
    // a sub-axis: never both sides of the block (d = 1 with a split axis has three passes); the extra static table of line offsets
    if (both || q.lds + FFTCOV_LONG_STATIC_LDS > FFTCOV_LDS_BYTES || sub->esub < 1 || (sub->inner & (sub->inner - 1)))
      HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: a split pass of %d lines x %d entries cannot be launched", q.lpw, q.L);
    const fftcov_split_args S{sub->inner, sub->esub, sub->sub_stride, fftcov_log2(sub->inner), sub->pm, sub->sm, sub->logP};
    if (gen) {
      const bool paired = q.stride > 1 ? (q.lpw >= 2 && q.nlines % 2 == 0) : q.L >= 2;
      if (!paired) HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: the noise pass of %d lines x %d entries does not pair its entries", q.lpw, q.L);
      hipLaunchKernelGGL(k_fftcov_split_draw, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A, *gen, S);
    } else {
      hipLaunchKernelGGL(k_fftcov_split, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A, S);
    }
  } else if (full && both) {
    if (gen || q.nlines != 1) HFMI_FAIL(HFMI_ERR_INVALID, "grid_factor: a pass that loads and stores vectors is the single line of d = 1");
    hipLaunchKernelGGL(k_fftcov_factor, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A);
  } else if (gen) {
    // two adjacent storage entries per thread: a line of >= 2 positions, or >= 2 adjacent lines from an even line number
    const bool paired = q.stride > 1 ? (q.lpw >= 2 && q.nlines % 2 == 0) : (q.L >= 2 || (int64_t)q.lpw * q.L == 1);
    if (!paired) HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: the noise pass of %d lines x %d entries does not pair its entries", q.lpw, q.L);
    hipLaunchKernelGGL(k_fftcov_draw, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A, *gen);
  } else {
    hipLaunchKernelGGL(k_fftcov_pass, dim3((unsigned)q.grid_x, (unsigned)pairs), dim3(q.threads), (size_t)q.lds, ctx->stream, A);
  }
  prof_stop(ctx, pidx);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// The long route fixes its plans when the operator or the sampler is created, so what fftcov_launch_pass would refuse is refused
// there: every pass of every kind the object can run (the same conditions, with the largest number of pairs a launch takes).
static int fftcov_long_check(const fftcov_state* st, const int* kinds, int nkinds) {
  for (int k = 0; k < nkinds; ++k) {
    const fftcov_long_plan lp = fftcov_long_plan_passes(kinds[k], st->d, st->n, st->growth, st->max_line);
    for (int i = 0; i < lp.npasses; ++i) {
      const fftcov_pass& q = lp.pass[i];
      const fftcov_sub& s = lp.sub[i];
      const bool split = s.part != FFTCOV_WHOLE, gen = (q.flags & FFTCOV_GEN) != 0;
      const bool both = (q.flags & FFTCOV_SCATTER) && (q.flags & FFTCOV_GATHER);
      const bool full = (q.flags & (FFTCOV_LOAD_FULL | FFTCOV_STORE_FULL)) != 0;
      bool ok = q.lds + (split ? FFTCOV_LONG_STATIC_LDS : FFTCOV_STATIC_LDS) <= FFTCOV_LDS_BYTES && q.lpw <= FFTCOV_MAX_LINES && q.grid_x <= 0x7fffffff;
      if (split) ok = ok && !both && s.esub >= 1 && !(s.inner & (s.inner - 1));
      if (!split && full && both) ok = ok && !gen && q.nlines == 1;
      if (gen) ok = ok && (q.stride > 1 ? (q.lpw >= 2 && q.nlines % 2 == 0) : (q.L >= 2 || (!split && (int64_t)q.lpw * q.L == 1)));
      if (!ok)
        HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid_long: pass %d of plan kind %d (%d lines x %d entries, %d bytes of LDS, grid %lld) cannot be launched",
                  i, kinds[k], q.lpw, q.L, q.lds, (long long)q.grid_x);
    }
  }
  return HFMI_OK;
}

int64_t fftcov_points(const fftcov_state* st) { return st->N; }

void fftcov_destroy(fftcov_state* st) { delete st; }

void fftcov_describe(const fftcov_state* st, fftcov_grid_desc* out) {
  out->d = st->d;
  for (int c = 0; c < 3; ++c) out->n[c] = st->n[c], out->h[c] = st->h[c];
  out->sigma = st->sigma, out->nugget = st->nugget;
  out->all_nodes = !st->inv && st->N == st->nnodes;
  out->long_route = st->long_route;
}

bool fftcov_same_covariance(const fftcov_state* a, const fftcov_state* b) {
  bool same = a->d == b->d && a->N == b->N && a->nnodes == b->nnodes && !a->inv == !b->inv && a->family == b->family && a->sigma == b->sigma &&
              a->ell == b->ell && a->nugget == b->nugget && a->has_metric == b->has_metric && a->nu == b->nu;
  for (int c = 0; c < 3; ++c) same = same && a->n[c] == b->n[c] && a->h[c] == b->h[c];
  for (int c = 0; c < 9; ++c) same = same && a->mL[c] == b->mL[c];
  return same;
}

int fftcov_offset_table(hfmi_ctx* ctx, const fftcov_state* st, double* table) {
  const int total = st->d == 1 ? 7 : st->d == 2 ? 49 : 343;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  const fftcov_metric_args G{st->mL[0], st->mL[3], st->mL[4], st->mL[6], st->mL[7], st->mL[8]};
  // the family dispatch of fftcov_create_device's column
  if (st->family == HFMI_KERNEL_MATERN) {
    kcov_nu_params K;
    HFMI_TRY(kcov_nu_params_init_as(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, 0.0, kcov_nu_ref{st->nu, st->nuca, st->nutab}));
    hipLaunchKernelGGL((k_fftcov_offsets<kcov_nu_params, true>), grid, block, 0, ctx->stream, K, G, table, total, st->h[0], st->h[1], st->h[2]);
  } else if (st->family == HFMI_KERNEL_MATERN1) {
    kcov_k1_params K;
    HFMI_TRY(kcov_params_init_as(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, 0.0));
    hipLaunchKernelGGL((k_fftcov_offsets<kcov_k1_params, true>), grid, block, 0, ctx->stream, K, G, table, total, st->h[0], st->h[1], st->h[2]);
  } else {
    kcov_params K;
    HFMI_TRY(kcov_params_init(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, 0.0));
    if (st->has_metric)
      hipLaunchKernelGGL((k_fftcov_offsets<kcov_params, true>), grid, block, 0, ctx->stream, K, G, table, total, st->h[0], st->h[1], st->h[2]);
    else
      hipLaunchKernelGGL((k_fftcov_offsets<kcov_params, false>), grid, block, 0, ctx->stream, K, G, table, total, st->h[0], st->h[1], st->h[2]);
  }
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// inv: the node map's inverse, on the host, or on the device (inv_on_device: a sampler copies its operator's)
static int fftcov_create_device(hfmi_ctx* ctx, fftcov_state* st, const int64_t* inv, bool inv_on_device = false) {
  const fftcov_plan& p = st->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipFuncSetAttribute((const void*)k_fftcov_pass, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - FFTCOV_STATIC_LDS));
  HIP_TRY(hipFuncSetAttribute((const void*)k_fftcov_draw, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - FFTCOV_STATIC_LDS));
  HIP_TRY(hipFuncSetAttribute((const void*)k_fftcov_factor, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - FFTCOV_STATIC_LDS));
  if (st->long_route) {
    HIP_TRY(hipFuncSetAttribute((const void*)k_fftcov_split, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - FFTCOV_LONG_STATIC_LDS));
    HIP_TRY(hipFuncSetAttribute((const void*)k_fftcov_split_draw, hipFuncAttributeMaxDynamicSharedMemorySize, FFTCOV_LDS_BYTES - FFTCOV_LONG_STATIC_LDS));
  }
  // the work buffer of one pair and Lambda: what decides whether the padded grid fits at all
  hipError_t e = (hipError_t)st->work.alloc((size_t)p.pair_bytes / sizeof(double2));
  if (e == hipSuccess) e = (hipError_t)st->lambda.alloc((size_t)p.Ptot);
  if (e != hipSuccess) {
    HFMI_FAIL(HFMI_ERR_HIP, "kernel_cov_grid: the padded grid %d x %d x %d needs %lld bytes of work buffer per pair of vectors and %lld bytes of spectrum: %s",
              p.P[0], p.P[1], p.P[2], (long long)p.pair_bytes, (long long)(p.Ptot * 8), hipGetErrorString(e));
  }
  if (inv) {
    OWN_TRY(st->inv.alloc((size_t)st->nnodes));
    HIP_TRY(hipMemcpy(st->inv, inv, (size_t)st->nnodes * sizeof(int64_t), inv_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  }
  HFMI_TRY(fft_twiddles_upload(st->tw, p.Pmax, p.twiddles));
  // Lambda = FFT(first column) / P by the forward passes over the whole padded array
  const int64_t blocks = std::min<int64_t>((p.Ptot + 255) / 256, (int64_t)ctx->num_cus * 8);
  const fftcov_metric_args G{st->mL[0], st->mL[3], st->mL[4], st->mL[6], st->mL[7], st->mL[8]};
  if (st->family == HFMI_KERNEL_MATERN) {
    kcov_nu_params K;
    HFMI_TRY(kcov_nu_upload(ctx, st->nu, &st->nutab, &st->nuca));
    HFMI_TRY(kcov_nu_params_init_as(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, st->nugget, kcov_nu_ref{st->nu, st->nuca, st->nutab}));
    hipLaunchKernelGGL(k_fftcov_column_signed<kcov_nu_params>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, K, G, st->work, p.Ptot,
                       fftcov_log2(p.P[0]), fftcov_log2(p.P[1]), p.P[0], p.P[1], p.P[2], st->h[0], st->h[1], st->h[2]);
  } else if (st->family == HFMI_KERNEL_MATERN1) {
    kcov_k1_params K;
    HFMI_TRY(kcov_params_init_as(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, st->nugget));   // no coordinates are read
    hipLaunchKernelGGL(k_fftcov_column_signed<kcov_k1_params>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, K, G, st->work, p.Ptot,
                       fftcov_log2(p.P[0]), fftcov_log2(p.P[1]), p.P[0], p.P[1], p.P[2], st->h[0], st->h[1], st->h[2]);
  } else {
    kcov_params K;
    HFMI_TRY(kcov_params_init(&K, st->lambda, 1, st->d, st->family, st->sigma, st->ell, st->nugget));
    if (st->has_metric)
      hipLaunchKernelGGL(k_fftcov_column_signed<kcov_params>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, K, G, st->work, p.Ptot,
                         fftcov_log2(p.P[0]), fftcov_log2(p.P[1]), p.P[0], p.P[1], p.P[2], st->h[0], st->h[1], st->h[2]);
    else      // one of the four first families without a metric: the even column, as ever
      hipLaunchKernelGGL(k_fftcov_column, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, K, st->work, p.Ptot, fftcov_log2(p.P[0]),
                         fftcov_log2(p.P[1]), p.P[0], p.P[1], p.P[2], st->h[0], st->h[1], st->h[2]);
  }
  HIP_TRY(hipGetLastError());
  if (st->long_route) {
    const fftcov_long_plan sp = fftcov_long_plan_passes(FFTCOV_KIND_SPECTRUM, st->d, st->n, st->growth, st->max_line);
    for (int i = 0; i < sp.npasses; ++i)
      HFMI_TRY(fftcov_launch_pass(ctx, st, sp.base, sp.pass[i], 1, 0, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, &sp.sub[i]));
  } else {
    const fftcov_plan sp = fftcov_sample_plan_passes(st->d, st->n, st->growth, true);   // growth 0: fftcov_plan_passes(d, n, true)
    for (int i = 0; i < sp.npasses; ++i) HFMI_TRY(fftcov_launch_pass(ctx, st, sp, sp.pass[i], 1, 0, nullptr, 0, nullptr, 0, 0, 0));
  }
  hipLaunchKernelGGL(k_fftcov_spectrum, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, st->work, st->lambda, p.Ptot, 1.0 / (double)p.Ptot);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return HFMI_OK;
}

int fftcov_create(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N, int family, double sigma,
                  double ell, double nugget, const double* metric_factor, fftcov_state** out, int max_line, double nu) {
  const int64_t maxn = max_line > 0 ? FFTCOV_LONG_MAXN : FFTCOV_MAXN;
  int64_t nnodes = 1;
  for (int c = 0; c < d; ++c) {
    if (n[c] < 1 || n[c] > maxn)
      HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: n[%d] = %lld is not in 1 .. %lld", c, (long long)n[c], (long long)maxn);
    if (!(h[c] > 0.0) || !isfinite(h[c])) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid: spacing h[%d] must be positive and finite", c);
    nnodes *= n[c];
  }
  if (max_line > 0 && !fftcov_long_feasible(d, n, 0, max_line))
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_grid_long: an embedding axis is longer than max_line^2 = %lld (tuning key \"fftcov_max_line\" = %d)",
              (long long)max_line * max_line, max_line);
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
  if (metric_factor) {      // d x d row-major lower factor -> the 3 x 3 of the state
    st->has_metric = true;
    for (int r = 0; r < d; ++r)
      for (int c = 0; c < d; ++c) st->mL[3 * r + c] = metric_factor[(size_t)r * d + c];
  }
  st->nu = nu;
  if (max_line > 0) {
    st->long_route = true;
    st->max_line = max_line;
    st->lplan = fftcov_long_plan_passes(FFTCOV_KIND_APPLY, d, st->n, 0, max_line);
    st->plan = st->lplan.base;
    const int kinds[] = {FFTCOV_KIND_APPLY, FFTCOV_KIND_SPECTRUM};
    HFMI_TRY(fftcov_long_check(st.get(), kinds, 2));
  } else {
    st->plan = fftcov_plan_passes(d, st->n, false);
  }
  const int s = fftcov_create_device(ctx, st.get(), host_nodes ? inv.data() : nullptr);
  if (s != HFMI_OK) {
    (void)hipStreamSynchronize(ctx->stream);      // before the buffers go: the kernels queued so far use them
    return s;
  }
  *out = st.release();
  return HFMI_OK;
}

// chunks of `nvec` columns, and a work buffer that holds one
static int fftcov_fit_work(hfmi_ctx* ctx, fftcov_state* st, fftcov_plan& p, int nvec) {
  return fft_fit_work(ctx, st->work, p, p.Ptot, nvec);
}

int fftcov_apply(hfmi_ctx* ctx, fftcov_state* st, const double* W, int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate) {
  if (nvec < 1) return HFMI_OK;
  if (st->long_route) {
    fftcov_long_plan lp = st->lplan;
    HFMI_TRY(fftcov_fit_work(ctx, st, lp.base, nvec));
    for (int c = 0; c < lp.base.nchunks; ++c) {
      const int pair0 = c * lp.base.chunk_pairs, pairs = std::min(lp.base.chunk_pairs, lp.base.pairs - pair0);
      for (int i = 0; i < lp.npasses; ++i)
        HFMI_TRY(fftcov_launch_pass(ctx, st, lp.base, lp.pass[i], pairs, 2 * pair0, W, ldw, Y, ldy, nvec, accumulate, nullptr, nullptr, &lp.sub[i], i));
    }
    return HFMI_OK;
  }
  fftcov_plan p = st->plan;
  HFMI_TRY(fftcov_fit_work(ctx, st, p, nvec));
  for (int c = 0; c < p.nchunks; ++c) {
    const int pair0 = c * p.chunk_pairs, pairs = std::min(p.chunk_pairs, p.pairs - pair0);
    for (int i = 0; i < p.npasses; ++i) HFMI_TRY(fftcov_launch_pass(ctx, st, p, p.pass[i], pairs, 2 * pair0, W, ldw, Y, ldy, nvec, accumulate));
  }
  return HFMI_OK;
}

// ------------------------------------------------------------------ exact draws m ~ N(0, C) by circulant embedding (hfmi_grid_sampler_*)
// The rules -- the grown embedding, the passes of a draw, the noise's element map, the floor and the clip's bound -- are in
// hfmi_fftcov_plan.h.  A sampler is a state of its own (grid, kernel, node map, twiddles, Lambda of ITS embedding, work buffer): it
// does not refer to the operator it was made from.

// extremes of the stored spectrum: a plain two-stage reduction, fixed grid, fixed order, vector stores and no atomics, so that two
// creations agree bit for bit
struct fftcov_extremes {
  double lmin, lmax, negsum;
  int64_t nneg;
};
constexpr int FFTCOV_EXT_THREADS = 256;
constexpr int FFTCOV_EXT_BLOCKS = 256;   // most partial records: the second stage is one workgroup with one thread each
__device__ __forceinline__ fftcov_extremes fc_ext_join(const fftcov_extremes& a, const fftcov_extremes& b) {
  return fftcov_extremes{fmin(a.lmin, b.lmin), fmax(a.lmax, b.lmax), a.negsum + b.negsum, a.nneg + b.nneg};
}
// FINAL: thread t of the one workgroup takes partial record t; otherwise block b takes the entries b, b + blocks, ... of 256-entry tiles
template <bool FINAL>
__global__ __launch_bounds__(FFTCOV_EXT_THREADS) void k_fftcov_extremes(const double* lambda, int64_t total, const fftcov_extremes* part,
                                                                        int nparts, fftcov_extremes* out) {
  __shared__ fftcov_extremes red[FFTCOV_EXT_THREADS];
  const int tid = threadIdx.x;
  fftcov_extremes v{INFINITY, -INFINITY, 0.0, 0};
  if (FINAL) {
    if (tid < nparts) v = part[tid];
  } else {
    for (int64_t e = (int64_t)blockIdx.x * FFTCOV_EXT_THREADS + tid; e < total; e += (int64_t)gridDim.x * FFTCOV_EXT_THREADS) {
      const double l = lambda[e];
      v.lmin = fmin(v.lmin, l);
      v.lmax = fmax(v.lmax, l);
      if (l < 0.0) v.negsum += l, ++v.nneg;
    }
  }
  red[tid] = v;
  __syncthreads();
  for (int s = FFTCOV_EXT_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fc_ext_join(red[tid], red[tid + s]);
    __syncthreads();
  }
  if (tid == 0) out[FINAL ? 0 : blockIdx.x] = red[0];
}

static int fftcov_spectrum_extremes(hfmi_ctx* ctx, const fftcov_state* st, fftcov_extremes* host) {
  const int64_t total = st->plan.Ptot;
  const int blocks = (int)std::min<int64_t>((total + FFTCOV_EXT_THREADS - 1) / FFTCOV_EXT_THREADS, FFTCOV_EXT_BLOCKS);
  dev_buf<fftcov_extremes> part;
  OWN_TRY(part.alloc((size_t)blocks + 1));
  hipLaunchKernelGGL(k_fftcov_extremes<false>, dim3((unsigned)blocks), dim3(FFTCOV_EXT_THREADS), 0, ctx->stream, st->lambda.get(), total, nullptr, 0,
                     part.get());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fftcov_extremes<true>, dim3(1), dim3(FFTCOV_EXT_THREADS), 0, ctx->stream, nullptr, 0, part.get(), blocks, part.get() + blocks);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(host, part.get() + blocks, sizeof(*host), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return HFMI_OK;
}

struct hfmi_grid_sampler {
  hfmi_ctx* ctx = nullptr;
  std::shared_ptr<fftcov_state> st;            // shared with the factor operators made from this sampler (hfmi_op_grid_factor)
  double lambda_min = 0.0, lambda_max = 0.0;   // eigenvalues of the embedding's circulant (the stored spectrum times prod P_c)
  int64_t n_clipped = 0;
  double cov_error_bound = 0.0;
};
const fftcov_state* grid_sampler_state(const hfmi_grid_sampler* s) { return s->st.get(); }
hfmi_ctx* grid_sampler_ctx(const hfmi_grid_sampler* s) { return s->ctx; }

// the state of the operator's grid at one growth, its spectrum and the extremes of that
// max_line > 0: the long route's embedding and passes (hfmi_grid_sampler_create_long)
static int grid_sampler_try(hfmi_ctx* ctx, const fftcov_state* src, int growth, int max_line, std::shared_ptr<fftcov_state>& st,
                            fftcov_extremes* ext) {
  st.reset(new (std::nothrow) fftcov_state(), fftcov_destroy);
  if (!st) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  st->d = src->d;
  for (int c = 0; c < 3; ++c) st->n[c] = src->n[c], st->h[c] = src->h[c];
  st->N = src->N, st->nnodes = src->nnodes;
  st->family = src->family, st->sigma = src->sigma, st->ell = src->ell, st->nugget = src->nugget;
  st->has_metric = src->has_metric;
  std::copy(src->mL, src->mL + 9, st->mL);
  st->nu = src->nu;
  st->growth = growth;
  if (max_line > 0) {
    st->long_route = true;
    st->max_line = max_line;
    st->lplan = fftcov_long_plan_passes(FFTCOV_KIND_DRAW, st->d, st->n, growth, max_line);
    st->plan = st->lplan.base;
    const int kinds[] = {FFTCOV_KIND_DRAW, FFTCOV_KIND_FACTOR, FFTCOV_KIND_FACTOR_T, FFTCOV_KIND_SPECTRUM};
    HFMI_TRY(fftcov_long_check(st.get(), kinds, 4));
  } else {
    st->plan = fftcov_sample_plan_passes(st->d, st->n, growth, false);
  }
  HFMI_TRY(fftcov_create_device(ctx, st.get(), src->inv, true));
  return fftcov_spectrum_extremes(ctx, st.get(), ext);
}

// long: the route of the operator's own (hfmi_grid_sampler_create_long, an operator of hfmi_op_kernel_cov_grid_long); otherwise the old
// route's embedding and passes, which an operator of either route with axes of at most FFTCOV_MAXN nodes takes
static int grid_sampler_create(hfmi_op* op, int max_growth, int clip, bool long_route, hfmi_grid_sampler** out) {
  if (!op || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (op->kind != OP_KERNEL_COV_GRID || !op->fc)
    HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: the operator is not a kernel covariance on a grid (hfmi_op_kernel_cov_grid)");
  const int gmax = long_route ? FFTCOV_LONG_MAX_GROWTH : FFTCOV_MAX_GROWTH;
  if (max_growth < 0 || max_growth > gmax) HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: max_growth = %d outside 0..%d", max_growth, gmax);
  hfmi_ctx* ctx = op->ctx;
  const fftcov_state* src = op->fc;
  if (long_route && !src->long_route)
    HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler_create_long: the operator is not one of hfmi_op_kernel_cov_grid_long");
  for (int c = 0; c < src->d; ++c)
    if (!long_route && src->n[c] > FFTCOV_MAXN)
      HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: axis %d has %lld nodes, more than %d: hfmi_grid_sampler_create_long", c, (long long)src->n[c], FFTCOV_MAXN);
  const int max_line = long_route ? src->max_line : 0;
  auto feasible = [&](int g) {
    return long_route ? fftcov_long_feasible(src->d, src->n, g, max_line) : fftcov_growth_feasible(src->d, src->n, g);
  };
  std::unique_ptr<hfmi_grid_sampler> s(new (std::nothrow) hfmi_grid_sampler());
  if (!s) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  s->ctx = ctx;
  fftcov_extremes ext{};
  bool definite = false;
  int g = std::min(fftcov_min_growth_knob(), max_growth);
  while (g > 0 && !feasible(g)) --g;
  for (;; ++g) {
    const int status = grid_sampler_try(ctx, src, g, max_line, s->st, &ext);
    if (status != HFMI_OK) {
      (void)hipStreamSynchronize(ctx->stream);    // before the buffers go: the kernels queued so far use them
      return status;
    }
    definite = ext.lmin >= -fftcov_floor(s->st->plan.Ptot, ext.lmax);
    if (definite || g == max_growth || !feasible(g + 1)) break;
  }
  if (!definite && !clip)
    HFMI_FAIL(HFMI_ERR_INVALID,
              "grid_sampler: the embedding %d x %d x %d (growth %d, the last one tried) is indefinite: lambda_min / lambda_max = %.3e; allow a "
              "larger growth or ask for clipping",
              s->st->plan.P[0], s->st->plan.P[1], s->st->plan.P[2], g, ext.lmin / ext.lmax);
  const double P = (double)s->st->plan.Ptot;
  s->lambda_min = ext.lmin * P, s->lambda_max = ext.lmax * P;
  s->n_clipped = definite ? 0 : ext.nneg;
  s->cov_error_bound = definite ? 0.0 : -ext.negsum;
  *out = s.release();
  return HFMI_OK;
}
extern "C" int hfmi_grid_sampler_create(hfmi_op* op, int max_growth, int clip, hfmi_grid_sampler** out) {
  return grid_sampler_create(op, max_growth, clip, false, out);
}
extern "C" int hfmi_grid_sampler_create_long(hfmi_op* op, int max_growth, int clip, hfmi_grid_sampler** out) {
  return grid_sampler_create(op, max_growth, clip, true, out);
}

extern "C" int hfmi_grid_sampler_info(const hfmi_grid_sampler* s, int* growth, int64_t* P, double* lambda_min, double* lambda_max,
                                      int64_t* n_clipped, double* cov_error_bound) {
  if (!s) HFMI_FAIL(HFMI_ERR_INVALID, "null sampler");
  if (growth) *growth = s->st->growth;
  if (P)
    for (int c = 0; c < 3; ++c) P[c] = s->st->plan.P[c];
  if (lambda_min) *lambda_min = s->lambda_min;
  if (lambda_max) *lambda_max = s->lambda_max;
  if (n_clipped) *n_clipped = s->n_clipped;
  if (cov_error_bound) *cov_error_bound = s->cov_error_bound;
  return HFMI_OK;
}

extern "C" int hfmi_grid_sampler_draw(hfmi_grid_sampler* s, const hfmi_block* Y, uint64_t seed, int64_t first_sample, int accumulate) {
  if (!s || !Y) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  fftcov_state* st = s->st.get();
  if (Y->N != st->N) HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: draws have length %lld, the block's vectors %lld", (long long)st->N, (long long)Y->N);
  if (first_sample < 0 || (first_sample & 1))
    HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: first_sample = %lld must be even and not negative (draws 2 p and 2 p + 1 are one transform)",
              (long long)first_sample);
  const int ncols = Y->nvec;
  if (first_sample / 2 + (ncols + 1) / 2 > ((int64_t)1 << 32))
    HFMI_FAIL(HFMI_ERR_INVALID, "grid_sampler: a seed has 2^33 draws, first_sample = %lld with %d columns goes past them", (long long)first_sample, ncols);
  if (ncols < 1) return HFMI_OK;
  hfmi_ctx* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  if (st->long_route) {
    fftcov_long_plan lp = st->lplan;
    HFMI_TRY(fftcov_fit_work(ctx, st, lp.base, ncols));
    for (int c = 0; c < lp.base.nchunks; ++c) {
      const int pair0 = c * lp.base.chunk_pairs, pairs = std::min(lp.base.chunk_pairs, lp.base.pairs - pair0);
      const fftcov_gen_args gen{(uint32_t)seed, (uint32_t)(seed >> 32), first_sample / 2 + pair0};
      for (int i = 0; i < lp.npasses; ++i)
        HFMI_TRY(fftcov_launch_pass(ctx, st, lp.base, lp.pass[i], pairs, 2 * pair0, nullptr, 0, Y->p, Y->ld, ncols, accumulate != 0,
                                    i == 0 ? &gen : nullptr, nullptr, &lp.sub[i]));
    }
    return HFMI_OK;
  }
  fftcov_plan p = st->plan;
  HFMI_TRY(fftcov_fit_work(ctx, st, p, ncols));
  for (int c = 0; c < p.nchunks; ++c) {
    const int pair0 = c * p.chunk_pairs, pairs = std::min(p.chunk_pairs, p.pairs - pair0);
    const fftcov_gen_args gen{(uint32_t)seed, (uint32_t)(seed >> 32), first_sample / 2 + pair0};
    for (int i = 0; i < p.npasses; ++i)
      HFMI_TRY(fftcov_launch_pass(ctx, st, p, p.pass[i], pairs, 2 * pair0, nullptr, 0, Y->p, Y->ld, ncols, accumulate != 0, i == 0 ? &gen : nullptr));
  }
  return HFMI_OK;
}

extern "C" int hfmi_grid_sampler_destroy(hfmi_grid_sampler* s) {
  if (!s) return HFMI_OK;
  (void)hipStreamSynchronize(s->ctx->stream);     // draws queued so far use the buffers
  delete s;
  return HFMI_OK;
}

// ------------------------------------------------------------------ the factor C = S S^T of a sampler's embedding (hfmi_op_grid_factor)
// The rules and the pass lists are in hfmi_fftcov_plan.h.  A factor operator shares the sampler's state (grid, node map, twiddles,
// Lambda, work buffer) and adds the root table to it, once, at the first factor of a sampler: Lambda itself is never written, so the
// sampler's draws are what they were.  Whoever goes last, sampler or operator, deletes the state.
// the root table of a sampler's state, made the first time a factor of it is asked for (hfmi_op_grid_factor, hfmi_op_interp_factor)
int grid_sampler_root(hfmi_grid_sampler* s, const char* who) {
  hfmi_ctx* ctx = s->ctx;
  fftcov_state* st = s->st.get();
  HIP_TRY(hipSetDevice(ctx->device));
  if (st->root) return HFMI_OK;
  const int64_t total = st->plan.Ptot;
  dev_buf<double> root;
  const hipError_t e = (hipError_t)root.alloc((size_t)total);
  if (e != hipSuccess)
    HFMI_FAIL(HFMI_ERR_HIP, "%s: the root table of the embedding %d x %d x %d needs %lld bytes: %s", who, st->plan.P[0], st->plan.P[1],
              st->plan.P[2], (long long)(total * 8), hipGetErrorString(e));
  const int64_t blocks = std::min<int64_t>((total + 255) / 256, (int64_t)ctx->num_cus * 8);
  hipLaunchKernelGGL(k_fftcov_root, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, st->lambda.get(), root.get(), total, (double)total);
  const hipError_t launched = hipGetLastError();
  const hipError_t done = hipStreamSynchronize(ctx->stream);   // whatever happened: `root` must not go while a kernel may write it
  HIP_TRY(launched);
  HIP_TRY(done);
  st->root = std::move(root);
  return HFMI_OK;
}
std::shared_ptr<fftcov_state> grid_sampler_share(hfmi_grid_sampler* s) { return s->st; }
int64_t fftcov_padded_len(const fftcov_state* st) { return st->plan.Ptot; }

extern "C" int hfmi_op_grid_factor(hfmi_grid_sampler* s, int transpose, hfmi_op** out) {
  if (!s || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (transpose != 0 && transpose != 1) HFMI_FAIL(HFMI_ERR_INVALID, "grid_factor: transpose = %d is not 0 (S) or 1 (S^T)", transpose);
  hfmi_ctx* ctx = s->ctx;
  HFMI_TRY(grid_sampler_root(s, "grid_factor"));
  std::unique_ptr<hfmi_op> op(new (std::nothrow) hfmi_op());
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->ctx = ctx;
  op->kind = OP_GRID_FACTOR;
  op->fac = s->st;
  op->fac_transpose = transpose;
  *out = op.release();
  return HFMI_OK;
}

int fftcov_factor_apply(hfmi_ctx* ctx, fftcov_state* st, int transpose, const hfmi_block* W, hfmi_block* Y, int accumulate) {
  const int64_t Ptot = st->plan.Ptot, nin = transpose ? st->N : Ptot, nout = transpose ? Ptot : st->N;
  if (W->N != nin || Y->N != nout)
    HFMI_FAIL(HFMI_ERR_INVALID, "grid_factor: %s maps vectors of length %lld to length %lld, got %lld -> %lld", transpose ? "S^T" : "S",
              (long long)nin, (long long)nout, (long long)W->N, (long long)Y->N);
  const int nvec = W->nvec;
  if (nvec < 1) return HFMI_OK;
  if (st->long_route) {
    fftcov_long_plan lp = fftcov_long_plan_passes(transpose ? FFTCOV_KIND_FACTOR_T : FFTCOV_KIND_FACTOR, st->d, st->n, st->growth, st->max_line);
    HFMI_TRY(fftcov_fit_work(ctx, st, lp.base, nvec));
    for (int c = 0; c < lp.base.nchunks; ++c) {
      const int pair0 = c * lp.base.chunk_pairs, pairs = std::min(lp.base.chunk_pairs, lp.base.pairs - pair0);
      for (int i = 0; i < lp.npasses; ++i)
        HFMI_TRY(fftcov_launch_pass(ctx, st, lp.base, lp.pass[i], pairs, 2 * pair0, W->p, W->ld, Y->p, Y->ld, nvec, accumulate, nullptr, st->root,
                                    &lp.sub[i]));
    }
    return HFMI_OK;
  }
  fftcov_plan p = fftcov_factor_plan_passes(st->d, st->n, st->growth, transpose);
  HFMI_TRY(fftcov_fit_work(ctx, st, p, nvec));
  for (int c = 0; c < p.nchunks; ++c) {
    const int pair0 = c * p.chunk_pairs, pairs = std::min(p.chunk_pairs, p.pairs - pair0);
    for (int i = 0; i < p.npasses; ++i)
      HFMI_TRY(fftcov_launch_pass(ctx, st, p, p.pass[i], pairs, 2 * pair0, W->p, W->ld, Y->p, Y->ld, nvec, accumulate, nullptr, st->root));
  }
  return HFMI_OK;
}
