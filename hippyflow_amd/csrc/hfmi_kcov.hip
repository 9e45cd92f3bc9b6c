// Matrix-free kernel covariance  Y (+)= C W,  C_ij = sigma^2 phi(|x_i - x_j| / ell) + nugget delta_ij  (hfmi_op_kernel_cov).
// C is never stored: every entry is evaluated in registers, in the A-operand layout of v_mfma_f64_16x16x4_f64 (lane l holds
// A[row l & 15][k l >> 4]), so ONE evaluation per lane is a 16 x 4 slab of C, and that slab is multiplied into every 16-column tile of
// W.  Only the coordinates, W and Y move: 16 N k bytes instead of 8 N^2.
//
// Work split: a workgroup of 8 waves owns 128 rows of Y (16 per wave) and sweeps ALL of j = 0 .. N-1 in order, 64 rows of W at a time
// through LDS; the accumulators (one d4 per column tile, at most 9 = 144 columns) stay in registers for the whole sweep.  No atomics, no
// split of j over workgroups: the summation order of every element is fixed (slab by slab, k = 0..3 inside the instruction), so two
// applies are bit-identical.  The CPU twin tests/helpers/kernel_cov_twin.py walks the same order.
//
// Overlap: the evaluation (differences, sqrt, polynomial, exp: a few tens of fp64 VALU instructions) of slab s+1 is issued before the MFMAs
// of slab s and has no dependence on them, and two waves share each SIMD, so the VALU work runs beside the matrix pipe.  The next chunk of W
// is fetched into registers before the current one is consumed and written to LDS after it.
//
// LDS image of a chunk: [column][66] doubles (64 rows + 2 of padding).  A column's stride is 132 dwords = 4 (mod 64 banks), so the 16
// columns x 2 k-rows a half-wave reads as its B fragment fall on 32 different bank pairs, and the staging stores (lanes along the rows of
// one column) are contiguous.
//
// Rectangular form (the kcov_cross_params instances; hfmi_op_kernel_cross_cov, hfmi_op_kernel_cov_rows):  Y (M rows) (+)= K W (N rows),
// K_ij = sigma^2 phi(|t_i - s_j| / ell) + nugget [j == i + diag_offset].  Same layout and the same sweep over ALL sources, with the row
// coordinates read from a second point set t (M targets) and the nugget on the source index i + diag_offset.  A row's sum does not depend
// on the tile, wave or lane row that holds it, so with t = s[row0 : row0 + M] and diag_offset = row0 the result is the same bits as rows
// row0 .. row0 + M - 1 of the square apply: a row slab per rank, summed over the ranks, IS the square apply.  The square instances take
// kcov_params as before: neither their arguments nor their registers know of the second set.
//
// Matern-1 (the kcov_k1_params / kcov_k1_cross_params instances): the same kernel with phi = a K_1(a) of hfmi_kcov_k1.h behind kcov_entry.
// Its evaluation is about 100 fp64 VALU instructions with log, exp, sqrt and a division, so that apply is bound by the VALU, not by the
// matrix pipe; eval(s + 1) is still issued before the MFMAs of slab s.  A metric (r^2 = delta^T G delta) never reaches this unit: the
// operator uploads x' = L^T x, G = L L^T (hfmi_op.hip).
//
// Matern of any smoothness (the kcov_nu_params / kcov_nu_cross_params instances): phi_nu of hfmi_kcov_nu.h behind kcov_entry, its table
// words read by scalar loads from a buffer the operator owns.  2.3 times the time of Matern-1 per entry (N = 32768, k = 32, nu = 1.25).
#include <algorithm>

#include "hfmi_gemm_common.h"
#include "hfmi_kcov_eval.h"

#define KC_JC 64            // rows of W (values of j) per LDS chunk
#define KC_JCP 66           // padded column stride of the LDS image
#define KC_WAVES 8
#define KC_ROWS (16 * KC_WAVES)
#define KC_MAXT 9           // column tiles per panel: 144 columns, k = 138 is one pass

// what differs between the two argument types: the number of rows, their coordinates, and the source index a row's nugget sits on
__device__ __forceinline__ int64_t kcov_targets(const kcov_params& P) { return P.N; }
__device__ __forceinline__ int64_t kcov_targets(const kcov_cross_params& P) { return P.M; }
__device__ __forceinline__ const double* kcov_t0(const kcov_params& P) { return P.x0; }
__device__ __forceinline__ const double* kcov_t1(const kcov_params& P) { return P.x1; }
__device__ __forceinline__ const double* kcov_t2(const kcov_params& P) { return P.x2; }
__device__ __forceinline__ const double* kcov_t0(const kcov_cross_params& P) { return P.t0; }
__device__ __forceinline__ const double* kcov_t1(const kcov_cross_params& P) { return P.t1; }
__device__ __forceinline__ const double* kcov_t2(const kcov_cross_params& P) { return P.t2; }
__device__ __forceinline__ int64_t kcov_diag_source(const kcov_params&, int64_t gi) { return gi; }
__device__ __forceinline__ int64_t kcov_diag_source(const kcov_cross_params& P, int64_t gi) { return P.diag_offset >= 0 ? gi + P.diag_offset : -1; }

// The Matern-1 evaluation needs some 40 VGPRs more than the others.  In its instances the leading dimensions pass through an empty
// statement where they are used, so that the 64-bit column offsets of the prefetch and of the final store are computed there and not
// kept in registers across the slab loop: 9 column tiles then fit without a spill (246 VGPRs).  The other instances do not see this.
template <class PT> constexpr bool kcov_tight_registers = false;
template <> constexpr bool kcov_tight_registers<kcov_k1_params> = true;
template <> constexpr bool kcov_tight_registers<kcov_k1_cross_params> = true;
template <> constexpr bool kcov_tight_registers<kcov_nu_params> = true;
template <> constexpr bool kcov_tight_registers<kcov_nu_cross_params> = true;

template <int NT, class PT>      // PT: kcov_params (square) or kcov_cross_params (rectangular); kcov_k1_params / kcov_k1_cross_params: Matern-1; kcov_nu_*: any nu
__global__ __launch_bounds__(64 * KC_WAVES) void k_kcov(PT P, const double* __restrict__ W, int64_t ldw, double* __restrict__ Y,
                                                        int64_t ldy, int ncols, int accumulate) {
  __shared__ double wl[16 * NT * KC_JCP];
  __shared__ double xl[3 * KC_JC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t N = P.N;                       // sources: rows of W
  const int64_t M = kcov_targets(P);           // targets: rows of Y
  const int d = P.d;
  const int64_t ntiles = (M + KC_ROWS - 1) / KC_ROWS;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * KC_ROWS + wave * 16;
    const int64_t gi = row0 + lr;
    const bool iv = gi < M;
    // the source index the nugget of row gi sits on: gi itself for the square operator, none (-1) for disjoint point sets
    const int64_t gd = kcov_diag_source(P, gi);
    const double xi0 = iv ? kcov_t0(P)[gi] : 0.0;
    const double xi1 = (iv && d > 1) ? kcov_t1(P)[gi] : 0.0;
    const double xi2 = (iv && d > 2) ? kcov_t2(P)[gi] : 0.0;
    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    // chunk prefetch: wave w fetches rows j0 + lane of columns w, w + 8, ... (512 contiguous bytes per load), and waves 0..2 one
    // coordinate array each; rows >= N and columns >= ncols are staged as zeros
    double pf[2 * NT], xpf;
    auto fetch = [&](int64_t j0) {
      const int64_t j = j0 + lane;
      if constexpr (kcov_tight_registers<PT>) asm volatile("" : "+s"(ldw));
#pragma unroll
      for (int e = 0; e < 2 * NT; ++e) {
        const int col = wave + KC_WAVES * e;
        pf[e] = (col < ncols && j < N) ? W[(int64_t)col * ldw + j] : 0.0;
      }
      const double* xw = wave == 0 ? P.x0 : wave == 1 ? P.x1 : P.x2;
      xpf = (wave < d && j < N) ? xw[j] : 0.0;
    };
    fetch(0);
    for (int64_t j0 = 0; j0 < N; j0 += KC_JC) {
      __syncthreads();          // every wave is done with the previous chunk
#pragma unroll
      for (int e = 0; e < 2 * NT; ++e) wl[(wave + KC_WAVES * e) * KC_JCP + lane] = pf[e];
      if (wave < 3) xl[wave * KC_JC + lane] = xpf;
      __syncthreads();
      if (j0 + KC_JC < N) fetch(j0 + KC_JC);
      const int64_t left = N - j0;
      const int nslab = left >= KC_JC ? KC_JC / 4 : (int)((left + 3) / 4);
      // one entry of K per lane: row gi, column j0 + 4 s + lk
      auto eval = [&](int s) -> double {
        const int jj = 4 * s + lk;
        const int64_t gj = j0 + jj;
        const double dx = xi0 - xl[jj];
        double r2 = dx * dx;
        if (d > 1) {
          const double dy = xi1 - xl[KC_JC + jj];
          r2 = fma(dy, dy, r2);
        }
        if (d > 2) {
          const double dz = xi2 - xl[2 * KC_JC + jj];
          r2 = fma(dz, dz, r2);
        }
        const double v = kcov_entry(P, r2, gd == gj);
        return (iv && gj < N) ? v : 0.0;
      };
      double a_next = eval(0);
      for (int s = 0; s < nslab; ++s) {
        const double a = a_next;
        if (s + 1 < nslab) a_next = eval(s + 1);     // independent of the MFMAs below: issued beside them
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const double b = wl[(16 * t + lr) * KC_JCP + 4 * s + lk];
          acc[t] = MFMA_F64(a, b, acc[t]);
        }
      }
    }
    if constexpr (kcov_tight_registers<PT>) asm volatile("" : "+s"(ldy));
    // C/D layout of the f64 instruction: column lane & 15, rows (lane >> 4) + 4 r: the four lk-lanes of a column write 32 contiguous bytes
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = 16 * t + lr;
      if (col < ncols) {
        double* yc = Y + (int64_t)col * ldy;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = row0 + lk + 4 * r;
          if (row < M) yc[row] = accumulate ? yc[row] + acc[t][r] : acc[t][r];
        }
      }
    }
  }
}

template <int NT, class PT>
static int kcov_launch(hfmi_ctx* ctx, const PT& P, int64_t M, const double* W, int64_t ldw, double* Y, int64_t ldy, int ncols, int accumulate) {
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_kcov<NT, PT>, 64 * KC_WAVES, 0));
  if (per_cu < 1) per_cu = 1;
  const int64_t ntiles = (M + KC_ROWS - 1) / KC_ROWS;
  const int64_t grid = std::min<int64_t>(ntiles, (int64_t)per_cu * ctx->num_cus);
  hipLaunchKernelGGL((k_kcov<NT, PT>), dim3((unsigned)grid), dim3(64 * KC_WAVES), 0, ctx->stream, P, W, ldw, Y, ldy, ncols, accumulate);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

int kcov_params_init(kcov_params* out, const double* x, int64_t N, int d, int family, double sigma, double ell, double nugget) {
  kcov_params P;
  P.x0 = x;
  P.x1 = d > 1 ? x + N : x;
  P.x2 = d > 2 ? x + 2 * N : x;
  P.N = N;
  P.d = d;
  P.inv_ell = 1.0 / ell;
  P.sigma2 = sigma * sigma;
  P.nugget = nugget;
  P.ca = 1.0, P.p1 = 0.0, P.p2 = 0.0, P.g1 = 1.0, P.g2 = 0.0;                      // Matern-1/2: exp(-a), a = r
  switch (family) {
    case HFMI_KERNEL_MATERN12: break;
    case HFMI_KERNEL_MATERN32: P.ca = 1.7320508075688772, P.p1 = 1.0; break;        // (1 + a) exp(-a), a = sqrt(3) r
    case HFMI_KERNEL_MATERN52: P.ca = 2.23606797749979, P.p1 = 1.0, P.p2 = 1.0 / 3.0; break;   // (1 + a + a^2/3) exp(-a), a = sqrt(5) r
    case HFMI_KERNEL_SQEXP: P.g1 = 0.0, P.g2 = 0.5; break;                           // exp(-r^2 / 2)
    case HFMI_KERNEL_MATERN1: P.ca = 1.4142135623730951; break;                      // a K_1(a), a = sqrt(2) r: the kcov_k1_* instances
    case HFMI_KERNEL_MATERN: break;                                                  // any nu: ca and the tables by kcov_nu_params_init_as
    default: HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov: unknown kernel family %d", family);
  }
  *out = P;
  return HFMI_OK;
}

// panels of at most 144 columns, one instance per number of column tiles
template <class PT>
static int kcov_panels(hfmi_ctx* ctx, const PT& P, int64_t M, const double* W, int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate) {
  for (int c0 = 0; c0 < nvec; c0 += 16 * KC_MAXT) {
    const int nc = std::min(16 * KC_MAXT, nvec - c0);
    const double* Wp = W + (int64_t)c0 * ldw;
    double* Yp = Y + (int64_t)c0 * ldy;
    switch ((nc + 15) / 16) {
      case 1: HFMI_TRY((kcov_launch<1, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 2: HFMI_TRY((kcov_launch<2, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 3: HFMI_TRY((kcov_launch<3, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 4: HFMI_TRY((kcov_launch<4, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 5: HFMI_TRY((kcov_launch<5, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 6: HFMI_TRY((kcov_launch<6, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 7: HFMI_TRY((kcov_launch<7, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      case 8: HFMI_TRY((kcov_launch<8, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
      default: HFMI_TRY((kcov_launch<9, PT>(ctx, P, M, Wp, ldw, Yp, ldy, nc, accumulate))); break;
    }
  }
  return HFMI_OK;
}

int launch_kernel_cov(hfmi_ctx* ctx, const double* x, int64_t N, int d, int family, double sigma, double ell, double nugget,
                      const double* W, int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate, const kcov_nu_ref& nu) {
  if (family == HFMI_KERNEL_MATERN) {
    kcov_nu_params P;
    HFMI_TRY(kcov_nu_params_init_as(&P, x, N, d, family, sigma, ell, nugget, nu));
    return kcov_panels(ctx, P, N, W, ldw, Y, ldy, nvec, accumulate);
  }
  if (family == HFMI_KERNEL_MATERN1) {
    kcov_k1_params P;
    HFMI_TRY(kcov_params_init_as(&P, x, N, d, family, sigma, ell, nugget));
    return kcov_panels(ctx, P, N, W, ldw, Y, ldy, nvec, accumulate);
  }
  kcov_params P;
  HFMI_TRY(kcov_params_init(&P, x, N, d, family, sigma, ell, nugget));
  return kcov_panels(ctx, P, N, W, ldw, Y, ldy, nvec, accumulate);
}

// the targets of the rectangular form, for either cross type
template <class PT>
static int kcov_cross_panels(hfmi_ctx* ctx, PT& P, const double* t, int64_t M, int64_t tstride, int64_t diag_offset, int d, const double* W,
                             int64_t ldw, double* Y, int64_t ldy, int nvec, int accumulate) {
  P.t0 = t;
  P.t1 = d > 1 ? t + tstride : t;
  P.t2 = d > 2 ? t + 2 * tstride : t;
  P.M = M;
  P.diag_offset = diag_offset >= 0 ? diag_offset : -1;
  return kcov_panels(ctx, P, M, W, ldw, Y, ldy, nvec, accumulate);
}

int launch_kernel_cross_cov(hfmi_ctx* ctx, const double* x, int64_t N, const double* t, int64_t M, int64_t tstride, int64_t diag_offset,
                            int d, int family, double sigma, double ell, double nugget, const double* W, int64_t ldw, double* Y,
                            int64_t ldy, int nvec, int accumulate, const kcov_nu_ref& nu) {
  if (M < 1) return HFMI_OK;      // an empty slab: no row of Y is this operator's
  if (diag_offset >= 0 && diag_offset + M > N)
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cross_cov: targets %lld .. %lld are not sources (N = %lld)", (long long)diag_offset,
              (long long)(diag_offset + M - 1), (long long)N);
  if (family == HFMI_KERNEL_MATERN) {
    kcov_nu_cross_params P;
    HFMI_TRY(kcov_nu_params_init_as(&P, x, N, d, family, sigma, ell, nugget, nu));
    return kcov_cross_panels(ctx, P, t, M, tstride, diag_offset, d, W, ldw, Y, ldy, nvec, accumulate);
  }
  if (family == HFMI_KERNEL_MATERN1) {
    kcov_k1_cross_params P;
    HFMI_TRY(kcov_params_init_as(&P, x, N, d, family, sigma, ell, nugget));
    return kcov_cross_panels(ctx, P, t, M, tstride, diag_offset, d, W, ldw, Y, ldy, nvec, accumulate);
  }
  kcov_cross_params P;
  HFMI_TRY(kcov_params_init(&P, x, N, d, family, sigma, ell, nugget));
  return kcov_cross_panels(ctx, P, t, M, tstride, diag_offset, d, W, ldw, Y, ldy, nvec, accumulate);
}
