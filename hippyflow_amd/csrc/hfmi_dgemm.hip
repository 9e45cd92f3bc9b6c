// General fp64 MFMA product C = alpha (op(A) op(B) + op(A2) op(B2)) + beta C, column-major, for every subsystem that needs one: the
// whole-GPU eigensolver (hfmi_eig_blocked.hip: rank-2k updates, merges, block reflectors) and, through the transposition identity
// and the triangular cuts, the wide Cholesky (hfmi_chol_wide.hip).  launch_dgemm (hfmi_dgemm.h) is the only way in.
#include <stdint.h>
#include <stdlib.h>

#include "hfmi_dgemm.h"
#include "hfmi_gemm_common.h"

namespace {
constexpr int GT = 64;             // k_dgemm: C tile
constexpr int GK = 16;             // reduction depth of an LDS stage
constexpr int GLD = 80;            // LDS row stride: = 16 mod 32 doubles, so the four k-rows of an MFMA operand fall into two bank halves

// ------------------------------------------------------------------------------------------------ fp64 MFMA GEMM
// element (t, k) of an operand tile, t = the operand's OWN index (row of op(A) / column of op(B)), for thread tid, slot u of 4
template <bool KC>
__device__ __forceinline__ void tile_idx(int tid, int u, int& t, int& k) {
  if (KC) {           // the reduction index is the contiguous one in memory
    k = tid & 15;
    t = (tid >> 4) + 16 * u;
  } else {            // the operand's own index is contiguous
    t = tid & 63;
    k = (tid >> 6) + 4 * u;
  }
}
template <bool KC>
__device__ __forceinline__ void tile_load(const double* __restrict__ X, int64_t ld, int t0, int k0, int Tdim, int Kdim, int tid,
                                          double (&r)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int t, k;
    tile_idx<KC>(tid, u, t, k);
    const bool ok = t0 + t < Tdim && k0 + k < Kdim;
    const int64_t off = KC ? (int64_t)(k0 + k) + (int64_t)(t0 + t) * ld : (int64_t)(t0 + t) + (int64_t)(k0 + k) * ld;
    r[u] = ok ? X[off] : 0.0;
  }
}
template <bool KC>
__device__ __forceinline__ void tile_store(double (*s)[GLD], int tid, const double (&r)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int t, k;
    tile_idx<KC>(tid, u, t, k);
    s[k][t] = r[u];
  }
}
// C (M x N) = alpha (op(A) op(B) + op(A2) op(B2)) + beta C, everything column-major.  op(A) = A (M x K, lda) or A^T (A is K x M);
// op(B) = B (K x N) or B^T (B is N x K); the second product (K2 columns, same shapes and leading dimensions) is optional
// (K2 = 0) -- it makes the symmetric rank-2k update one pass over C.  blockIdx.z = batch index (element strides sA, sB, sC).
// 64 x 64 tile per workgroup, 4 waves of 32 x 32 (2 x 2 MFMA 16x16x4 tiles), operands staged k-major through two LDS buffers.
// The MFMA's first operand carries the N index, the second the M index: the accumulator then holds 16 consecutive rows of a
// column per register, and the stores of C are 128-byte runs.
// CUT: triangular operands (gemm_desc::cut, one product only) and the skip flag; without it neither argument is looked at.
template <bool TA, bool TB, bool CUT>
__global__ __launch_bounds__(256) void k_dgemm(int M, int N, int K, double alpha, const double* __restrict__ A, int64_t lda,
                                               const double* __restrict__ B, int64_t ldb, int K2, const double* __restrict__ A2,
                                               const double* __restrict__ B2, double beta, double* __restrict__ C, int64_t ldc,
                                               int64_t sA, int64_t sB, int64_t sC, int cut, const int* __restrict__ skip) {
  __shared__ double s_a[2][GK][GLD], s_b[2][GK][GLD];
  if (CUT && skip && skip[0]) return;
  if (CUT && (cut & 1) && blockIdx.y > blockIdx.x) return;
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, li = l & 15, lk = l >> 4;
  const int wm = w & 1, wn = w >> 1;
  const int i0 = blockIdx.x * GT, j0 = blockIdx.y * GT;
  A += (int64_t)blockIdx.z * sA;
  B += (int64_t)blockIdx.z * sB;
  C += (int64_t)blockIdx.z * sC;
  // the reduction range of this tile's first product
  const int klo = (CUT && (cut & 4)) ? min(K, (int)blockIdx.y * GT) : 0;
  const int khi = (CUT && (cut & 2)) ? min(K, ((int)blockIdx.x + 1) * GT) : K;
  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};
  const int nk1 = (CUT && khi <= klo) ? 0 : (khi - klo + GK - 1) / GK, nk2 = CUT ? 0 : (K2 + GK - 1) / GK, nk = nk1 + nk2;
  double ra[4], rb[4];
  auto gload = [&](int kt) {
    const bool second = kt >= nk1;
    const double* Ap = second ? A2 : A;
    const double* Bp = second ? B2 : B;
    const int Kc = second ? K2 : khi, k0 = second ? (kt - nk1) * GK : klo + kt * GK;
    tile_load<TA>(Ap, lda, i0, k0, M, Kc, tid, ra);
    tile_load<!TB>(Bp, ldb, j0, k0, N, Kc, tid, rb);
  };
  if (nk > 0) {
    gload(0);
    tile_store<TA>(s_a[0], tid, ra);
    tile_store<!TB>(s_b[0], tid, rb);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int k4 = 0; k4 < GK / 4; ++k4) {
      double af[2], bf[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) af[mi] = s_a[buf][k4 * 4 + lk][wm * 32 + mi * 16 + li];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) bf[ni] = s_b[buf][k4 * 4 + lk][wn * 32 + ni * 16 + li];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = MFMA_F64(bf[ni], af[mi], acc[mi][ni]);
    }
    if (kt + 1 < nk) {
      tile_store<TA>(s_a[buf ^ 1], tid, ra);
      tile_store<!TB>(s_b[buf ^ 1], tid, rb);
    }
    __syncthreads();
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = i0 + wm * 32 + mi * 16 + li, j = j0 + wn * 32 + ni * 16 + lk + 4 * reg;
        if (i < M && j < N) {
          double* cp = C + (int64_t)i + (int64_t)j * ldc;
          double v = alpha * acc[mi][ni][reg];
          if (beta != 0.0) v = fma(beta, *cp, v);
          *cp = v;
        }
      }
}

// ------------------------------------------------------------------------------------------------ fp64 MFMA GEMM, software-pipelined
// The same contract as k_dgemm for the large products (trailing rank-2k updates, Q S of the upper merges, the block reflectors of
// the back-transformation), built for the MFMA pipe to stay busy:
//   * workgroup tile BM x 128 (BM = 128 | 64), 4 waves of (BM / 2) x 64: 4 x 4 (2 x 4) accumulator tiles per wave, so a reduction
//     step of 4 costs 4 + 4 (2 + 4) eight-byte LDS reads for 16 (8) MFMAs of 64 cycles each;
//   * the operand fragments of step k + 1 are read into a second register set while the MFMAs of step k issue (register double
//     buffering: the 128 x 128 variant of round 5 read its fragments right before their use and lost to the 64 x 64 one);
//   * the next 16-deep slab of both operands travels global -> registers (16-byte loads) during the whole slab, and is written to
//     the other LDS buffer after the last MFMA: one barrier per 64 (32) MFMAs of a wave;
//   * LDS layout by the operand's memory layout, both conflict-free for the 16-byte stores and the 8-byte fragment reads:
//       own index contiguous in memory -> k-major rows of BT + 16 doubles (= 16 mod 32: the four k-rows of a fragment fall into
//       two bank halves), reduction index contiguous -> own-index-major rows of 18 doubles (36 li mod 64 are 16 distinct multiples
//       of 4: a fragment's 16 rows x 2 columns cover the 64 banks exactly once).
// 16-byte loads need 16-byte aligned operands (even offsets and leading dimensions): `vec` says so, else 8-byte loads.
constexpr int PK = 16;              // reduction depth of an LDS stage
constexpr int PS_KC = 18;           // row stride (doubles) of a stage whose rows are the operand's own index
template <bool KC, int BT>
struct pstage {
  static constexpr int ND2 = BT * PK / 2 / 256;            // 16-byte pieces per thread
  static constexpr int LDK = BT + 16;                      // k-major row stride
  static constexpr int DOUBLES = KC ? BT * PS_KC : PK * LDK;
  // piece u of thread tid: own index t (pair t, t + 1 if !KC), reduction index k (pair k, k + 1 if KC)
  static __device__ __forceinline__ void idx(int tid, int u, int& t, int& k) {
    if (KC) {
      k = 2 * (tid & 7);
      t = (tid >> 3) + 32 * u;
    } else {
      t = 2 * (tid & (BT / 2 - 1));
      k = tid / (BT / 2) + (512 / BT) * u;
    }
  }
  // FAST: the whole slab lies inside the operand and is 16-byte aligned -- plain 16-byte loads, no predicate.  Otherwise 8-byte loads
  // from clamped (always valid) addresses and a select: no lane-divergent branch in either form (a predicated load that shares
  // its destination with another load makes the compiler wait for the first one: eight serialised round trips per slab).
  template <bool FAST>
  static __device__ __forceinline__ void load(const double* __restrict__ X, int64_t ld, int t0, int k0, int Tdim, int Kdim, int tid,
                                              d2 (&r)[ND2], unsigned& valid) {
    valid = ~0u;
#pragma unroll
    for (int u = 0; u < ND2; ++u) {
      int t, k;
      idx(tid, u, t, k);
      const int tt = t0 + t, kk = k0 + k;
      if (FAST) {
        const int64_t off = KC ? (int64_t)kk + (int64_t)tt * ld : (int64_t)tt + (int64_t)kk * ld;
        r[u] = *(const d2*)(X + off);
      } else {
        const int tt1 = KC ? tt : tt + 1, kk1 = KC ? kk + 1 : kk;
        const bool ok0 = tt < Tdim && kk < Kdim, ok1 = tt1 < Tdim && kk1 < Kdim;
        const int tc0 = min(tt, Tdim - 1), kc0 = min(kk, Kdim - 1), tc1 = min(tt1, Tdim - 1), kc1 = min(kk1, Kdim - 1);
        r[u].x = X[KC ? (int64_t)kc0 + (int64_t)tc0 * ld : (int64_t)tc0 + (int64_t)kc0 * ld];
        r[u].y = X[KC ? (int64_t)kc1 + (int64_t)tc1 * ld : (int64_t)tc1 + (int64_t)kc1 * ld];
        if (!ok0) valid &= ~(1u << (2 * u));
        if (!ok1) valid &= ~(2u << (2 * u));
      }
    }
  }
  // (the zeroing of out-of-range entries happens here, after the MFMAs of the slab that hid the loads)
  static __device__ __forceinline__ void store(double* __restrict__ s, int tid, const d2 (&r)[ND2], unsigned valid) {
#pragma unroll
    for (int u = 0; u < ND2; ++u) {
      int t, k;
      idx(tid, u, t, k);
      d2 v = r[u];
      if (!((valid >> (2 * u)) & 1u)) v.x = 0.0;
      if (!((valid >> (2 * u)) & 2u)) v.y = 0.0;
      if (KC) *(d2*)(s + t * PS_KC + k) = v;
      else *(d2*)(s + k * LDK + t) = v;
    }
  }
  // fragment element (own index t, reduction index k)
  static __device__ __forceinline__ double frag(const double* __restrict__ s, int t, int k) { return KC ? s[t * PS_KC + k] : s[k * LDK + t]; }
};
template <bool TA, bool TB, int BM>
__global__ __launch_bounds__(256, 2) void k_dgemm_p(int M, int N, int K, double alpha, const double* __restrict__ A, int64_t lda,
                                                    const double* __restrict__ B, int64_t ldb, int K2, const double* __restrict__ A2,
                                                    const double* __restrict__ B2, double beta, double* __restrict__ C, int64_t ldc,
                                                    int64_t sA, int64_t sB, int64_t sC, int vec, int lower) {
  constexpr int BN = 128, MI = BM / 32, NI = 4;
  typedef pstage<TA, BM> SA;          // op(A) = A^T: the reduction index is the contiguous one
  typedef pstage<!TB, BN> SB;
  extern __shared__ __attribute__((aligned(16))) double s_p[];
  auto s_a = [&](int b) { return s_p + b * SA::DOUBLES; };
  auto s_b = [&](int b) { return s_p + 2 * SA::DOUBLES + b * SB::DOUBLES; };
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, li = l & 15, lk = l >> 4;
  const int wm = w & 1, wn = w >> 1;
  const int i0 = blockIdx.x * BM, j0 = blockIdx.y * BN;
  // symmetric update, lower part only: `lower` - 1 is the position of C's first row / column inside its 128 x 128 block of the matrix;
  // a tile is skipped when it lies entirely above the diagonal 128-blocks (the lower-triangle products read those blocks whole)
  if (lower && ((i0 + lower - 1 + BM - 1) >> 7) < ((j0 + lower - 1) >> 7)) return;
  A += (int64_t)blockIdx.z * sA;
  B += (int64_t)blockIdx.z * sB;
  C += (int64_t)blockIdx.z * sC;
  if (K2 > 0) {
    A2 += (int64_t)blockIdx.z * sA;
    B2 += (int64_t)blockIdx.z * sB;
  }
  d4 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};
  const int nk1 = (K + PK - 1) / PK, nk2 = (K2 + PK - 1) / PK, nk = nk1 + nk2;
  d2 ra[SA::ND2], rb[SB::ND2];
  unsigned va = ~0u, vb = ~0u;
  const bool inside = vec && i0 + BM <= M && j0 + BN <= N;      // workgroup-uniform
  auto gload = [&](int kt) {
    const bool second = kt >= nk1;
    const double* Ap = second ? A2 : A;
    const double* Bp = second ? B2 : B;
    const int Kc = second ? K2 : K, k0 = (second ? kt - nk1 : kt) * PK;
    if (inside && k0 + PK <= Kc) {
      SA::template load<true>(Ap, lda, i0, k0, M, Kc, tid, ra, va);
      SB::template load<true>(Bp, ldb, j0, k0, N, Kc, tid, rb, vb);
    } else {
      SA::template load<false>(Ap, lda, i0, k0, M, Kc, tid, ra, va);
      SB::template load<false>(Bp, ldb, j0, k0, N, Kc, tid, rb, vb);
    }
  };
  if (nk > 0) {
    gload(0);
    SA::store(s_a(0), tid, ra, va);
    SB::store(s_b(0), tid, rb, vb);
  }
  __syncthreads();
  const int ta0 = wm * (BM / 2) + li, tb0 = wn * 64 + li;
  for (int kt = 0; kt < nk; ++kt) {
    const double* __restrict__ pa = s_a(kt & 1);
    const double* __restrict__ pb = s_b(kt & 1);
    if (kt + 1 < nk) gload(kt + 1);
    double fa[2][MI], fb[2][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) fa[0][mi] = SA::frag(pa, ta0 + 16 * mi, lk);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) fb[0][ni] = SB::frag(pb, tb0 + 16 * ni, lk);
#pragma unroll
    for (int k4 = 0; k4 < PK / 4; ++k4) {
      const int cur = k4 & 1, nxt = cur ^ 1;
      if (k4 + 1 < PK / 4) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) fa[nxt][mi] = SA::frag(pa, ta0 + 16 * mi, 4 * (k4 + 1) + lk);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) fb[nxt][ni] = SB::frag(pb, tb0 + 16 * ni, 4 * (k4 + 1) + lk);
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = MFMA_F64(fb[cur][ni], fa[cur][mi], acc[mi][ni]);
    }
    if (kt + 1 < nk) {
      SA::store(s_a((kt + 1) & 1), tid, ra, va);
      SB::store(s_b((kt + 1) & 1), tid, rb, vb);
    }
    __syncthreads();
  }
  // epilogue: lane (li, lk), register reg of tile (mi, ni) holds C[i0 + wm BM/2 + 16 mi + li, j0 + wn 64 + 16 ni + lk + 4 reg].
  // beta != 0: the old values are fetched two column tiles at a time -- 8 MI loads per lane in flight (from clamped, always valid
  // addresses: no predicate on a load), then the same number of stores -- two round trips per tile instead of one per column
  const int ib = i0 + wm * (BM / 2) + li, jb = j0 + wn * 64 + lk;
#pragma unroll
  for (int nh = 0; nh < NI; nh += 2) {
    double old[2][4][MI];
    if (beta != 0.0) {
#pragma unroll
      for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int i = min(ib + 16 * mi, M - 1), j = min(jb + 16 * (nh + n2) + 4 * reg, N - 1);
            old[n2][reg][mi] = C[(int64_t)i + (int64_t)j * ldc];
          }
    }
#pragma unroll
    for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int i = ib + 16 * mi, j = jb + 16 * (nh + n2) + 4 * reg;
          double v = alpha * acc[mi][nh + n2][reg];
          if (beta != 0.0) v = fma(beta, old[n2][reg][mi], v);
          if (i < M && j < N) C[(int64_t)i + (int64_t)j * ldc] = v;
        }
  }
}

template <bool TA, bool TB, int BM>
int launch_dgemm_p(hfmi_ctx* ctx, const gemm_desc& g, const gemm_route& r) {
  typedef pstage<TA, BM> SA;
  typedef pstage<!TB, 128> SB;
  const size_t lds = (size_t)2 * (SA::DOUBLES + SB::DOUBLES) * sizeof(double);
  static bool attr_set = false;       // (one flag per instantiation)
  if (!attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void*)k_dgemm_p<TA, TB, BM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  const dim3 grid(r.gx, r.gy, r.gz), block(256);
  hipLaunchKernelGGL((k_dgemm_p<TA, TB, BM>), grid, block, lds, ctx->stream, g.M, g.N, g.K, g.alpha, g.A, g.lda, g.B, g.ldb, g.K2, g.A2, g.B2,
                     g.beta, g.C, g.ldc, g.sA, g.sB, g.sC, r.vec, g.lower);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
}  // namespace

int dgemm_pipelined_switch() {
  static const int pipelined = [] {      // HFMI_EIG_GEMM = 0: the 64 x 64 kernel of round 5 everywhere (A/B)
    const char* e = getenv("HFMI_EIG_GEMM");
    return e ? atoi(e) : 1;
  }();
  return pipelined;
}

// The decision is dgemm_route_make's (hfmi_dgemm.h); this launches what it says.
int launch_dgemm(hfmi_ctx* ctx, const gemm_desc& g) {
  const gemm_route r = dgemm_route_make(g, dgemm_pipelined_switch());
  if (r.error == HFMI_DGEMM_ERR_K2_BATCH) HFMI_FAIL(HFMI_ERR_INVALID, "dgemm: a second product (K2=%d) takes no batch (%d)", g.K2, g.batch);
  if (r.error == HFMI_DGEMM_ERR_CUT) HFMI_FAIL(HFMI_ERR_INVALID, "dgemm: a cut product takes one untransposed A (ta=%d, K2=%d)", (int)g.ta, g.K2);
  if (r.kernel == HFMI_DGEMM_NONE) return HFMI_OK;
  if (r.kernel == HFMI_DGEMM_P128 || r.kernel == HFMI_DGEMM_P64) {
    const bool big = r.kernel == HFMI_DGEMM_P128;
#define EB_GEMM_P(TAV, TBV) (big ? launch_dgemm_p<TAV, TBV, 128>(ctx, g, r) : launch_dgemm_p<TAV, TBV, 64>(ctx, g, r))
    if (!g.ta && !g.tb) return EB_GEMM_P(false, false);
    if (g.ta && !g.tb) return EB_GEMM_P(true, false);
    if (!g.ta && g.tb) return EB_GEMM_P(false, true);
    return EB_GEMM_P(true, true);
#undef EB_GEMM_P
  }
  const bool cut = r.kernel == HFMI_DGEMM_K64_CUT;
  const dim3 grid(r.gx, r.gy, r.gz), block(256);
#define EB_GEMM(TAV, TBV, CUTV)                                                                                                           \
  hipLaunchKernelGGL((k_dgemm<TAV, TBV, CUTV>), grid, block, 0, ctx->stream, g.M, g.N, g.K, g.alpha, g.A, g.lda, g.B, g.ldb, g.K2, g.A2, \
                     g.B2, g.beta, g.C, g.ldc, g.sA, g.sB, g.sC, g.cut, g.skip)
  if (cut && g.tb) EB_GEMM(false, true, true);
  else if (cut) EB_GEMM(false, false, true);
  else if (!g.ta && !g.tb) EB_GEMM(false, false, false);
  else if (g.ta && !g.tb) EB_GEMM(true, false, false);
  else if (!g.ta && g.tb) EB_GEMM(false, true, false);
  else EB_GEMM(true, true, false);
#undef EB_GEMM
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// instrumentation: C (M x N) = op(A) op(B) through launch_dgemm (the products of the eigensolver), host operands column-major with
// their natural leading dimensions (A: ta ? K x M : M x K; B: tb ? N x K : K x N); average time of `reps` launches after one warm-up
int eig_dgemm_bench(hfmi_ctx* ctx, int M, int N, int K, int ta, int tb, int reps, const double* host_A, const double* host_B,
                    double* host_C, double* avg_ms) {
  const int64_t ra = ta ? K : M, ca = ta ? M : K, rb = tb ? N : K, cb = tb ? K : N;
  const int64_t lda = round_up(ra, 2), ldb = round_up(rb, 2), ldc = round_up(M, 2);
  void* wv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)(lda * ca + ldb * cb + ldc * N) * sizeof(double), &wv));
  double *A = (double*)wv, *B = A + lda * ca, *C = B + ldb * cb;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpy2DAsync(A, lda * sizeof(double), host_A, ra * sizeof(double), ra * sizeof(double), ca, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpy2DAsync(B, ldb * sizeof(double), host_B, rb * sizeof(double), rb * sizeof(double), cb, hipMemcpyHostToDevice, st));
  gemm_desc g;
  g.ta = ta != 0;
  g.tb = tb != 0;
  g.M = M;
  g.N = N;
  g.K = K;
  g.alpha = 1.0;
  g.beta = 0.0;
  g.A = A;
  g.B = B;
  g.lda = lda;
  g.ldb = ldb;
  g.C = C;
  g.ldc = ldc;
  HFMI_TRY(launch_dgemm(ctx, g));
  HIP_TRY(hipEventRecord(ctx->ev0, st));
  for (int r = 0; r < reps; ++r) HFMI_TRY(launch_dgemm(ctx, g));
  HIP_TRY(hipEventRecord(ctx->ev1, st));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  if (avg_ms) *avg_ms = reps > 0 ? ms / reps : 0.0;
  if (host_C) {
    HIP_TRY(hipMemcpy2DAsync(host_C, (size_t)M * sizeof(double), C, ldc * sizeof(double), (size_t)M * sizeof(double), N, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return HFMI_OK;
}
