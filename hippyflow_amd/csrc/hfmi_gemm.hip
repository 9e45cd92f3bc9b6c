// FP64 tall-skinny contractions on gfx950 matrix cores (v_mfma_f64_16x16x4_f64).
//
// Two shapes carry every operator application, Gram matrix and back-transform on the
// double-pass path (DESIGN.md section "kernels"):
//
//   tsgemm_tn :  C (m x k)  = A^T B     A: N x m, B: N x k   -- reduction over the long axis N
//                (X W in the snapshot-Gram / Jacobian-Gram apply, Q^T B Q, (AQ)^T Q, C W)
//   tsgemm_nn :  Y (N x r)  = A S       A: N x m, S: m x r   -- long axis preserved
//                (X^T G, Q R^{-1}, U = Q V)
//
// All blocks are column-major with every vector contiguous along N, so in tsgemm_tn BOTH
// operands are contiguous along the reduction index: an MFMA k-step may use any 4 reduction
// indices as long as A and B agree, which lets each lane fetch 16 or 32 contiguous bytes of its own
// vector straight from HBM into the fragment layout -- no transposition through LDS.  The operand
// shared by the waves of a workgroup (B in tn, S in nn) is staged through LDS; the streamed
// operand goes HBM -> VGPR directly, prefetched one iteration ahead.  A wave holds a
// (16*MT) x (16*NT) fp64 accumulator tile: up to 16 MFMA tiles with two waves per SIMD (the default),
// up to 32 with one.  A last column tile of at most 12 columns runs on the 4x4x4 MFMA (R4).
// tsgemm_nn lives in hfmi_gemm_nn.hip, the skinny x skinny case of tn in hfmi_skinny.hip.
//
// MFMA fragment maps (cdna_hip_programming.md section 3): lane l supplies A[i = l&15][kk = l>>4] and
// B[kk = l>>4][j = l&15]; it receives D[row = (l>>4) + 4*reg][col = l&15], reg = 0..3.
#include "hfmi_gemm_common.h"

// =====================================================================================
// tsgemm_tn
// =====================================================================================
// the streamed operand is read once by one workgroup: -DHFMI_TN_NT marks its loads non-temporal (A/B build, scripts/build_variant.sh)
#ifdef HFMI_TN_NT
#define TN_LOAD_A(p) __builtin_nontemporal_load(p)
#else
#define TN_LOAD_A(p) (*(p))
#endif
// the finely split tail of a launch (see the block mapping in k_tsgemm_tn); nrb = 0: none
struct TnTail {
  int nrb, nsplit;
  int64_t chunk;
  double* out;
  int64_t si, sj, sps;
};

// Preconditions (guaranteed by the block layout, hfmi.h): lda, ldb multiples of 32 doubles, rows N..ld-1 of
// every vector are zero, so the reduction runs over whole 32-row stages with NO masks or branches in the loop:
// every load below is unconditional (clamped addresses), which is what lets the prefetches stay in flight.
//
// WAVES = 4: one wave per SIMD with up to 32 accumulator tiles (256 AGPRs).  WAVES = 8: two waves per SIMD with
// up to 16 tiles each -- same workgroup tile, but while one wave of a SIMD sits in a barrier / LDS / HBM wait the
// other keeps the matrix pipe busy.
// R4 > 0: the LAST of the NT column tiles holds at most 4 R4 real columns and is computed with R4
// v_mfma_f64_4x4x4_4b instructions (16 cycles each, four 4x4x4 blocks = the four 4-row groups of a 16-row tile)
// instead of one 16x16x4 (64 cycles): k = 84 costs 5 x 64 + 16 cycles per k-step instead of 6 x 64, k = 74
// 4 x 64 + 48 instead of 5 x 64.  Lane layout of the 4x4x4 instruction (scripts/mfma4x4_probe.hip): A lane
// 16 k + 4 g + i = A_g[i][k], B lane 16 k + 4 g + j = B_g[k][j], D lane 16 i + 4 g + j = D_g[i][j] -- so the 16x16x4
// A fragment (lane (row & 15, k)) already IS the 4x4x4 A operand with block g = rows 4g..4g+3, and B only has to be
// read from LDS with the 4 columns of a group repeated for every block.
template <int MT, int NT, bool TR, int WAVES, int R4>
__global__ __launch_bounds__(WAVES * 64, (WAVES == 8 || MT * NT <= 20) ? 2 : 1) void k_tsgemm_tn(const double* __restrict__ A, int64_t lda, int m,
                                                                    const double* B /* not restrict: see the stage loop */, int64_t ldb, int k,
                                                                    int64_t Npad, int64_t chunk, int nrb, int nsplit,
                                                                    double* __restrict__ out, int64_t si, int64_t sj,
                                                                    int64_t sps, int direct, int probe_arg, TnTail tail) {
  // timing-only diagnostic (scripts/tn_probe.py; results are garbage): compiled in only with -DHFMI_TN_PROBE
  // (HFMI_EXTRA_HIPCC_FLAGS), the production instance carries no run-time branch for it
#ifdef HFMI_TN_PROBE
  const int probe = probe_arg;
#else
  constexpr int probe = 0;
  (void)probe_arg;
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BK = TN_BK;
  constexpr int COLS = NT * 16;
  constexpr int LDB = BK + 2;
  constexpr int BUFD = COLS * LDB;                // doubles per stage buffer
  constexpr int CSH = 4;                          // log2(16-byte chunks per column per stage)
  constexpr int NTF = R4 > 0 ? NT - 1 : NT;       // full 16-column tiles
  constexpr int NR4 = R4 > 0 ? R4 : 1;
  constexpr int NTHR = WAVES * 64;
  constexpr int CH = COLS * (BK / 2);             // 16-byte chunks per stage
  constexpr int NQ = (CH + NTHR - 1) / NTHR;      // chunks per thread
  // AH = 2: one iteration is 16 reduction indices and every lane fetches 32 contiguous bytes of its vector (see
  // load_a); taken where the VGPR estimate leaves room for the 8 MT extra registers, else 8 indices / 16 bytes
  constexpr int EST = MT * NTF * 8 + MT * R4 * 2 + NTF * 4 + R4 * 4 + 16 * MT + NQ * 6;
  constexpr int AH = (EST <= ((WAVES == 8 || MT * NT <= 20) ? 218 : 470)) ? 2 : 1;
  double* lds = reinterpret_cast<double*>(smem);  // [2][NT*16][LDB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kk = lane >> 4;

  // Row blocks [0, nrb) are whole rounds of the CUs, each split nsplit ways over the reduction axis; the tail.nrb row blocks
  // behind them (fewer than one round: m = 1e5 is 261 blocks of 384 rows on 256 CUs) are split tail.nsplit ways -- as finely as
  // it takes to fill one more round of workgroups for 1 / tail.nsplit of a block's time -- and write to their own, compact
  // partial buffer.  The two groups are remapped over the XCDs separately (see k_tsgemm_nn).
  const int nfull = nrb * nsplit;
  const bool in_tail = (int)blockIdx.x >= nfull;
  const int logical = in_tail ? xcd_remap((int)blockIdx.x - nfull, tail.nrb * tail.nsplit) : xcd_remap(blockIdx.x, nfull);
  const int sp = in_tail ? logical / tail.nrb : logical / nrb;
  const int rb = in_tail ? nrb + logical % tail.nrb : logical % nrb;
  if (in_tail) {
    chunk = tail.chunk;
    out = tail.out;
    si = tail.si;
    sj = tail.sj;
    sps = tail.sps;
    direct = 0;
  }
  const int row_off = in_tail ? nrb * (16 * MT * WAVES) : 0;   // the tail's partial buffer starts at its first row
  const int64_t t_begin = (int64_t)sp * chunk;
  int64_t t_end = t_begin + chunk;
  if (t_end > Npad) t_end = Npad;
  const int nstages = (int)((t_end - t_begin) / BK);
  const int64_t t_last = t_end - 8 * AH;  // last iteration base that is safe to fetch
  const int rowbase = rb * (16 * MT * WAVES) + wave * (16 * MT);

  const double* a_ptr[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    int row = rowbase + mt * 16 + r16;
    if (row > m - 1) row = m - 1;
    a_ptr[mt] = A + (int64_t)row * lda + kk * 2 * AH;
  }
  const double* b_ptr[NQ];
#pragma unroll
  for (int qd = 0; qd < NQ; ++qd) {
    int c = tid + NTHR * qd;
    if (c > CH - 1) c = CH - 1;
    int col = c >> CSH;
    if (col > k - 1) col = k - 1;
    b_ptr[qd] = B + (int64_t)col * ldb + (c & ((1 << CSH) - 1)) * 2;
  }

  constexpr int NTA = NTF > 0 ? NTF : 1;
  d4 acc[MT][NTA];
  double acc4[MT][NR4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int nt = 0; nt < NTA; ++nt) acc[mt][nt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < NR4; ++q) acc4[mt][q] = 0.0;
  }

  d2 breg[NQ];
  auto stage_load = [&](int64_t ts) {
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) breg[qd] = *reinterpret_cast<const d2*>(b_ptr[qd] + ts);
  };
  auto stage_store = [&](double* L) {
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) {
      const int c = tid + NTHR * qd;
      const int col = c >> CSH, q = c & ((1 << CSH) - 1);
      const int off = col * LDB + q * 2;
      if (CH % NTHR == 0 || c < CH) *reinterpret_cast<d2*>(L + off) = breg[qd];
    }
  };
  // AH = 2: one iteration = 16 reduction indices; lane (r16, kk) fetches the 32 contiguous bytes t + 4 kk .. t + 4 kk + 3
  // of vector r16 as two 16-byte loads issued back to back, so the four kk lanes cover a whole 128-byte line of every
  // vector at once (HBM delivers 128-byte runs at 6.3-6.7 TB/s, 64-byte runs at 3.5-3.9 TB/s: scripts/stream_probe2.hip).
  // Any assignment of reduction indices to (lane, k-step) is legal as long as the LDS fragments of B use the same one:
  // half h of the iteration covers indices t + 2 AH kk + 2 h + {0, 1}.
  auto load_a = [&](d2(&dst)[AH][MT], int64_t t) {
    if (t > t_last) t = t_last;  // wave-uniform clamp: prefetches past the end re-read valid data
    if (probe & 1) t = t_begin;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < AH; ++h) dst[h][mt] = TN_LOAD_A(reinterpret_cast<const d2*>(a_ptr[mt] + t + 2 * h));
  };
  // Full tiles: lane (r16, kk) reads column nt*16 + r16.  The fragments are SINGLE-buffered: the moment the MFMAs
  // of column tile nt have been issued, its registers are refilled with the next iteration's fragment, and the MFMAs of
  // the other column tiles cover the LDS latency (the sched_barriers pin that order; left alone the scheduler hoists
  // all reads to the top, which is the double-buffered register budget again -- 4 NT VGPRs more).  The 4-column groups
  // of the last tile (lane -> column NTF*16 + 4 q + (lane & 3), the same for every row group) are read at the top of
  // their own iteration; the full-tile MFMAs in front of them cover the latency.
  d2 bf[NTA];
  // `it` counts half iterations (8 reduction indices): offset of this lane's two indices inside the stage
  auto koff = [&](int it) { return (it / AH) * (8 * AH) + kk * (2 * AH) + (it % AH) * 2; };
  auto ldsb1 = [&](const double* L, int it, int nt) {
    bf[nt] = *reinterpret_cast<const d2*>(L + (nt * 16 + r16) * LDB + koff(it));
  };
  auto mma = [&](const d2(&a)[MT], const double* L, int it, bool refill) {
    d2 bg[NR4];
    if constexpr (R4 > 0) {
#pragma unroll
      for (int q = 0; q < R4; ++q)
        bg[q] = *reinterpret_cast<const d2*>(L + (NTF * 16 + 4 * q + (lane & 3)) * LDB + koff(it));
    }
#pragma unroll
    for (int nt = 0; nt < NTF; ++nt) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt][nt] = TR ? MFMA_F64(bf[nt].x, a[mt].x, acc[mt][nt]) : MFMA_F64(a[mt].x, bf[nt].x, acc[mt][nt]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt][nt] = TR ? MFMA_F64(bf[nt].y, a[mt].y, acc[mt][nt]) : MFMA_F64(a[mt].y, bf[nt].y, acc[mt][nt]);
      if (refill) ldsb1(L, it + 1, nt);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (R4 > 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < R4; ++q) acc4[mt][q] = MFMA_F64_4(a[mt].x, bg[q].x, acc4[mt][q]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < R4; ++q) acc4[mt][q] = MFMA_F64_4(a[mt].y, bg[q].y, acc4[mt][q]);
    }
    // keep the scheduler from hoisting later iterations' loads above these MFMAs
    // (it would otherwise blow the register budget and spill the accumulators)
    __builtin_amdgcn_sched_barrier(0);
  };

  if (nstages > 0) {
    stage_load(t_begin);
    stage_store(lds);
    __syncthreads();
  }
  // streamed operand: two register buffers over iterations of 8 AH reduction indices (prefetch distance one iteration;
  // a ring of 4 x 8 indices at distance 3 measured no faster on any shape -- latency is not what limits the kernel)
  {
    constexpr int NIT = BK / (8 * AH), NH = BK / 8;
    d2 a[2][AH][MT];
    load_a(a[0], t_begin);
    for (int s = 0; s < nstages; ++s) {
      const int64_t ts = t_begin + (int64_t)s * BK;
      const bool has_next = s + 1 < nstages;
      // UNCONDITIONAL (the last stage re-reads its own slab): vmcnt retires loads in issue order, and these loads sit
      // between the streamed operand's fragment fetched one iteration ago and the wait in front of its first MFMA.  Behind
      // a branch (as it was until round 2) the compiler has to assume the path WITHOUT them at the join and emits
      // vmcnt(6) instead of vmcnt(6 + NQ): every stage then began by waiting for these loads' L2 / HBM round trip --
      // 10-12 % of the kernel (round-2 experiment builds, profiles/r02o_tn_variants.txt).
      stage_load(has_next ? ts + BK : ts);
      asm volatile("" ::: "memory");   // keeps the loads HERE: left alone they are sunk to their ds_write and waited for with vmcnt(0)
      const double* L = lds + (s & 1) * BUFD;
#pragma unroll
      for (int nt = 0; nt < NTF; ++nt) ldsb1(L, 0, nt);
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        load_a(a[(it + 1) & 1], ts + 8 * AH * (it + 1));
#pragma unroll
        for (int h = 0; h < AH; ++h) mma(a[it & 1][h], L, it * AH + h, it * AH + h + 1 < NH);
      }
      if (!(probe & 2)) {
      if (has_next) stage_store(lds + ((s + 1) & 1) * BUFD);
      __syncthreads();
      }
    }
  }

  // Results: element (i, j) goes to P[i si + j sj].  Split launches write raw partial tiles (padded image of split
  // sp, summed by k_reduce_partials); a launch with ONE split and nothing to scale or accumulate writes the result
  // block itself (direct: bounds-checked) -- config 2's m = 1e5 launches used to spend 0.28 ms copying one partial.
  double* P = out + (int64_t)sp * sps;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTF; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = TR ? rowbase + mt * 16 + r16 : rowbase + mt * 16 + kk + 4 * r;
        const int j = TR ? nt * 16 + kk + 4 * r : nt * 16 + r16;
        if (!direct || (i < m && j < k)) P[(int64_t)(i - row_off) * si + (int64_t)j * sj] = acc[mt][nt][r];
      }
  if constexpr (R4 > 0) {
    // 4x4x4 results: lane 16 i + 4 g + j holds (row 4 g + i of the tile, column 4 q + j of the last tile)
    const int i4 = lane >> 4, g4 = (lane >> 2) & 3, j4 = lane & 3;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < R4; ++q) {
        const int i = rowbase + mt * 16 + 4 * g4 + i4;
        const int j = NTF * 16 + 4 * q + j4;
        if (!direct || (i < m && j < k)) P[(int64_t)(i - row_off) * si + (int64_t)j * sj] = acc4[mt][q];
      }
  }
}

// C[i*rs + j*cs] = scale * sum_sp part[sp][...] + beta * C.  A workgroup is 64 outputs x RY split lanes: lane y sums
// the slices y, y+RY, y+2RY, ... (four independent running sums, so four loads are in flight), the RY lane totals
// are combined through LDS in a fixed order -> deterministic, and the sum over hundreds of slices is no longer
// one serial chain per output element (that chain used to cost more than the contraction itself for k <= 138).
// RY = 16 for the many-slice launches of tsgemm_ss, 4 when there are only a few slices (big tn launches: every
// lane then has work and the kernel is a plain HBM stream).
template <int RY>
__global__ __launch_bounds__(64 * RY) void k_reduce_partials(const double* __restrict__ part, int nsplit, int64_t pstride,
                                                             int inner_ld, int tr, int m, int k, double scale, double beta,
                                                             double* __restrict__ C, int64_t rs, int64_t cs) {
  __shared__ double sh[RY][64];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int fast = blockIdx.x * 64 + tx;
  const int fastn = tr ? m : k, slown = tr ? k : m;
  for (int slow = blockIdx.y; slow < slown; slow += gridDim.y) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (fast < fastn) {
      const double* p = part + (int64_t)slow * inner_ld + fast;
      int sp = ty;
      for (; sp + 3 * RY < nsplit; sp += 4 * RY) {
        s0 += p[(int64_t)sp * pstride];
        s1 += p[(int64_t)(sp + RY) * pstride];
        s2 += p[(int64_t)(sp + 2 * RY) * pstride];
        s3 += p[(int64_t)(sp + 3 * RY) * pstride];
      }
      for (; sp < nsplit; sp += RY) s0 += p[(int64_t)sp * pstride];
    }
    sh[ty][tx] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (ty == 0 && fast < fastn) {
      double s = 0.0;
#pragma unroll
      for (int y = 0; y < RY; ++y) s += sh[y][tx];
      const int i = tr ? fast : slow, j = tr ? slow : fast;
      double* out = C + (int64_t)i * rs + (int64_t)j * cs;
      *out = (beta != 0.0) ? scale * s + beta * (*out) : scale * s;
    }
    __syncthreads();
  }
}

// Flat variant for a row-major result whose row stride equals the partial's (C = G of an operator application,
// m x kpad): the m * kpad entries are one contiguous array per slice, so every lane streams (no 74-of-128 lane waste
// on a narrow fast axis); pad columns j >= k are written as zeros (tsgemm_nn reads G as a zero-padded small matrix).
template <int RY>
__global__ __launch_bounds__(64 * RY) void k_reduce_flat(const double* __restrict__ part, int nsplit, int64_t pstride,
                                                         int64_t total, int kpad, int k, double scale, double beta,
                                                         double* __restrict__ C) {
  __shared__ double sh[RY][64];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 64 + tx;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (idx < total) {
    const double* p = part + idx;
    int sp = ty;
    for (; sp + 3 * RY < nsplit; sp += 4 * RY) {
      s0 += p[(int64_t)sp * pstride];
      s1 += p[(int64_t)(sp + RY) * pstride];
      s2 += p[(int64_t)(sp + 2 * RY) * pstride];
      s3 += p[(int64_t)(sp + 3 * RY) * pstride];
    }
    for (; sp < nsplit; sp += RY) s0 += p[(int64_t)sp * pstride];
  }
  sh[ty][tx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ty == 0 && idx < total) {
    double s = 0.0;
#pragma unroll
    for (int y = 0; y < RY; ++y) s += sh[y][tx];
    const bool real = (int)(idx % kpad) < k;
    C[idx] = real ? ((beta != 0.0) ? scale * s + beta * C[idx] : scale * s) : 0.0;
  }
}

// Vector form of the two kernels above for the layouts the big launches use -- the fast axis is contiguous in the partials AND
// in C, rows 16-byte aligned: every thread owns TWO consecutive outputs and walks the slices with four independent running
// sums of 16-byte loads (the 8-byte, one-load-per-thread forms above moved 0.5 TB/s: 0.12 ms for the 65 MB of a config-4
// launch).  Same fixed summation order on every run.  kreal < rowlen: columns >= kreal of a row are written as zeros.
__global__ __launch_bounds__(256) void k_reduce_vec(const double* __restrict__ part, int nsplit, int64_t pstride, int64_t prow,
                                                    int64_t rowlen, int nrows, int64_t kpad, int kreal, double scale, double beta,
                                                    double* __restrict__ C, int64_t crow) {
  const int64_t f = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  if (f >= rowlen) return;
  for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
    const double* p = part + (int64_t)row * prow + f;
    d2 s0 = d2{0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0;
    int sp = 0;
    for (; sp + 3 < nsplit; sp += 4) {
      s0 += *reinterpret_cast<const d2*>(p + (int64_t)sp * pstride);
      s1 += *reinterpret_cast<const d2*>(p + (int64_t)(sp + 1) * pstride);
      s2 += *reinterpret_cast<const d2*>(p + (int64_t)(sp + 2) * pstride);
      s3 += *reinterpret_cast<const d2*>(p + (int64_t)(sp + 3) * pstride);
    }
    for (; sp < nsplit; ++sp) s0 += *reinterpret_cast<const d2*>(p + (int64_t)sp * pstride);
    d2 v = ((s0 + s1) + (s2 + s3)) * scale;
    double* out = C + (int64_t)row * crow + f;
    if (beta != 0.0) v += beta * *reinterpret_cast<const d2*>(out);
    if (kreal < kpad) {
      if ((int)(f % kpad) >= kreal) v.x = 0.0;
      if ((int)((f + 1) % kpad) >= kreal) v.y = 0.0;
    }
    *reinterpret_cast<d2*>(out) = v;
  }
}

int launch_reduce_partials(hfmi_ctx* ctx, const double* part, const reduce_call& c, double scale, double beta, double* C, int64_t rs,
                           int64_t cs) {
  const reduce_plan p = reduce_plan_make(c, rs, cs, (((uintptr_t)part | (uintptr_t)C) & 15) == 0);
  const dim3 grid(p.gx, p.gy);
  switch (p.route) {
    case HFMI_REDUCE_VEC_LONG:
    case HFMI_REDUCE_VEC_ROWS:
      hipLaunchKernelGGL(k_reduce_vec, grid, dim3(256), 0, ctx->stream, part, p.nsplit, c.pstride, (int64_t)c.inner_ld, p.rowlen, p.nrows,
                         p.kpad, p.kreal, scale, beta, C, p.crow);
      break;
    case HFMI_REDUCE_FLAT:
      hipLaunchKernelGGL(p.ry == 4 ? k_reduce_flat<4> : k_reduce_flat<16>, grid, dim3(64, p.ry), 0, ctx->stream, part, p.nsplit, c.pstride,
                         p.rowlen, c.inner_ld, p.k, scale, beta, C);
      break;
    default:
      hipLaunchKernelGGL(p.ry == 4 ? k_reduce_partials<4> : k_reduce_partials<16>, grid, dim3(64, p.ry), 0, ctx->stream, part, p.nsplit,
                         c.pstride, c.inner_ld, p.tr, p.m, p.k, scale, beta, C, rs, cs);
  }
  HIP_TRY(hipGetLastError());
  reduce_plan_words(p, plan_slot(ctx));
  return HFMI_OK;
}

// the instance <MT, NT, TR, WAVES, R4> of a plan; null: not compiled
typedef void (*tn_kernel_t)(const double*, int64_t, int, const double*, int64_t, int, int64_t, int64_t, int, int, double*, int64_t, int64_t,
                            int64_t, int, int, TnTail);
template <int MT, int NT, int WAVES>
static tn_kernel_t tn_kernel_r4(bool tr, int r4) {
#define TN_R4(R) \
  case R:        \
    return tr ? k_tsgemm_tn<MT, NT, true, WAVES, R> : k_tsgemm_tn<MT, NT, false, WAVES, R>;
  if constexpr (WAVES == 8) {
    switch (r4) { TN_R4(1) TN_R4(2) TN_R4(3) }
  }
  switch (0) { TN_R4(0) }
#undef TN_R4
  return nullptr;
}
template <int NT, int WAVES>
static tn_kernel_t tn_kernel_mt(int mt, bool tr, int r4) {
#define TN_CASE(M) \
  case M:          \
    if constexpr (M * NT <= tn_mt_limit(WAVES)) return tn_kernel_r4<M, NT, WAVES>(tr, r4); \
    break;
  switch (mt) { HFMI_TN_MT_CASES(TN_CASE) }
#undef TN_CASE
  return nullptr;
}
static tn_kernel_t tn_kernel(const tn_plan& p) {
#define TN_NT(NTV) \
  case NTV:        \
    return p.waves == 8 ? tn_kernel_mt<NTV, 8>(p.mt, p.tr, p.r4) : tn_kernel_mt<NTV, 4>(p.mt, p.tr, 0);
  switch (p.nt) { HFMI_TN_NT_CASES(TN_NT) }
#undef TN_NT
  return nullptr;
}

// one panel of at most 256 columns of B
static int tn_panel(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* B, int64_t ldb, int k,
                    int64_t N, double scale, double beta, double* C, int64_t rs, int64_t cs, int nsplit_req) {
  const tsgemm_knobs& kn = tsgemm_knobs_ref();
  const tn_plan p = tn_plan_make(m, k, N, scale, beta, rs, cs, C == A || C == B, nsplit_req, kn, ctx->num_cus);
  if (lda % 32 != 0 || ldb % 32 != 0 || lda < p.Npad || ldb < p.Npad)
    HFMI_FAIL(HFMI_ERR_INVALID, "tsgemm_tn: leading dimensions must be multiples of 32 and >= round_up(N,32)");
  const tn_kernel_t kern = p.has_instance ? tn_kernel(p) : nullptr;
  if (!kern) HFMI_FAIL(HFMI_ERR_INVALID, "tsgemm_tn: no instance for MT=%d NT=%d WAVES=%d", p.mt, p.nt, p.waves);
  void* partv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_PART, p.ws_bytes, &partv));
  double* part = (double*)partv;
  HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.shmem));
  // where the launch writes: split partials (the reduce kernel sums them) or, for one split with nothing to scale, C itself
  const int64_t psi = p.tr ? 1 : p.kpad;
  const TnTail tail = {p.tail_nrb, p.tail_nsplit, p.tail_chunk, p.tail_nrb ? part + p.tail_off : nullptr, psi, p.tr ? p.tail_mpad : 1,
                       (int64_t)p.tail_mpad * p.kpad};
  // algorithmic work of this launch: flops 2 N m k, bytes 8 (N m + N k + m k)
  const int pidx = prof_start(ctx, 0, m, k, N);
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.waves * 64), p.shmem, ctx->stream, A, lda, m, B, ldb, k, p.Npad, p.chunk, p.nrb, p.nsplit,
                     p.direct ? C : part, p.direct ? rs : psi, p.direct ? cs : (int64_t)(p.tr ? p.mpad : 1), (int64_t)p.mpad * p.kpad,
                     p.direct ? 1 : 0, kn.probe, tail);
  HIP_TRY(hipGetLastError());
  tn_plan_words(p, plan_slot(ctx));
  prof_stop(ctx, pidx);
  for (int i = 0; i < p.nred; ++i)
    HFMI_TRY(launch_reduce_partials(ctx, part + p.red[i].part_off, p.red[i], scale, beta, C + p.red[i].c_off, rs, cs));
  return HFMI_OK;
}

int launch_tsgemm_tn(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* B, int64_t ldb, int k,
                     int64_t N, double scale, double beta, double* C, int64_t rs, int64_t cs, int nsplit_req) {
  if (m <= 0 || k <= 0 || N <= 0) return HFMI_OK;
  if (tsgemm_knobs_ref().ss && ss_applicable(m, k, A == B && lda == ldb && m == k))
    return launch_tsgemm_ss(ctx, A, lda, m, B, ldb, k, N, scale, beta, C, rs, cs, nsplit_req);
  for (int k0 = 0; k0 < k; k0 += 256) {
    const int kp = (k - k0 < 256) ? (k - k0) : 256;
    HFMI_TRY(tn_panel(ctx, A, lda, m, B + (int64_t)k0 * ldb, ldb, kp, N, scale, beta, C + (int64_t)k0 * cs, rs, cs,
                      nsplit_req));
  }
  return HFMI_OK;
}
