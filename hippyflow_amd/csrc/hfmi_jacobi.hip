// Jacobi kernels of the Rayleigh-Ritz step, k <= 256, ONE workgroup with the matrix resident in LDS when it fits, fp64 throughout:
//   k_jacobi_eig[_db] : parallel cyclic Jacobi (round-robin ordering with the matrix kept in seat order, one 2x2-block rotation
//                       phase per round); rotations are logged and replayed on the identity by k_jacobi_vectors[_wave] (one
//                       workgroup or wave per eigenvector-matrix row), so the eigenvector update never sits on the critical path
//   k_jacobi_svd      : one-sided Jacobi SVD with the same ordering and the same replay
// The default eigensolver of the stage is divide and conquer (hfmi_eig_dc.hip); launch_sym_eig picks by sym_eig_route, and every
// launcher here launches what its plan (hfmi_small_plan.h) says.
#include "hfmi_internal.h"
#include "hfmi_small_dev.h"
#include "hfmi_small_plan.h"

// ------------------------------------------------------------------------------------------------
// Jacobi eigensolver
// ------------------------------------------------------------------------------------------------
// Round-robin tournament on n = 2 np players kept in SLOT order: the players of pair P always sit in the adjacent
// slots (2P, 2P+1) and the matrix is stored in slot order, S[s][t] = A[player(s)][player(t)].  After a round every
// player but the one in slot 0 moves one seat along the ring  1 -> 2 -> 4 -> ... -> n-2 -> n-1 -> n-3 -> ... -> 3 -> 1
// (Brent-Luk): n - 1 rounds meet every pair once and bring every player back to its own slot, so after whole
// sweeps slot order == player order.  The rotated 2x2 blocks are WRITTEN to their next-round seats, which makes
// every read of the update phase a fixed, aligned 16-byte pair (no index tables, no bank-conflict lottery).
__device__ __forceinline__ int jac_next_slot(int s, int n) {
  if (s == 0 || n == 2) return s;
  if (s & 1) return s == 1 ? 2 : s - 2;  // bottom row walks left; seat 1 climbs to the top row
  return s == n - 2 ? n - 1 : s + 2;     // top row walks right; the last seat drops to the bottom row
}

// Rotation (c, s) that annihilates the pivot of [[app, apq], [apq, aqq]]:  t = tan(phi) = sign(theta) /
// (|theta| + sqrt(theta^2 + 1)), theta = (aqq - app) / (2 apq), written with two reciprocal square roots instead of
// two divisions and two square roots (the dependent chain of this phase is pure latency on one CU):
// h = hypot(d, 2 apq), cos(2 phi) = |d| / h, c^2 = (1 + |d|/h) / 2, s = sign(d) apq / (h c).
__device__ __forceinline__ void jac_rotation(double app, double apq, double aqq, double& c, double& s) {
  c = 1.0;
  s = 0.0;
  const double g = 100.0 * fabs(apq);
  if (apq == 0.0 || (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq))) return;
  const double d = aqq - app;
  const double h2 = d * d + 4.0 * apq * apq;
  if (!(h2 > 1e-300) || !(h2 < 1e300)) {  // out of the safe range of the squared form: the classical formula
    const double theta = 0.5 * d / apq;
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = rsqrt(t * t + 1.0);
    s = t * c;
    return;
  }
  const double rh = fast_rsqrt(h2);
  const double c2 = 0.5 + 0.5 * fabs(d) * rh;
  const double rc = fast_rsqrt(c2);
  c = c2 * rc;
  s = (d >= 0.0 ? apq : -apq) * rh * rc;
}

// NB = 2x2 blocks per thread in the update phase (ceil(cells / threads)); the block coordinates of a thread never
// change, so all its addresses are computed once.
template <int NB, bool LDS>
__global__ __launch_bounds__(SMALL_THREADS) void k_jacobi_eig(const double* __restrict__ T, int ldt, int k,
                                                              double* __restrict__ gwork, int use_lds,
                                                              double2* __restrict__ rotlog, double* __restrict__ dvals,
                                                              int* __restrict__ perm, int sort_by_abs,
                                                              hfmi_status_words* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);                // 32
  double2* rot = reinterpret_cast<double2*>(red + 32);          // 128 (c, s) per pair
  double* Ad = reinterpret_cast<double*>(rot + 128);            // 256 diagonal copy / keys
  double* lds_a = Ad + 256;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int n = (k + 1) & ~1;  // players (one dummy if k is odd: a zero row/column that is never rotated)
  const int np = n / 2;
  // even leading dimension: the (2P, 2P+1) column pairs are 16-byte aligned.  LDS is a template parameter so that
  // the matrix pointer has ONE address space (a runtime LDS/global select would compile to FLAT accesses).
  int lda;
  double* A;
  if constexpr (LDS) {
    lda = n;
    A = lds_a;
  } else {
    lda = SM_LD;
    A = gwork;
  }
  const float inv_np1 = __frcp_rn((float)(np + 1));
  const int cells = ((np + 1) >> 1) * (np + 1);

  double fro = 0.0;
  for (int i = wave; i < n; i += nw)
    for (int j = lane; j < n; j += 64) {
      const double v = (i < k && j < k) ? 0.5 * (T[i * ldt + j] + T[j * ldt + i]) : 0.0;
      A[i * lda + j] = v;
      fro += v * v;
    }
  fro = block_sum(fro, red);
  __syncthreads();
  const double tol2 = EPS_D * EPS_D * fro;

  // this thread's blocks {P <= Q}: read offset of the block's first row and the next-round seat of each of its four
  // entries.  Only the block-upper triangle (pair(row) <= pair(col)) is stored and read: an entry whose new seat
  // falls below it is written transposed, so every entry costs ONE LDS store.
  int rd[NB], P_[NB], Q_[NB], d11[NB], d12[NB], d21[NB], d22[NB];
  bool live[NB];
  auto seat = [&](int r, int c) {
    const bool upper = (r >> 1) != (c >> 1) ? (r >> 1) < (c >> 1) : r <= c;
    return upper ? r * lda + c : c * lda + r;
  };
#pragma unroll
  for (int bi = 0; bi < NB; ++bi) {
    const int e = tid + bi * nthr;
    int P = 0, Q = 0;
    live[bi] = e < cells && tri_cell(e, np, inv_np1, P, Q);
    P_[bi] = P;
    Q_[bi] = Q;
    rd[bi] = 2 * P * lda + 2 * Q;
    const int r1 = jac_next_slot(2 * P, n), r2 = jac_next_slot(2 * P + 1, n);
    const int c1 = jac_next_slot(2 * Q, n), c2 = jac_next_slot(2 * Q + 1, n);
    d11[bi] = seat(r1, c1);
    d12[bi] = seat(r1, c2);
    d21[bi] = seat(r2, c1);
    d22[bi] = seat(r2, c2);
  }

  const long long tj0 = clock64();
  int sweeps = 0;
  double off2 = 0.0;
  for (; sweeps < JAC_MAX_SWEEPS; ++sweeps) {
    off2 = 0.0;
    for (int i = wave; i < n; i += nw)
      for (int j = i + 1 + lane; j < n; j += 64) off2 += 2.0 * A[i * lda + j] * A[i * lda + j];
    off2 = block_sum(off2, red);
    __syncthreads();
    if (off2 <= tol2) break;
    for (int r = 0; r < n - 1; ++r) {
      // phase 1: one rotation per pair from the diagonal block in seats (2P, 2P+1)
      if (tid < np) {
        const double2 top = *reinterpret_cast<const double2*>(A + 2 * tid * lda + 2 * tid);
        const double aqq = A[(2 * tid + 1) * lda + 2 * tid + 1];
        double c, sn;
        jac_rotation(top.x, top.y, aqq, c, sn);
        rot[tid] = make_double2(c, sn);
        rotlog[((size_t)sweeps * (n - 1) + r) * np + tid] = make_double2(c, sn);
      }
      __syncthreads();
      // phase 2: every 2x2 block {P, Q}, P <= Q, <- J_P^T * block * J_Q, written to the seats its players take in
      // the next round (block-upper triangle only).  All reads precede all writes.
      double z11[NB], z12[NB], z21[NB], z22[NB];
#pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
        if (!live[bi]) continue;
        const double2 x1 = *reinterpret_cast<const double2*>(A + rd[bi]);
        double2 x2 = *reinterpret_cast<const double2*>(A + rd[bi] + lda);
        if (P_[bi] == Q_[bi]) x2.x = x1.y;  // below the diagonal of a diagonal block: not stored
        {
          const double2 rp = rot[P_[bi]], rq = rot[Q_[bi]];
          // columns: (x_ip, x_iq) <- (c x_ip - s x_iq, s x_ip + c x_iq) with J_Q
          const double y11 = rq.x * x1.x - rq.y * x1.y, y12 = rq.y * x1.x + rq.x * x1.y;
          const double y21 = rq.x * x2.x - rq.y * x2.y, y22 = rq.y * x2.x + rq.x * x2.y;
          // rows with J_P
          z11[bi] = rp.x * y11 - rp.y * y21;
          z21[bi] = rp.y * y11 + rp.x * y21;
          z12[bi] = rp.x * y12 - rp.y * y22;
          z22[bi] = rp.y * y12 + rp.x * y22;
          if (P_[bi] == Q_[bi] && rp.y != 0.0) z12[bi] = 0.0;   // the annihilated pivot (an identity rotation keeps it)
        }
      }
      __syncthreads();
#pragma unroll
      for (int bi = 0; bi < NB; ++bi) {
        if (!live[bi]) continue;
        A[d11[bi]] = z11[bi];
        A[d22[bi]] = z22[bi];
        if (P_[bi] == Q_[bi]) {
          A[d12[bi]] = z12[bi];  // d12 == d21 here
        } else {
          A[d12[bi]] = z12[bi];
          A[d21[bi]] = z21[bi];
        }
      }
      __syncthreads();
    }
  }
  // whole sweeps bring every player back to its own slot: slot order == index order here.
  // eigenvalues, sort descending (rank by counting; ties broken by index -> a permutation)
  for (int i = tid; i < k; i += nthr) Ad[i] = A[i * lda + i];
  __syncthreads();
  for (int i = tid; i < k; i += nthr) {
    const double ki = sort_by_abs ? fabs(Ad[i]) : Ad[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const double kj = sort_by_abs ? fabs(Ad[j]) : Ad[j];
      if (kj > ki || (kj == ki && j < i)) ++rank;
    }
    perm[rank] = i;
    dvals[rank] = Ad[i];
  }
  if (tid == 0) {
    status->offdiag = fro > 0.0 ? sqrt(off2 / fro) : 0.0;
    status->sweeps = sweeps;
    status->failed = (sweeps >= JAC_MAX_SWEEPS && off2 > tol2) ? 1 : 0;
    status->tick[0] = clock64() - tj0;
    status->tick[1] = 0;
    status->tick[2] = 0;
    status->tick[3] = sweeps;
    status->tick[4] = 1;
  }
}

// The 2x2 block update shared by the update phase and the look-ahead pivots of k_jacobi_eig_db (which must
// reproduce the stored values bit for bit): z = J_P^T [x1; x2] J_Q, rp / rq = (c, s) of pairs P / Q.
__device__ __forceinline__ void jac_block(double2 x1, double2 x2, const double2 rp, const double2 rq, const bool diag,
                                          double& z11, double& z12, double& z21, double& z22) {
  if (diag) x2.x = x1.y;  // below the diagonal of a diagonal block: not stored
  const double y11 = rq.x * x1.x - rq.y * x1.y, y12 = rq.y * x1.x + rq.x * x1.y;
  const double y21 = rq.x * x2.x - rq.y * x2.y, y22 = rq.y * x2.x + rq.x * x2.y;
  z11 = rp.x * y11 - rp.y * y21;
  z21 = rp.y * y11 + rp.x * y21;
  z12 = rp.x * y12 - rp.y * y22;
  z22 = rp.y * y12 + rp.x * y22;
  if (diag && rp.y != 0.0) z12 = 0.0;  // the annihilated pivot (an identity rotation keeps it)
}

// k_jacobi_eig_db: the same tournament with ONE barrier per round instead of three (n <= 138).
//  * The block-upper triangle is PACKED, block (P, Q), P <= Q, at index P np - P (P - 1) / 2 + Q - P, in two planes
//    of 16-byte elements (top row / bottom row of the 2x2 block), and there are TWO such images: a round reads one and
//    writes the players' next seats into the other, so no barrier separates its reads from its writes
//    (2 x 2 x 2415 x 16 B = 154.6 KB at n = 138 -- the full square would not fit twice).
//  * The rotations of round g + 1 are computed DURING round g by the last two waves, which own no blocks: pair P' of the
//    next round is made of two players that sit in different pairs now, its three entries are three values the update
//    phase is about to store, and the look-ahead threads recompute exactly those (jac_block on the three source blocks,
//    same operation order) from the old image and the current rotations.  The dependent chain LDS read -> rotation ->
//    barrier -> LDS read -> update -> LDS write -> barrier of the three-barrier kernel becomes max(update, look-ahead).
template <int NB>
__global__ __launch_bounds__(SMALL_THREADS) void k_jacobi_eig_db(const double* __restrict__ T, int ldt, int k,
                                                                 double2* __restrict__ rotlog, double* __restrict__ dvals,
                                                                 int* __restrict__ perm, int sort_by_abs,
                                                                 hfmi_status_words* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);                // 32
  double2* rot = reinterpret_cast<double2*>(red + 32);          // 2 x 128 (c, s) per pair: this round / next round
  double* Ad = reinterpret_cast<double*>(rot + 256);            // 256 diagonal copy / keys
  double* img = Ad + 256;                                       // [2 images][4 planes][nblk]
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int n = (k + 1) & ~1;  // players (one dummy if k is odd: a zero row/column that is never rotated)
  const int np = n / 2;
  const int nblk = np * (np + 1) / 2;
  const int nupd = nthr - 128;                                   // update threads; the last two waves look ahead
  const float inv_np1 = __frcp_rn((float)(np + 1));
  const int cells = ((np + 1) >> 1) * (np + 1);
  auto bidx = [&](int P, int Q) { return P * np - P * (P - 1) / 2 + (Q - P); };
  // double index (within one image) of entry (r, c) of the seat-ordered matrix; lower entries map to their mirror
  auto seat = [&](int r, int c) {
    const bool upper = (r >> 1) != (c >> 1) ? (r >> 1) < (c >> 1) : r <= c;
    const int rr = upper ? r : c, cc = upper ? c : r;
    return ((rr & 1) * 2 + (cc & 1)) * nblk + bidx(rr >> 1, cc >> 1);
  };

  // this thread's blocks: element index in a plane, and the next-round seats of its four entries
  int bx[NB], d11[NB], d12[NB], d21[NB], d22[NB], P_[NB], Q_[NB];
  bool live[NB];
#pragma unroll
  for (int bi = 0; bi < NB; ++bi) {
    const int e = tid + bi * nupd;
    int P = 0, Q = 0;
    live[bi] = tid < nupd && e < cells && tri_cell(e, np, inv_np1, P, Q);
    P_[bi] = P;
    Q_[bi] = Q;
    bx[bi] = bidx(P, Q);
    const int r1 = jac_next_slot(2 * P, n), r2 = jac_next_slot(2 * P + 1, n);
    const int c1 = jac_next_slot(2 * Q, n), c2 = jac_next_slot(2 * Q + 1, n);
    d11[bi] = seat(r1, c1);
    d12[bi] = seat(r1, c2);
    d21[bi] = seat(r2, c1);
    d22[bi] = seat(r2, c2);
  }
  // look-ahead thread pi: the pair that will sit in seats (2 pi, 2 pi + 1) comes from the seats a, b of this round
  const int pi = tid - nupd;
  const bool ahead = pi >= 0 && pi < np;
  int pa = 0, pb = 0, ia = 0, ib = 0, bab = 0, baa = 0, bbb = 0;
  bool ab_swapped = false;
  if (ahead) {
    int a = 0, b = 0;
    for (int sl = 0; sl < n; ++sl) {
      const int nx = jac_next_slot(sl, n);
      if (nx == 2 * pi) a = sl;
      if (nx == 2 * pi + 1) b = sl;
    }
    pa = a >> 1; ia = a & 1; pb = b >> 1; ib = b & 1;
    ab_swapped = pb < pa;
    bab = ab_swapped ? bidx(pb, pa) : bidx(pa, pb);
    baa = bidx(pa, pa);
    bbb = bidx(pb, pb);
  }

  // load (symmetrised) into image 0, seat order == index order
  double fro = 0.0;
#pragma unroll
  for (int bi = 0; bi < NB; ++bi) {
    if (!live[bi]) continue;
    double v[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = 2 * P_[bi] + i, c = 2 * Q_[bi] + j;
        v[i][j] = (r < k && c < k) ? 0.5 * (T[r * ldt + c] + T[c * ldt + r]) : 0.0;
      }
    img[bx[bi]] = v[0][0];
    img[nblk + bx[bi]] = v[0][1];
    img[2 * nblk + bx[bi]] = v[1][0];
    img[3 * nblk + bx[bi]] = v[1][1];
    if (P_[bi] == Q_[bi]) fro += v[0][0] * v[0][0] + v[1][1] * v[1][1] + 2.0 * v[0][1] * v[0][1];
    else fro += 2.0 * (v[0][0] * v[0][0] + v[0][1] * v[0][1] + v[1][0] * v[1][0] + v[1][1] * v[1][1]);
  }
  fro = block_sum(fro, red);
  __syncthreads();
  const double tol2 = EPS_D * EPS_D * fro;
  const long long max_rounds = (long long)JAC_MAX_SWEEPS * (n - 1);

  // rotations of the very first round, straight from the diagonal blocks
  if (tid < np) {
    const int bd = bidx(tid, tid);
    double c, sn;
    jac_rotation(img[bd], img[nblk + bd], img[3 * nblk + bd], c, sn);
    rot[tid] = make_double2(c, sn);
    rotlog[tid] = make_double2(c, sn);
  }
  __syncthreads();

  // the look-ahead chain is serial and decides the length of a round: its waves get issue priority over the update
  // waves they share a SIMD with (without it k = 74 ran 16 % slower than the three-barrier kernel)
  if (tid >= nupd) __builtin_amdgcn_s_setprio(3);
  const long long tj0 = clock64();
  int sweeps = 0, cur = 0;
  long long g = 0;  // global round counter
  double off2 = 0.0;
  for (; sweeps < JAC_MAX_SWEEPS; ++sweeps) {
    const double* A = img + (size_t)cur * 4 * nblk;
    off2 = 0.0;
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
      if (!live[bi]) continue;
      const double2 x1 = make_double2(A[bx[bi]], A[nblk + bx[bi]]), x2 = make_double2(A[2 * nblk + bx[bi]], A[3 * nblk + bx[bi]]);
      if (P_[bi] == Q_[bi]) off2 += 2.0 * x1.y * x1.y;
      else off2 += 2.0 * (x1.x * x1.x + x1.y * x1.y + x2.x * x2.x + x2.y * x2.y);
    }
    off2 = block_sum(off2, red);
    __syncthreads();
    if (off2 <= tol2) break;
    for (int r = 0; r < n - 1; ++r, ++g) {
      const double* Ar = img + (size_t)cur * 4 * nblk;
      double* Aw = img + (size_t)(cur ^ 1) * 4 * nblk;
      auto blk = [&](int b, double2& x1, double2& x2) {
        x1 = make_double2(Ar[b], Ar[nblk + b]);
        x2 = make_double2(Ar[2 * nblk + b], Ar[3 * nblk + b]);
      };
      const double2* rt = rot + (g & 1) * 128;
      if (tid < nupd) {
#pragma unroll
        for (int bi = 0; bi < NB; ++bi) {
          if (!live[bi]) continue;
          double2 x1, x2;
          blk(bx[bi], x1, x2);
          double z11, z12, z21, z22;
          jac_block(x1, x2, rt[P_[bi]], rt[Q_[bi]], P_[bi] == Q_[bi], z11, z12, z21, z22);
          Aw[d11[bi]] = z11;
          Aw[d22[bi]] = z22;
          Aw[d12[bi]] = z12;                          // d12 == d21 for a diagonal block
          if (P_[bi] != Q_[bi]) Aw[d21[bi]] = z21;
        }
      } else if (ahead) {
        double z11, z12, z21, z22;
        double2 x1, x2;
        const double2 ra = rt[pa], rb = rt[pb];
        blk(baa, x1, x2);
        jac_block(x1, x2, ra, ra, true, z11, z12, z21, z22);
        const double naa = ia ? z22 : z11;
        blk(bbb, x1, x2);
        jac_block(x1, x2, rb, rb, true, z11, z12, z21, z22);
        const double nbb = ib ? z22 : z11;
        double nab;
        blk(bab, x1, x2);
        if (pa == pb) {
          jac_block(x1, x2, ra, ra, true, z11, z12, z21, z22);
          nab = z12;
        } else if (!ab_swapped) {
          jac_block(x1, x2, ra, rb, false, z11, z12, z21, z22);
          nab = ia ? (ib ? z22 : z21) : (ib ? z12 : z11);
        } else {  // stored block is (pb, pa): rows belong to b's pair
          jac_block(x1, x2, rb, ra, false, z11, z12, z21, z22);
          nab = ib ? (ia ? z22 : z21) : (ia ? z12 : z11);
        }
        double c, sn;
        jac_rotation(naa, nab, nbb, c, sn);
        rot[((g + 1) & 1) * 128 + pi] = make_double2(c, sn);
        if (g + 1 < max_rounds) rotlog[(size_t)(g + 1) * np + pi] = make_double2(c, sn);
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  // whole sweeps bring every player back to its own slot: slot order == index order here.
  {
    const double* A = img + (size_t)cur * 4 * nblk;
    for (int i = tid; i < k; i += nthr) {
      const int P = i >> 1;
      Ad[i] = (i & 1) ? A[3 * nblk + bidx(P, P)] : A[bidx(P, P)];
    }
  }
  __syncthreads();
  for (int i = tid; i < k; i += nthr) {
    const double ki = sort_by_abs ? fabs(Ad[i]) : Ad[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const double kj = sort_by_abs ? fabs(Ad[j]) : Ad[j];
      if (kj > ki || (kj == ki && j < i)) ++rank;
    }
    perm[rank] = i;
    dvals[rank] = Ad[i];
  }
  if (tid == 0) {
    status->offdiag = fro > 0.0 ? sqrt(off2 / fro) : 0.0;
    status->sweeps = sweeps;
    status->failed = (sweeps >= JAC_MAX_SWEEPS && off2 > tol2) ? 1 : 0;
    status->tick[0] = clock64() - tj0;
    status->tick[1] = 0;
    status->tick[2] = 0;
    status->tick[3] = sweeps;
    status->tick[4] = 2;
  }
}

// Row i of V = e_i^T * (product of all logged rotations); one workgroup per row.  The row is kept in slot order
// in two LDS buffers: lane P rotates the adjacent pair (2P, 2P+1) of the current buffer and writes it to the
// players' next seats in the other one -- one barrier per round, no index arithmetic.
__global__ __launch_bounds__(128) void k_jacobi_vectors(const double2* __restrict__ rotlog, int k,
                                                        const hfmi_status_words* __restrict__ status,
                                                        const int* __restrict__ perm, double* __restrict__ V, int ldv) {
  __shared__ __attribute__((aligned(16))) double row[2][SM_MAXK + 2];
  const int n = (k + 1) & ~1, np = n / 2;
  const int i = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < n; j += blockDim.x) row[0][j] = (j == i) ? 1.0 : 0.0;
  __syncthreads();
  const int rounds = status->sweeps * (n - 1);
  const int s1 = jac_next_slot(2 * tid, n), s2 = jac_next_slot(2 * tid + 1, n);
  int cur = 0;
  // the (c, s) pairs come from global memory and depend on nothing: keep PF rounds of them in flight in registers,
  // otherwise every round pays a full memory round trip between two barriers
  constexpr int PF = 8;
  const bool act = tid < np;
  const double2* lg = rotlog + (act ? tid : 0);
  double2 ring[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) ring[u] = (u < rounds) ? lg[(size_t)u * np] : make_double2(1.0, 0.0);
  for (int r0 = 0; r0 < rounds; r0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int rr = r0 + u;
      if (rr < rounds) {   // uniform
        const double2 cs = ring[u];
        const int nx = rr + PF;
        ring[u] = (nx < rounds) ? lg[(size_t)nx * np] : make_double2(1.0, 0.0);
        if (act) {
          const double2 v = *reinterpret_cast<const double2*>(&row[cur][2 * tid]);
          row[cur ^ 1][s1] = cs.x * v.x - cs.y * v.y;
          row[cur ^ 1][s2] = cs.y * v.x + cs.x * v.y;
        }
        __syncthreads();
        cur ^= 1;
      }
    }
  }
  for (int c = tid; c < k; c += blockDim.x) V[i * ldv + c] = row[cur][perm[c]];
  for (int c = k + tid; c < ((k + 15) & ~15); c += blockDim.x) V[i * ldv + c] = 0.0;
}

// ------------------------------------------------------------------------------------------------
// k_jacobi_vectors_wave: the same replay with one WAVE per row (n <= 128 seats: lane P keeps the pair seated in
// (2P, 2P+1) in registers).  A round is a rotation in registers and three lane shifts (the top row of the tournament
// walks right, the bottom row left, the two end seats swap rows) -- no LDS, no barrier.
// whole-wave shifts by one lane as DPP moves (wave_shr:1 = 0x138, wave_shl:1 = 0x130 on GFX9): two v_mov_b32_dpp per
// double instead of two ds_bpermute round trips (with __shfl the replay was slower than the LDS version)
__device__ __forceinline__ double lane_shr1(double v) {   // lane P <- lane P - 1 (lane 0 keeps its own)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_shl1(double v) {   // lane P <- lane P + 1 (lane 63 keeps its own)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__global__ __launch_bounds__(256) void k_jacobi_vectors_wave(const double2* __restrict__ rotlog, int k,
                                                             const hfmi_status_words* __restrict__ status,
                                                             const int* __restrict__ perm, double* __restrict__ V, int ldv) {
  __shared__ double rowbuf[4][130];
  const int n = (k + 1) & ~1, np = n / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;                     // row of V handled by this wave (wave-uniform)
  const int rounds = status->sweeps * (n - 1);
  const bool act = lane < np;
  double x = (2 * lane == i) ? 1.0 : 0.0, y = (2 * lane + 1 == i) ? 1.0 : 0.0;
  constexpr int PF = 32;   // a round is ~100 cycles here: 8 rounds ahead no longer cover the memory latency
  const double2* lg = rotlog + (act ? lane : 0);
  double2 ring[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) ring[u] = (u < rounds) ? lg[(size_t)u * np] : make_double2(1.0, 0.0);
  if (i < k) {
    for (int r0 = 0; r0 < rounds; r0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int rr = r0 + u;
        if (rr < rounds) {   // uniform
          const double2 cs = act ? ring[u] : make_double2(1.0, 0.0);
          const int nxt = rr + PF;
          ring[u] = (nxt < rounds) ? lg[(size_t)nxt * np] : make_double2(1.0, 0.0);
          const double nx = cs.x * x - cs.y * y, ny = cs.y * x + cs.x * y;
          if (n > 2) {
            const double xr = lane_shr1(nx), yr = lane_shr1(ny), yl = lane_shl1(ny);
            x = (lane == 0) ? nx : (lane == 1) ? yr : xr;    // seat 0 stays, seat 1 climbs to seat 2, 2P-2 -> 2P
            y = (lane == np - 1) ? nx : yl;                  // seat n-2 drops to n-1, 2P+3 -> 2P+1
          } else {
            x = nx;
            y = ny;
          }
        }
      }
    }
    if (act) {
      rowbuf[wave][2 * lane] = x;
      rowbuf[wave][2 * lane + 1] = y;
    }
  }
  __syncthreads();
  if (i < k) {
    for (int c = lane; c < k; c += 64) V[i * ldv + c] = rowbuf[wave][perm[c]];
    for (int c = k + lane; c < ((k + 15) & ~15); c += 64) V[i * ldv + c] = 0.0;
  }
}

// One-sided (Hestenes) Jacobi SVD of a small square matrix R = U diag(sigma) V^T: column pairs of W (= R, then
// R V) are rotated until mutually orthogonal; sigma_j = ||w_j||, U = W diag(1/sigma), V = product of the
// rotations (logged, replayed by k_jacobi_vectors).  Full relative accuracy for small singular values (unlike
// eig(R^T R)).  Used by accuracyEnhancedSVD (hippylib randomizedSVD; activeSubspaceProjector.py:813-834,1026).
// One 16-lane group per column pair, one workgroup barrier per round.
// ------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(SMALL_THREADS) void k_jacobi_svd(const double* __restrict__ R, int ldr, int k,
                                                              double* __restrict__ gwork, int use_lds,
                                                              double2* __restrict__ rotlog, double* __restrict__ svals,
                                                              int* __restrict__ perm, double* __restrict__ Uleft, int ldu,
                                                              hfmi_status_words* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);   // 32
  double* sig = red + 32;                          // 256
  short* who = reinterpret_cast<short*>(sig + 256);  // [2][264]: player seated in each slot (jac_next_slot schedule)
  double* lds_w = sig + 256 + 132;
  int ldw;
  double* W;                                       // column-major: W[col * ldw + row]; one address space (see k_chol_inv)
  if constexpr (LDS) {
    ldw = k | 1;
    W = lds_w;
  } else {
    ldw = SM_LD;
    W = gwork;
  }
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int grp = tid >> 4, gl = tid & 15, ngrp = nthr >> 4;
  const int n = (k + 1) & ~1, np = n / 2;
  // power-of-two scaling to max |entry| in [1, 2), undone on sigma at the end (exact both ways, so U, V and the bits of sigma do
  // not depend on it): the pair test below multiplies two squared column norms, the FOURTH power of the data, which unscaled
  // leaves the exponent range for entries beyond 1e+-77 -- every pair then looked orthogonal and R came back unrotated
  double amax = 0.0;
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) amax = fmax(amax, fabs(R[i * ldr + j]));
  amax = -block_min(-amax, red);
  int sexp = 0;
  if (amax > 0.0 && isfinite(amax)) sexp = ilogb(amax);
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) W[j * ldw + i] = ldexp(R[i * ldr + j], -sexp);
  for (int j = tid; j < n; j += nthr) who[j] = (short)j;
  __syncthreads();
  int sweeps = 0, cur = 0;
  double worst = 0.0;
  for (; sweeps < JAC_MAX_SWEEPS; ++sweeps) {
    double mx = 0.0;
    for (int r = 0; r < n - 1; ++r) {
      const short* wc = who + cur * 264;
      for (int P = grp; P < np; P += ngrp) {
        // the pair seated in slots (2P, 2P+1); same schedule and orientation as k_jacobi_vectors replays
        const int a = wc[2 * P], b = wc[2 * P + 1];
        double c = 1.0, sn = 0.0;
        if (a < k && b < k) {
          double* wa = W + a * ldw;
          double* wb = W + b * ldw;
          double al = 0.0, be = 0.0, ga = 0.0;
          for (int i = gl; i < k; i += 16) {
            const double x = wa[i], y = wb[i];
            al += x * x;
            be += y * y;
            ga += x * y;
          }
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) {
            al += __shfl_xor(al, off, 64);
            be += __shfl_xor(be, off, 64);
            ga += __shfl_xor(ga, off, 64);
          }
          const double lim = sqrt(al * be);
          const double ratio = lim > 0.0 ? fabs(ga) / lim : 0.0;
          mx = fmax(mx, ratio);
          if (ratio > EPS_D) {
            const double zeta = 0.5 * (be - al) / ga;
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            c = rsqrt(1.0 + t * t);
            sn = c * t;
            for (int i = gl; i < k; i += 16) {
              const double x = wa[i], y = wb[i];
              wa[i] = c * x - sn * y;
              wb[i] = sn * x + c * y;
            }
          }
        }
        if (gl == 0) rotlog[((size_t)sweeps * (n - 1) + r) * np + P] = make_double2(c, sn);
      }
      for (int j = tid; j < n; j += nthr) who[(cur ^ 1) * 264 + jac_next_slot(j, n)] = wc[j];
      cur ^= 1;
      __syncthreads();
    }
    // convergence: every pair of the sweep was already orthogonal to round-off
    mx = -block_min(-mx, red);
    worst = mx;
    __syncthreads();
    if (mx <= 4.0 * EPS_D) {
      ++sweeps;
      break;
    }
  }
  // singular values, sort descending
  for (int j = wave; j < k; j += nw) {
    double a2 = 0.0;
    for (int i = lane; i < k; i += 64) a2 += W[j * ldw + i] * W[j * ldw + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a2 += __shfl_down(a2, off, 64);
    if (lane == 0) sig[j] = sqrt(a2);
  }
  __syncthreads();
  for (int i = tid; i < k; i += nthr) {
    const double ki = sig[i];
    int rank = 0;
    for (int j = 0; j < k; ++j)
      if (sig[j] > ki || (sig[j] == ki && j < i)) ++rank;
    perm[rank] = i;
    svals[rank] = ldexp(ki, sexp);
  }
  __syncthreads();
  // left singular vectors U[:, c] = w_perm[c] / sigma  (row-major k x k output)
  for (int cidx = wave; cidx < k; cidx += nw) {
    const int j = perm[cidx];
    const double inv = sig[j] > 0.0 ? 1.0 / sig[j] : 0.0;
    for (int i = lane; i < k; i += 64) Uleft[i * ldu + cidx] = W[j * ldw + i] * inv;
  }
  if (tid == 0) {
    status->offdiag = worst;
    status->sweeps = sweeps > JAC_MAX_SWEEPS ? JAC_MAX_SWEEPS : sweeps;
    status->failed = (worst > 1e-12) ? 1 : 0;
    status->tick[4] = 2;
  }
}

// the instances of a plan (HFMI_JACOBI_*_CASES, hfmi_small_plan.h); null: not compiled
typedef decltype(&k_jacobi_eig<1, true>) jacobi_eig_fn;
static jacobi_eig_fn jacobi_eig_kernel(int nb, int lds) {
  switch (nb) {
#define X(NB) \
  case NB:    \
    return lds ? k_jacobi_eig<NB, true> : k_jacobi_eig<NB, false>;
    HFMI_JACOBI_NB_CASES(X)
#undef X
  }
  return nullptr;
}
typedef decltype(&k_jacobi_eig_db<1>) jacobi_db_fn;
static jacobi_db_fn jacobi_db_kernel(int nb) {
  switch (nb) {
#define X(NB) \
  case NB:    \
    return k_jacobi_eig_db<NB>;
    HFMI_JACOBI_DB_CASES(X)
#undef X
  }
  return nullptr;
}
// the replay of the logged rotations on the identity: the second launch of both plans
static void launch_jacobi_replay(hfmi_ctx* ctx, const small_launch& L, int k, const double2* rotlog, const int* perm, int slot_v) {
  hipLaunchKernelGGL(L.family == SF_JACOBI_VECTORS_WAVE ? k_jacobi_vectors_wave : k_jacobi_vectors, dim3(L.grid), dim3(L.threads), 0,
                     ctx->stream, rotlog, k, ctx->status_dev, perm, sm_ptr(ctx, slot_v), SM_LD);
}

int launch_jacobi_svd(hfmi_ctx* ctx, int k, int slot_r, int slot_u, int slot_v, double* svals) {
  if (k < 1 || k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "jacobi_svd: k=%d out of range", k);
  const small_plan p = jacobi_svd_plan(k, small_knobs_ref());
  void* logv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_MISC, (size_t)p.ws_bytes, &logv));
  const jacobi_ws w = jacobi_ws_carve(p, logv);
  double2* rotlog = (double2*)w.rotlog;
  int* perm = (int*)w.perm;
  const small_launch& L = p.launch[0];
  const auto kern = L.t[0] ? k_jacobi_svd<true> : k_jacobi_svd<false>;
  HFMI_TRY(small_raise_lds((const void*)kern, L));
  hipLaunchKernelGGL(kern, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, sm_ptr(ctx, slot_r), SM_LD, k, sm_ptr(ctx, SM_TMP), p.use_lds,
                     rotlog, svals, perm, sm_ptr(ctx, slot_u), SM_LD, ctx->status_dev);
  HIP_TRY(hipGetLastError());
  launch_jacobi_replay(ctx, p.launch[1], k, rotlog, perm, slot_v);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

int launch_jacobi_eig(hfmi_ctx* ctx, int k, int slot_t, int slot_v, double* dvals, int sort_by_abs) {
  if (k < 1 || k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "jacobi_eig: k=%d out of range", k);
  const small_plan p = jacobi_eig_plan(k, small_knobs_ref());
  if (p.refuse)
    HFMI_FAIL(HFMI_ERR_INVALID, "jacobi_eig: %d blocks per thread (k=%d, %d threads) not instantiated", p.nb, k, small_knobs_ref().small_threads);
  void* logv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_MISC, (size_t)p.ws_bytes, &logv));
  const jacobi_ws w = jacobi_ws_carve(p, logv);
  double2* rotlog = (double2*)w.rotlog;
  int* perm = (int*)w.perm;
  const small_launch& L = p.launch[0];
  if (L.family == SF_JACOBI_EIG_DB) {
    const jacobi_db_fn kern = jacobi_db_kernel(L.t[0]);
    if (!kern) HFMI_FAIL(HFMI_ERR_INVALID, "jacobi_eig: no k_jacobi_eig_db<%d>", L.t[0]);
    HFMI_TRY(small_raise_lds((const void*)kern, L));
    hipLaunchKernelGGL(kern, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, sm_ptr(ctx, slot_t), SM_LD, k, rotlog, dvals, perm,
                       sort_by_abs, ctx->status_dev);
  } else {
    const jacobi_eig_fn kern = jacobi_eig_kernel(L.t[0], L.t[1]);
    if (!kern) HFMI_FAIL(HFMI_ERR_INVALID, "jacobi_eig: no k_jacobi_eig<%d, %d>", L.t[0], L.t[1]);
    HFMI_TRY(small_raise_lds((const void*)kern, L));
    hipLaunchKernelGGL(kern, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, sm_ptr(ctx, slot_t), SM_LD, k, sm_ptr(ctx, SM_TMP),
                       p.use_lds, rotlog, dvals, perm, sort_by_abs, ctx->status_dev);
  }
  HIP_TRY(hipGetLastError());
  launch_jacobi_replay(ctx, p.launch[1], k, rotlog, perm, slot_v);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}

// Rayleigh-Ritz eigensolver selection.  Default: divide and conquer (hfmi_eig_dc.hip; k = 74: 0.68 -> about 0.15 ms).  The
// Jacobi kernels above stay for callers that want the high RELATIVE accuracy of small eigenvalues of graded positive
// definite matrices (hfmi_sym_eig_small flag bit 1, hfmi_double_pass flag bit 3) and for A/B runs (tuning "eig" = 1).
int launch_sym_eig(hfmi_ctx* ctx, int k, int slot_t, int slot_v, double* dvals, int sort_by_abs, int method) {
  if (sym_eig_route(method, small_knobs_ref())) return launch_jacobi_eig(ctx, k, slot_t, slot_v, dvals, sort_by_abs);
  return launch_dc_eig(ctx, k, slot_t, slot_v, dvals, sort_by_abs);
}
