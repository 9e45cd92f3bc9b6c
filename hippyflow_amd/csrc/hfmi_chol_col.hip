// Column-at-a-time Cholesky + triangular inverse of the Cholesky-QR step, k <= 256, ONE workgroup, fp64 throughout:
//   k_chol_inv  : the generic kernel (any k; the matrix in LDS when it fits, else in a global slot)
//   k_chol_reg  : k <= 139, the upper triangle in registers, dealt cyclically over 512 threads
//   k_chol_tile : register tiles of TR x TC per thread; 512 threads with the factor's copy in LDS (k <= 139), 1024 threads with
//                 the copy in a global slot (140 <= k <= 256)
// G = R^T R (upper), optional diagonal shift on breakdown, R^{-1}, running R product.  The default route is the blocked MFMA
// kernel of hfmi_chol.hip; these stay for A/B runs and as the reference the tests compare that kernel with.  launch_chol_inv
// launches what chol_plan (hfmi_small_plan.h) says.
#include "hfmi_internal.h"
#include "hfmi_small_dev.h"
#include "hfmi_small_plan.h"

// ------------------------------------------------------------------------------------------------
// Cholesky + triangular inverse.  M points at the working k x k matrix (LDS when it fits, else a global
// scratch slot), row-major with leading dimension ldm.
//
// One workgroup; everything here is issue/latency bound on a single CU (fp64 VALU is quarter rate: a dependent
// v_fma_f64 costs 32 cycles with 4 waves per SIMD; a software fp64 divide ~300), so the structure avoids
// redundant scalar fp64 math (v_rsq_f64 + Newton instead of sqrt and divide on every thread), maps triangular
// index sets onto ALL lanes (folded triangle, reciprocal-multiply index split) and spends ONE barrier per column
// of the factorisation and one per row of the inverse.
// ------------------------------------------------------------------------------------------------
// Generic path (any k <= 256; the matrix in LDS when it fits, else in a global scratch slot -- the pointer is then
// generic and the accesses are FLAT: this kernel is the fallback, k_chol_reg below is the fast path for k <= 139).
__global__ __launch_bounds__(SMALL_THREADS) void k_chol_inv(const double* __restrict__ G, int ldg, int k,
                                                            double* __restrict__ Rout, double* __restrict__ Rinv,
                                                            double* __restrict__ Rtot, double* __restrict__ Rtmp,
                                                            int ldo, int rtot_mode, int full_r, double shift_rel,
                                                            double pivot_tol, double* __restrict__ gscratch,
                                                            int use_lds, double* __restrict__ colnorm0,
                                                            double* __restrict__ rdiag,
                                                            hfmi_status_words* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);       // 32 doubles of reduction scratch
  double* diag0 = red + 32;                            // k original diagonal entries
  double* invd = diag0 + 256;                          // 1 / R_jj
  double* ird0 = invd + 256;                           // 1 / (original diagonal + shift): pivot-ratio bookkeeping
  double* lds_m = ird0 + 256;
  const int ldm = use_lds ? (k | 1) : ldo;
  double* M = use_lds ? lds_m : gscratch;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  __shared__ int s_break;

  long long tk0 = clock64(), tk1, tk2, tk3, tk4;
  // diag and orthonormality defect || D^-1/2 G D^-1/2 - I ||_F of the input
  for (int i = tid; i < k; i += nthr) {
    diag0[i] = G[i * ldg + i];
    if (rtot_mode == 1) colnorm0[i] = sqrt(fmax(diag0[i], 0.0));  // norms of the ORIGINAL columns (first pass)
  }
  __syncthreads();
  for (int i = tid; i < k; i += nthr) invd[i] = diag0[i] > 0.0 ? fast_rsqrt(diag0[i]) : 0.0;
  __syncthreads();
  double dev = 0.0, tr = 0.0;
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) {
      const double g = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
      const double x = g * invd[i] * invd[j] - (i == j ? 1.0 : 0.0);
      dev += x * x;
      if (i == j) tr += g;
    }
  dev = block_sum(dev, red);
  tr = block_sum(tr, red);
  tk1 = clock64();

  int shifted = 0, failed = 0;
  double min_ratio = 1e300;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const double shift = attempt ? shift_rel * tr : 0.0;
    for (int i = wave; i < k; i += nw)
      for (int j = lane; j < k; j += 64) {
        double g = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
        if (i == j) g += shift;
        M[i * ldm + j] = (j >= i) ? g : 0.0;
      }
    if (tid == 0) s_break = 0;
    for (int i = tid; i < k; i += nthr) ird0[i] = (diag0[i] + shift > 0.0) ? 1.0 / (diag0[i] + shift) : 0.0;
    __syncthreads();
    double ratio_local = 1e300;
    // Unscaled (LDL^T-style) right-looking factorisation: U[i][c] = G[i][c] - sum_{j<i} U[j][i] U[j][c] / U[j][j].
    // Row j is never rewritten once it is the pivot row, so a column step is ONE barrier phase: every thread reads
    // the pivot, forms 1 / U[j][j] itself (v_rsq_f64 + Newton, squared) and updates its share of the trailing
    // triangle.  R = diag(U)^{-1/2} U is formed by one scaling pass at the end.
    for (int j = 0; j < k; ++j) {
      const double piv = M[j * ldm + j];
      const double ref = diag0[j] + shift;
      if (!(piv > pivot_tol * ref) || !(ref > 0.0)) {  // uniform decision: every thread reads the same words
        if (tid == 0) s_break = 1;
        break;
      }
      const double inv = fast_rsqrt(piv);
      const double rp = inv * inv;
      if (tid == 0) {
        ratio_local = fmin(ratio_local, piv * ird0[j]);
        invd[j] = inv;
      }
      // trailing update of the upper triangle: M[i][c] -= U[j][i] U[j][c] / U[j][j], j < i <= c (folded onto all lanes)
      const int n = k - j - 1;
      if (n > 0) {
        const float inv_np1 = __frcp_rn((float)(n + 1));
        const int cells = ((n + 1) >> 1) * (n + 1);
        const double* rj = M + j * ldm + j + 1;
        for (int e = tid; e < cells; e += nthr) {
          int a, b;
          if (tri_cell(e, n, inv_np1, a, b)) M[(j + 1 + a) * ldm + j + 1 + b] -= rj[a] * rp * rj[b];
        }
      }
      __syncthreads();
    }
    __syncthreads();
    if (!s_break) {
      min_ratio = ratio_local;
      break;
    }
    if (attempt == 0) shifted = 1;
    else failed = 1;
    __syncthreads();
  }
  if (failed) {
    if (tid == 0) {
      status->min_pivot_ratio = 0.0;
      status->gram_dev = sqrt(dev);
      status->shifted = shifted;
      status->failed = 1;
    }
    return;
  }
  // R = diag(U)^{-1/2} U
  for (int i = wave; i < k; i += nw) {
    const double sc = invd[i];
    for (int j = i + lane; j < k; j += 64) M[i * ldm + j] *= sc;
  }
  __syncthreads();
  tk2 = clock64();
  // R out (upper triangle, zeros below)
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) Rout[i * ldo + j] = (j >= i) ? M[i * ldm + j] : 0.0;
  // Inverse X = R^-1 by back substitution, one ROW per barrier phase (bottom up): x_cc = 1/R_cc and, for i < c,
  // x_ic = -(sum_{l=i+1..c} R[i][l] x_lc) / R_ii.  All columns c > i of row i are independent: one 8-lane group per
  // column, both factors of the dot product contiguous along l (x is kept in the unused strictly lower triangle,
  // X[i][c] -> M[c][i]).
  {
    const int g8 = tid & 7, grp8 = tid >> 3, ngrp8 = nthr >> 3;
    for (int i = k - 2; i >= 0; --i) {
      const double* ri = M + i * ldm;
      const double mi = -invd[i];
      for (int c = i + 1 + grp8; c < k; c += ngrp8) {
        const double* xr = M + c * ldm;
        const double xc = invd[c];
        double sacc = 0.0;
        for (int l = i + 1 + g8; l <= c; l += 8) sacc += ri[l] * (l == c ? xc : xr[l]);
        sacc += __shfl_xor(sacc, 4, 64);
        sacc += __shfl_xor(sacc, 2, 64);
        sacc += __shfl_xor(sacc, 1, 64);
        if (g8 == 0) M[c * ldm + i] = sacc * mi;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  tk3 = clock64();
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) Rinv[i * ldo + j] = (j > i) ? M[j * ldm + i] : (j == i ? invd[i] : 0.0);
  // diagonal of the running product R = R_p ... R_1 (its ratio to the original column norms exposes
  // numerically dependent columns); the full product only when the caller wants R
  for (int i = tid; i < k; i += nthr) rdiag[i] = (rtot_mode == 1 ? 1.0 : rdiag[i]) * M[i * ldm + i];
  if (full_r) {
    if (rtot_mode == 1) {
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) Rtot[i * ldo + j] = (j >= i) ? M[i * ldm + j] : 0.0;
    } else {
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) {
          double acc = 0.0;
          if (j >= i)
            for (int l = i; l <= j; ++l) acc += M[i * ldm + l] * Rtot[l * ldo + j];
          Rtmp[i * ldo + j] = acc;
        }
      __syncthreads();
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) Rtot[i * ldo + j] = Rtmp[i * ldo + j];
    }
  }
  tk4 = clock64();
  if (tid == 0) {
    status->min_pivot_ratio = min_ratio;
    status->gram_dev = sqrt(dev);
    status->shifted = shifted;
    status->failed = 0;
    status->tick[0] = tk1 - tk0;  // load + defect
    status->tick[1] = tk2 - tk1;  // Cholesky
    status->tick[2] = tk3 - tk2;  // inverse
    status->tick[3] = tk4 - tk3;  // outputs + R product
    status->tick[4] = 0;

  }
}

// ------------------------------------------------------------------------------------------------
// k_chol_reg: the same contract as k_chol_inv for an LDS-resident matrix (k <= 139), built around what one CU
// actually charges for: INSTRUCTION ISSUE (one VALU and one scalar instruction per SIMD every 4 cycles, shared by
// the waves of the SIMD) and the 32-cycle dependent fp64 latency -- not flops.  512 threads; the upper triangle is
// enumerated bottom row first and dealt cyclically, entry e -> thread e % 512, register slot e / 512, so slot q of
// all threads is one band of adjacent rows.  A factorisation step publishes the pivot row into a fixed LDS row
// buffer (static read addresses), takes one barrier, and updates whole slot groups: per entry two ds_reads, one
// mul, one fma, no mask (an entry whose row is finished is dead: it has been published and may be overwritten
// with garbage), one wave-uniform test per GROUP of four slots, all loads of a group issued before their first
// use.  The inverse runs the same way bottom-up (see below).
// ------------------------------------------------------------------------------------------------
template <int EPT>
__global__ __launch_bounds__(CHOL_REG_THREADS, 2) void k_chol_reg(const double* __restrict__ G, int ldg, int k,
                                                               double* __restrict__ Rout, double* __restrict__ Rinv,
                                                               double* __restrict__ Rtot, double* __restrict__ Rtmp,
                                                               int ldo, int rtot_mode, int full_r, double shift_rel,
                                                               double pivot_tol, double* __restrict__ colnorm0,
                                                               double* __restrict__ rdiag,
                                                               hfmi_status_words* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);       // 32 doubles of reduction scratch
  double* diag0 = red + 32;                            // k original diagonal entries
  double* invd = diag0 + 256;                          // 1 / R_jj
  double* rb0 = invd + 256;                            // published row, two alternating buffers
  double* rb1 = rb0 + 256;
  double* M = rb1 + 256;                               // U, then R (upper triangle), row-major
  const int ldm = k | 1;
  constexpr int NT = CHOL_REG_THREADS;
  constexpr int GQ = 4;                                // slots per group
  constexpr int NG = (EPT + GQ - 1) / GQ;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  __shared__ int s_break;

  long long tk0 = clock64(), tk1, tk2, tk3, tk4;
  for (int i = tid; i < k; i += NT) {
    diag0[i] = G[i * ldg + i];
    if (rtot_mode == 1) colnorm0[i] = sqrt(fmax(diag0[i], 0.0));  // norms of the ORIGINAL columns (first pass)
  }
  for (int i = tid; i < 512; i += NT) rb0[i] = 0.0;               // both row buffers
  __syncthreads();
  for (int i = tid; i < k; i += NT) invd[i] = diag0[i] > 0.0 ? fast_rsqrt(diag0[i]) : 0.0;
  __syncthreads();
  double dev = 0.0, tr = 0.0;
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) {
      const double g = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
      const double x = g * invd[i] * invd[j] - (i == j ? 1.0 : 0.0);
      dev += x * x;
      if (i == j) tr += g;
    }
  dev = block_sum(dev, red);
  tr = block_sum(tr, red);
  tk1 = clock64();

  // Near-orthonormal input (the polishing pass of Cholesky-QR2: G = D^1/2 (I + E) D^1/2 with |E| ~ eps cond^2): the
  // sequential factorisation is replaced by the first-order inverse square root X = D^-1/2 (I - E/2), for which
  // X^T G X = I - 3/4 E^2 + O(E^3) -- below 1e-14 for |E|_F < 1e-7.  X is not triangular, so this is only taken when
  // the caller does not ask for the triangular factor (the fused solves: only the span and the B-orthonormality of Q
  // matter there).  k = 138: 0.27 ms -> 0.02 ms for the second pass of every solve.
  if (!full_r && dev < 1e-14) {
    bool pos = true;
    for (int i = tid; i < k; i += NT) pos = pos && diag0[i] > 0.0;
    if (__syncthreads_and(pos ? 1 : 0)) {
      for (int i = wave; i < k; i += nw) {
        const double di = invd[i];
        for (int j = lane; j < k; j += 64) {
          const double g = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
          const double dj = invd[j];
          const double e = g * di * dj - (i == j ? 1.0 : 0.0);
          const double id = (i == j) ? 1.0 : 0.0;
          Rinv[i * ldo + j] = di * (id - 0.5 * e);
          Rout[i * ldo + j] = (id + 0.5 * e) * diag0[j] * dj;          // (I + E/2) D^1/2, d^1/2 = d * d^-1/2
          if (i == j) rdiag[i] = (rtot_mode == 1 ? 1.0 : rdiag[i]) * (1.0 + 0.5 * e) * diag0[i] * di;
        }
      }
      if (tid == 0) {
        status->min_pivot_ratio = 1.0;
        status->gram_dev = sqrt(dev);
        status->shifted = 0;
        status->failed = 0;
        status->tick[0] = tk1 - tk0;
        status->tick[1] = 0;
        status->tick[2] = 0;
        status->tick[3] = clock64() - tk1;
        status->tick[4] = 3;
      }
      return;
    }
  }

  // owned entries: slot q holds cell e = tid + q * NT; rows counted from the bottom, m (m+1)/2 <= e < (m+1)(m+2)/2
  const int total = k * (k + 1) / 2;
  int oi[EPT], oc[EPT];   // row (clamped into the matrix for idle slots: they compute garbage nobody reads), column
  bool own[EPT];
  double v[EPT];
#pragma unroll
  for (int q = 0; q < EPT; ++q) {
    const int e = tid + q * NT;
    own[q] = e < total;
    const int ee = own[q] ? e : 0;
    int m = (int)((sqrtf(8.0f * (float)ee + 1.0f) - 1.0f) * 0.5f);
    while (m * (m + 1) / 2 > ee) --m;
    while ((m + 1) * (m + 2) / 2 <= ee) ++m;
    oi[q] = k - 1 - m;
    oc[q] = (k - 1 - m) + (ee - m * (m + 1) / 2);
    v[q] = 0.0;
  }

  int shifted = 0, failed = 0;
  double shift = 0.0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    shift = attempt ? shift_rel * tr : 0.0;
    if (tid == 0) s_break = 0;
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
      v[q] = 0.5 * (G[oi[q] * ldg + oc[q]] + G[oc[q] * ldg + oi[q]]);
      if (oi[q] == oc[q]) v[q] += shift;
    }
    // Unscaled (LDL^T-style) right-looking factorisation: U[i][c] = G[i][c] - sum_{j<i} U[j][i] U[j][c] / U[j][j];
    // R = diag(U)^{-1/2} U is formed by one scaling pass at the end.
    for (int j = 0; j < k; ++j) {
      double* rb = (j & 1) ? rb1 : rb0;
      const int m = k - 1 - j;                            // row j counted from the bottom
      const int e0 = m * (m + 1) / 2;                     // its cells are e0 .. e0 + m (k - j of them)
      const int qp0 = e0 / NT, qp1 = (e0 + m) / NT;       // the (at most two) slots that hold them
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (g * GQ <= qp1 && qp0 < g * GQ + GQ) {
#pragma unroll
          for (int q = g * GQ; q < g * GQ + GQ && q < EPT; ++q)
            if (own[q] && oi[q] == j) {                   // row j is final: publish it
              rb[oc[q]] = v[q];
              M[j * ldm + oc[q]] = v[q];
            }
        }
      __syncthreads();
      const double piv = rb[j];
      const double ref = diag0[j] + shift;
      if (!(piv > pivot_tol * ref) || !(ref > 0.0)) {     // uniform decision: every thread reads the same words
        if (tid == 0) s_break = 1;
        break;
      }
      const double inv = fast_rsqrt(piv);
      const double nrp = -(inv * inv);
      if (tid == 0) invd[j] = inv;
      // slots 0 .. qa-1 still hold rows > j (cells below row j are exactly e < e0)
      const int qa = (e0 + NT - 1) / NT;
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (g * GQ < qa) {
          double xa[GQ], xb[GQ];
#pragma unroll
          for (int u = 0; u < GQ; ++u)
            if (g * GQ + u < EPT) {
              xa[u] = rb[oi[g * GQ + u]];
              xb[u] = rb[oc[g * GQ + u]];
            }
#pragma unroll
          for (int u = 0; u < GQ; ++u)
            if (g * GQ + u < EPT) v[g * GQ + u] = fma(xa[u] * nrp, xb[u], v[g * GQ + u]);
        }
    }
    __syncthreads();
    if (!s_break) break;
    if (attempt == 0) shifted = 1;
    else failed = 1;
    __syncthreads();
  }
  if (failed) {
    if (tid == 0) {
      status->min_pivot_ratio = 0.0;
      status->gram_dev = sqrt(dev);
      status->shifted = shifted;
      status->failed = 1;
    }
    return;
  }
  // smallest pivot relative to the (shifted) original diagonal: piv_j = 1 / invd_j^2
  double ratio = 1e300;
  for (int j = tid; j < k; j += NT) ratio = fmin(ratio, 1.0 / (invd[j] * invd[j] * (diag0[j] + shift)));
  const double min_ratio = block_min(ratio, red);
  // R = diag(U)^{-1/2} U
  for (int i = wave; i < k; i += nw) {
    const double sc = invd[i];
    for (int j = i + lane; j < k; j += 64) M[i * ldm + j] *= sc;
  }
  for (int i = tid; i < 512; i += NT) rb0[i] = 0.0;  // the inverse relies on zeros left of the published row
  __syncthreads();
  tk2 = clock64();
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) Rout[i * ldo + j] = (j >= i) ? M[i * ldm + j] : 0.0;
  // Inverse X = R^-1, right-looking and bottom-up: once row l of X is final (x_ll = 1/R_ll, x_lc = -acc / R_ll) it
  // goes to the output and into the row buffer, and every entry (i, c) with i < l accumulates R[i][l] x_lc -- x_lc
  // reads as 0 for c < l (the buffers are zeroed and row l only writes c >= l), finished entries (i >= l) are
  // dead, so again no masks.
#pragma unroll
  for (int q = 0; q < EPT; ++q) v[q] = 0.0;
  for (int l = k - 1; l >= 0; --l) {
    double* xr = (l & 1) ? rb1 : rb0;
    const int m = k - 1 - l;
    const int e0 = m * (m + 1) / 2;
    const int qp0 = e0 / NT, qp1 = (e0 + m) / NT;
    const double il = invd[l];
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (g * GQ <= qp1 && qp0 < g * GQ + GQ) {
#pragma unroll
        for (int q = g * GQ; q < g * GQ + GQ && q < EPT; ++q)
          if (own[q] && oi[q] == l) {
            const double x = (oc[q] == l) ? il : -il * v[q];
            xr[oc[q]] = x;
            Rinv[l * ldo + oc[q]] = x;
          }
      }
    __syncthreads();
    // slots qs .. EPT-1 hold rows < l (cells of rows above row l are exactly e >= e0 + m + 1)
    const int qs = (e0 + m + 1) / NT;
    const double* ml = M + l;
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (g * GQ + GQ > qs) {
        double xa[GQ], xb[GQ];
#pragma unroll
        for (int u = 0; u < GQ; ++u)
          if (g * GQ + u < EPT) {
            xa[u] = ml[oi[g * GQ + u] * ldm];
            xb[u] = xr[oc[g * GQ + u]];
          }
#pragma unroll
        for (int u = 0; u < GQ; ++u)
          if (g * GQ + u < EPT) v[g * GQ + u] = fma(xa[u], xb[u], v[g * GQ + u]);
      }
  }
  __syncthreads();
  tk3 = clock64();
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < i; j += 64) Rinv[i * ldo + j] = 0.0;
  // diagonal of the running product R = R_p ... R_1 (its ratio to the original column norms exposes
  // numerically dependent columns); the full product only when the caller wants R
  for (int i = tid; i < k; i += NT) rdiag[i] = (rtot_mode == 1 ? 1.0 : rdiag[i]) * M[i * ldm + i];
  if (full_r) {
    if (rtot_mode == 1) {
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) Rtot[i * ldo + j] = (j >= i) ? M[i * ldm + j] : 0.0;
    } else {
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) {
          double acc = 0.0;
          if (j >= i)
            for (int l = i; l <= j; ++l) acc += M[i * ldm + l] * Rtot[l * ldo + j];
          Rtmp[i * ldo + j] = acc;
        }
      __syncthreads();
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) Rtot[i * ldo + j] = Rtmp[i * ldo + j];
    }
  }
  tk4 = clock64();
  if (tid == 0) {
    status->min_pivot_ratio = min_ratio;
    status->gram_dev = sqrt(dev);
    status->shifted = shifted;
    status->failed = 0;
    status->tick[0] = tk1 - tk0;  // load + defect
    status->tick[1] = tk2 - tk1;  // Cholesky
    status->tick[2] = tk3 - tk2;  // inverse
    status->tick[3] = tk4 - tk3;  // outputs + R product
    status->tick[4] = 0;
  }
}

// ------------------------------------------------------------------------------------------------
// k_chol_tile: k_chol_reg with a two-dimensional ownership map.  With the entries dealt cyclically every entry of a
// thread needs its own two LDS words per step (the pivot row at its row and at its column): 2 EPT reads per step,
// 164 KB per step at k = 138 -- the factorisation was LDS-bandwidth bound (1.3 k of its 2 k cycles per step).  Here a
// thread owns a TR x TC rectangle of the upper triangle and reads TR + TC words for TR TC entries (10 instead of 50
// at k = 138); everything else is the same algorithm: unscaled right-looking factorisation with the pivot row
// published through alternating LDS row buffers, one barrier per column, dead entries instead of masks, and the
// inverse accumulated the same way bottom-up.
// ------------------------------------------------------------------------------------------------
// NTHR = 512, MG = false: k <= 139, the factor in LDS.  NTHR = 1024, MG = true (round 3): 140 <= k <= 256, where k x k doubles
// no longer fit the 160 KB of LDS: the tiles still live in registers (6 x 6 per thread at k = 256), only the copy of the
// factor that the inverse reads column by column goes to an L2-resident global slot, and those reads do not depend on the
// step's barrier, so they are issued one step ahead.  (The generic k_chol_inv with its FLAT accesses took 3.0 ms at k = 256.)
template <int TR, int TC, int NTHR = CHOL_REG_THREADS, bool MG = false>
__global__ __launch_bounds__(NTHR, NTHR == 1024 ? 1 : 2) void k_chol_tile(const double* __restrict__ G, int ldg, int k,
                                                                double* __restrict__ Rout, double* __restrict__ Rinv,
                                                                double* __restrict__ Rtot, double* __restrict__ Rtmp,
                                                                int ldo, int rtot_mode, int full_r, double shift_rel,
                                                                double pivot_tol, double* __restrict__ colnorm0,
                                                                double* __restrict__ rdiag,
                                                                hfmi_status_words* __restrict__ status,
                                                                double* __restrict__ Mglob) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = reinterpret_cast<double*>(smem);       // 32 doubles of reduction scratch
  double* diag0 = red + 32;                            // k original diagonal entries
  double* invd = diag0 + 256;                          // 1 / R_jj
  double* rb0 = invd + 256;                            // published row, two alternating buffers
  double* rb1 = rb0 + 256;
  // U, then R (upper triangle), row-major: in LDS, or (MG) in the global slot -- two differently typed names so that every
  // access compiles to ds_* or global_* and never to FLAT
  double* Ml = rb1 + 256;
  const int ldm = MG ? ldo : (k | 1);
  constexpr int NT = NTHR;
#define CHOL_M(idx) (*(MG ? (Mglob + (idx)) : (Ml + (idx))))
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  __shared__ int s_break;

  long long tk0 = clock64(), tk1, tk2, tk3, tk4;
  for (int i = tid; i < k; i += NT) {
    diag0[i] = G[i * ldg + i];
    if (rtot_mode == 1) colnorm0[i] = sqrt(fmax(diag0[i], 0.0));  // norms of the ORIGINAL columns (first pass)
  }
  for (int i = tid; i < 512; i += NT) rb0[i] = 0.0;               // both row buffers
  __syncthreads();
  for (int i = tid; i < k; i += NT) invd[i] = diag0[i] > 0.0 ? fast_rsqrt(diag0[i]) : 0.0;
  __syncthreads();
  double dev = 0.0, tr = 0.0;
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) {
      const double g = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
      const double x = g * invd[i] * invd[j] - (i == j ? 1.0 : 0.0);
      dev += x * x;
      if (i == j) tr += g;
    }
  dev = block_sum(dev, red);
  tr = block_sum(tr, red);
  tk1 = clock64();

  // near-orthonormal input and no triangular factor wanted: first-order inverse square root (see k_chol_reg)
  if (!full_r && dev < 1e-14) {
    bool pos = true;
    for (int i = tid; i < k; i += NT) pos = pos && diag0[i] > 0.0;
    if (__syncthreads_and(pos ? 1 : 0)) {
      for (int i = wave; i < k; i += nw) {
        const double di = invd[i];
        for (int j = lane; j < k; j += 64) {
          const double g = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
          const double dj = invd[j];
          const double e = g * di * dj - (i == j ? 1.0 : 0.0);
          const double id = (i == j) ? 1.0 : 0.0;
          Rinv[i * ldo + j] = di * (id - 0.5 * e);
          Rout[i * ldo + j] = (id + 0.5 * e) * diag0[j] * dj;
          if (i == j) rdiag[i] = (rtot_mode == 1 ? 1.0 : rdiag[i]) * (1.0 + 0.5 * e) * diag0[i] * di;
        }
      }
      if (tid == 0) {
        status->min_pivot_ratio = 1.0;
        status->gram_dev = sqrt(dev);
        status->shifted = 0;
        status->failed = 0;
        status->tick[0] = tk1 - tk0;
        status->tick[1] = 0;
        status->tick[2] = 0;
        status->tick[3] = clock64() - tk1;
        status->tick[4] = 3;
      }
      return;
    }
  }

  // this thread's tile: the tid-th rectangle (tile row I ascending, then tile column J) that touches the upper triangle
  const int ntr = (k + TR - 1) / TR, ntc = (k + TC - 1) / TC;
  bool own = false;
  int r0 = 0, c0 = 0;
  {
    int left = tid;
    for (int I = 0; I < ntr; ++I) {
      int jmin = (I * TR - TC + 1 + TC - 1) / TC;          // smallest J with J TC + TC - 1 >= I TR
      if (I * TR - TC + 1 <= 0) jmin = 0;
      const int cnt = ntc - jmin;
      if (cnt <= 0) continue;
      if (left < cnt) {
        own = true;
        r0 = I * TR;
        c0 = (jmin + left) * TC;
        break;
      }
      left -= cnt;
    }
  }
  double v[TR][TC];

  int shifted = 0, failed = 0;
  double shift = 0.0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    shift = attempt ? shift_rel * tr : 0.0;
    if (tid == 0) s_break = 0;
#pragma unroll
    for (int a = 0; a < TR; ++a)
#pragma unroll
      for (int b = 0; b < TC; ++b) {
        const int r = r0 + a, c = c0 + b;
        double g = 0.0;
        if (own && r < k && c < k && c >= r) g = 0.5 * (G[r * ldg + c] + G[c * ldg + r]) + (r == c ? shift : 0.0);
        v[a][b] = g;
      }
    for (int j = 0; j < k; ++j) {
      double* rb = (j & 1) ? rb1 : rb0;
      if (own && j >= r0 && j < r0 + TR) {                 // row j is final: publish it
#pragma unroll
        for (int a = 0; a < TR; ++a)
          if (r0 + a == j) {
#pragma unroll
            for (int b = 0; b < TC; ++b) {
              const int c = c0 + b;
              if (c >= j && c < k) {
                rb[c] = v[a][b];
                CHOL_M(j * ldm + c) = v[a][b];
              }
            }
          }
      }
      __syncthreads();
      const double piv = rb[j];
      const double ref = diag0[j] + shift;
      if (!(piv > pivot_tol * ref) || !(ref > 0.0)) {     // uniform decision: every thread reads the same words
        if (tid == 0) s_break = 1;
        break;
      }
      const double inv = fast_rsqrt(piv);
      const double nrp = -(inv * inv);
      if (tid == 0) invd[j] = inv;
      if (own && r0 + TR - 1 > j) {                        // the tile still holds rows below row j
        double xa[TR], xb[TC];
#pragma unroll
        for (int a = 0; a < TR; ++a) xa[a] = rb[r0 + a];
#pragma unroll
        for (int b = 0; b < TC; ++b) xb[b] = rb[c0 + b];
#pragma unroll
        for (int a = 0; a < TR; ++a) {
          const double f = xa[a] * nrp;
#pragma unroll
          for (int b = 0; b < TC; ++b) v[a][b] = fma(f, xb[b], v[a][b]);
        }
      }
    }
    __syncthreads();
    if (!s_break) break;
    if (attempt == 0) shifted = 1;
    else failed = 1;
    __syncthreads();
  }
  if (failed) {
    if (tid == 0) {
      status->min_pivot_ratio = 0.0;
      status->gram_dev = sqrt(dev);
      status->shifted = shifted;
      status->failed = 1;
    }
    return;
  }
  double ratio = 1e300;
  for (int j = tid; j < k; j += NT) ratio = fmin(ratio, 1.0 / (invd[j] * invd[j] * (diag0[j] + shift)));
  const double min_ratio = block_min(ratio, red);
  // R = diag(U)^{-1/2} U
  for (int i = wave; i < k; i += nw) {
    const double sc = invd[i];
    for (int j = i + lane; j < k; j += 64) CHOL_M(i * ldm + j) *= sc;
  }
  for (int i = tid; i < 512; i += NT) rb0[i] = 0.0;  // the inverse relies on zeros left of the published row
  __syncthreads();
  tk2 = clock64();
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < k; j += 64) Rout[i * ldo + j] = (j >= i) ? CHOL_M(i * ldm + j) : 0.0;
  // Inverse X = R^-1, right-looking and bottom-up (see k_chol_reg)
#pragma unroll
  for (int a = 0; a < TR; ++a)
#pragma unroll
    for (int b = 0; b < TC; ++b) v[a][b] = 0.0;
  double xan[TR];                                        // column l of R at this tile's rows, fetched one step ahead
#pragma unroll
  for (int a = 0; a < TR; ++a) {
    const int r = r0 + a < k ? r0 + a : k - 1;
    xan[a] = CHOL_M(r * ldm + (k - 1));
  }
  for (int l = k - 1; l >= 0; --l) {
    double* xr = (l & 1) ? rb1 : rb0;
    const double il = invd[l];
    if (own && l >= r0 && l < r0 + TR) {
#pragma unroll
      for (int a = 0; a < TR; ++a)
        if (r0 + a == l) {
#pragma unroll
          for (int b = 0; b < TC; ++b) {
            const int c = c0 + b;
            if (c >= l && c < k) {
              const double x = (c == l) ? il : -il * v[a][b];
              xr[c] = x;
              Rinv[l * ldo + c] = x;
            }
          }
        }
    }
    __syncthreads();
    double xa[TR];
#pragma unroll
    for (int a = 0; a < TR; ++a) {
      xa[a] = xan[a];
      const int r = r0 + a < k ? r0 + a : k - 1;
      xan[a] = CHOL_M(r * ldm + (l > 0 ? l - 1 : 0));     // R is final: this read does not wait for the next barrier
    }
    if (own && r0 < l) {                                   // the tile still holds rows above row l
      double xb[TC];
#pragma unroll
      for (int b = 0; b < TC; ++b) xb[b] = xr[c0 + b];
#pragma unroll
      for (int a = 0; a < TR; ++a)
#pragma unroll
        for (int b = 0; b < TC; ++b) v[a][b] = fma(xa[a], xb[b], v[a][b]);
    }
  }
  __syncthreads();
  tk3 = clock64();
  for (int i = wave; i < k; i += nw)
    for (int j = lane; j < i; j += 64) Rinv[i * ldo + j] = 0.0;
  for (int i = tid; i < k; i += NT) rdiag[i] = (rtot_mode == 1 ? 1.0 : rdiag[i]) * CHOL_M(i * ldm + i);
  if (full_r) {
    if (rtot_mode == 1) {
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) Rtot[i * ldo + j] = (j >= i) ? CHOL_M(i * ldm + j) : 0.0;
    } else {
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) {
          double acc = 0.0;
          if (j >= i)
            for (int l = i; l <= j; ++l) acc += CHOL_M(i * ldm + l) * Rtot[l * ldo + j];
          Rtmp[i * ldo + j] = acc;
        }
      __syncthreads();
      for (int i = wave; i < k; i += nw)
        for (int j = lane; j < k; j += 64) Rtot[i * ldo + j] = Rtmp[i * ldo + j];
    }
  }
  tk4 = clock64();
  if (tid == 0) {
    status->min_pivot_ratio = min_ratio;
    status->gram_dev = sqrt(dev);
    status->shifted = shifted;
    status->failed = 0;
    status->tick[0] = tk1 - tk0;
    status->tick[1] = tk2 - tk1;
    status->tick[2] = tk3 - tk2;
    status->tick[3] = tk4 - tk3;
    status->tick[4] = 0;
  }
}
#undef CHOL_M

// the instances of a plan (HFMI_CHOL_*_CASES, hfmi_small_plan.h); null: not compiled
typedef decltype(&k_chol_reg<1>) chol_reg_fn;
static chol_reg_fn chol_reg_kernel(int ept) {
  switch (ept) {
#define X(E) \
  case E:    \
    return k_chol_reg<E>;
    HFMI_CHOL_REG_CASES(X)
#undef X
  }
  return nullptr;
}
typedef decltype(&k_chol_tile<1, 2>) chol_tile_fn;
static chol_tile_fn chol_tile_kernel(int family, int tr, int tc) {
  switch ((family == SF_CHOL_BIG ? 100 : 0) + 10 * tr + tc) {
#define X(A, B)        \
  case 10 * (A) + (B): \
    return k_chol_tile<A, B>;
    HFMI_CHOL_TILE_CASES(X)
#undef X
#define X(A, B)              \
  case 100 + 10 * (A) + (B): \
    return k_chol_tile<A, B, 1024, true>;
    HFMI_CHOL_BIG_CASES(X)
#undef X
  }
  return nullptr;
}

int launch_chol_inv(hfmi_ctx* ctx, int k, int slot_gram, int slot_r, int slot_rinv, int slot_rtot, int rtot_mode,
                    int full_r, double shift_rel, double pivot_tol) {
  if (k < 1 || k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "chol_inv: k=%d out of range", k);
  const small_plan p = chol_plan(k, small_knobs_ref());
  if (!p.route) return launch_chol_mfma(ctx, k, slot_gram, slot_r, slot_rinv, slot_rtot, rtot_mode, full_r, shift_rel, pivot_tol);
  if (pivot_tol <= 0.0) pivot_tol = 64.0 * k * EPS_D;
  const small_launch& L = p.launch[0];
  double *G = sm_ptr(ctx, slot_gram), *R = sm_ptr(ctx, slot_r), *Rinv = sm_ptr(ctx, slot_rinv), *Rtot = sm_ptr(ctx, slot_rtot);
  double *Rtmp = sm_ptr(ctx, SM_TMP2), *colnorm0 = sm_ptr(ctx, SM_AUX), *rdiag = sm_ptr(ctx, SM_AUX) + SM_LD;
  if (L.family == SF_CHOL_REG) {
    const chol_reg_fn kern = chol_reg_kernel(L.t[0]);
    if (!kern) HFMI_FAIL(HFMI_ERR_INVALID, "chol_inv: no k_chol_reg<%d>", L.t[0]);
    HFMI_TRY(small_raise_lds((const void*)kern, L));
    hipLaunchKernelGGL(kern, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, G, SM_LD, k, R, Rinv, Rtot, Rtmp, SM_LD, rtot_mode, full_r,
                       shift_rel, pivot_tol, colnorm0, rdiag, ctx->status_dev);
  } else if (L.family == SF_CHOL_TILE || L.family == SF_CHOL_BIG) {
    const chol_tile_fn kern = chol_tile_kernel(L.family, L.t[0], L.t[1]);
    if (!kern) HFMI_FAIL(HFMI_ERR_INVALID, "chol_inv: no k_chol_tile<%d, %d> at %d threads", L.t[0], L.t[1], L.threads);
    HFMI_TRY(small_raise_lds((const void*)kern, L));
    hipLaunchKernelGGL(kern, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, G, SM_LD, k, R, Rinv, Rtot, Rtmp, SM_LD, rtot_mode, full_r,
                       shift_rel, pivot_tol, colnorm0, rdiag, ctx->status_dev, L.family == SF_CHOL_BIG ? sm_ptr(ctx, SM_TMP) : (double*)nullptr);
  } else {
    HFMI_TRY(small_raise_lds((const void*)k_chol_inv, L));
    hipLaunchKernelGGL(k_chol_inv, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, G, SM_LD, k, R, Rinv, Rtot, Rtmp, SM_LD, rtot_mode,
                       full_r, shift_rel, pivot_tol, sm_ptr(ctx, SM_TMP), p.use_lds, colnorm0, rdiag, ctx->status_dev);
  }
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
