// Blocked LU with partial pivoting of the single pass, m <= 256, ONE workgroup, fp64 throughout; launch_lu_solve launches what
// lu_plan (hfmi_small_plan.h) says.
#include "hfmi_internal.h"
#include "hfmi_small_dev.h"
#include "hfmi_small_plan.h"

// ------------------------------------------------------------------------------------------------
// k_lu_solve: X = W^-1 Z for small square W, Z (m <= 256) by LU with partial pivoting on ONE workgroup -- the
// np.linalg.solve(Wt, Zt) of hippylib's singlePass[G] -- and optionally T = (X + X^T) / 2 straight into the
// eigensolver's slot, so the single-pass Rayleigh-Ritz matrix never crosses PCIe.
//
// Right-looking blocked LU (LAPACK dgetrf's recurrence; CPU twin: tests/helpers/lu_small_twin.py), with the m right-hand
// sides carried as extra columns to the right of W so that the forward substitution is part of the elimination:
//   for each panel of nb columns starting at j0:
//     1. the panel W[j0:m, j0:j0+nb] is loaded into LDS and factored there column by column (pivot = first row of
//        largest |entry|, row swap inside the panel, multipliers, rank-1 update of the panel's remaining columns);
//     2. the panel goes back to the global working copy; the panel's row swaps are applied to every column to its right
//        (the rest of W and all of Z; the L columns to its left are never read again and keep their rows);
//     3. U12 = L11^-1 A12 on those columns (unit lower triangular solve, one barrier per row of L11);
//     4. trailing update A22 -= L21 U12 (L21 from LDS, U12 from the L2-resident global copy).
//   then back substitution with U, T = (X + X^T) / 2.
// lu_panel_width() picks nb: the whole matrix (nb = m, one panel, no trailing update) while m x (m|1) doubles fit the LDS
// next to the bookkeeping (m <= 141), otherwise the widest multiple of 16 that fits (m = 256: nb = 64).
// Status words: min_pivot_ratio = min |pivot|, gram_dev = max |pivot|, failed = 1 for non-finite input, 2 for a pivot
// <= m eps max |pivot| (numerically singular W), 3 for a non-finite pivot or solution entry produced by the elimination
// (overflow of finite input).  On failure T is written as zeros, so nothing downstream sees a NaN;
// the host turns the status into HFMI_ERR_NUMERIC.
// All memory writes are plain vector / LDS stores.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LU_THREADS) void k_lu_solve(const double* __restrict__ W, const double* __restrict__ Z, int ld, int m,
                                                         int nb, double* __restrict__ A, double* __restrict__ X,
                                                         double* __restrict__ T, hfmi_status_words* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double lu_smem[];
  double* red_a = lu_smem;                  // 16 wave maxima |v|
  double* red_v = red_a + 32;               // 16 signed values
  int* red_i = reinterpret_cast<int*>(red_v + 32);   // 16 row indices (64 doubles' room)
  double* invd = red_v + 96;                // 1 / U_jj (0 for a zero pivot)
  int* piv = reinterpret_cast<int*>(invd + 256);     // global row swapped with row j at step j
  double* Pn = invd + 256 + 128;            // the panel: rows j0..m-1, nb columns, ld ldp
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const int ldp = nb | 1;
  __shared__ int s_bad;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // working copies: A <- W, X <- Z; non-finite input is reported, not propagated
  int bad = 0;
  for (int e = tid; e < m * m; e += nthr) {
    const int i = e / m, j = e - i * m;
    const double w = W[i * ld + j], z = Z[i * ld + j];
    if (!isfinite(w) || !isfinite(z)) bad = 1;
    A[i * ld + j] = w;
    X[i * ld + j] = z;
  }
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  double pmin = INFINITY, pmax = 0.0;       // meaningful on thread 0
  bool pivot_nonfinite = false;             // thread 0
  if (s_bad == 0) {
    for (int j0 = 0; j0 < m; j0 += nb) {
      const int nbc = min(nb, m - j0), rows = m - j0;
      const int na = m - j0 - nbc, ncr = na + m;   // columns right of the panel: na of W, then the m of Z
      auto right = [&](int row, int c) -> double* { return c < na ? A + row * ld + j0 + nbc + c : X + row * ld + (c - na); };
      // 1. panel into LDS, factored in place
      for (int e = tid; e < rows * nbc; e += nthr) {
        const int r = e / nbc, c = e - r * nbc;
        Pn[r * ldp + c] = A[(j0 + r) * ld + j0 + c];
      }
      __syncthreads();
      for (int jj = 0; jj < nbc; ++jj) {
        // pivot: first row of largest |entry| in column jj at or below the diagonal (rows <= 256 < nthr: one row per thread)
        const int r = jj + tid;
        double va = -1.0, vv = 0.0;
        int vi = 0x7fffffff;
        if (r < rows) {
          vv = Pn[r * ldp + jj];
          va = fabs(vv);
          vi = r;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double oa = __shfl_down(va, off, 64), ov = __shfl_down(vv, off, 64);
          const int oi = __shfl_down(vi, off, 64);
          if (oa > va || (oa == va && oi < vi)) {
            va = oa;
            vv = ov;
            vi = oi;
          }
        }
        if (lane == 0) {
          red_a[wave] = va;
          red_v[wave] = vv;
          red_i[wave] = vi;
        }
        __syncthreads();
        double ba = red_a[0], bv = red_v[0];
        int bi = red_i[0];
        for (int w = 1; w < nw; ++w)
          if (red_a[w] > ba || (red_a[w] == ba && red_i[w] < bi)) {
            ba = red_a[w];
            bv = red_v[w];
            bi = red_i[w];
          }
        if (bi != jj)
          for (int c = tid; c < nbc; c += nthr) {
            const double t0 = Pn[jj * ldp + c];
            Pn[jj * ldp + c] = Pn[bi * ldp + c];
            Pn[bi * ldp + c] = t0;
          }
        const double inv = (bv != 0.0) ? 1.0 / bv : 0.0;
        if (tid == 0) {
          piv[j0 + jj] = j0 + bi;
          invd[j0 + jj] = inv;
          pmin = fmin(pmin, ba);
          pmax = fmax(pmax, ba);
          if (!isfinite(bv)) pivot_nonfinite = true;
        }
        __syncthreads();
        // multipliers and rank-1 update: four lanes of one wave per row, so every lane of a row reads the unscaled
        // multiplier before the first lane overwrites it (LDS operations of a wave complete in order)
        const int rr = tid >> 2, sub = tid & 3;
        if (rr > jj && rr < rows) {
          const double l = Pn[rr * ldp + jj] * inv;
          for (int c = jj + 1 + sub; c < nbc; c += 4) Pn[rr * ldp + c] = fma(-l, Pn[jj * ldp + c], Pn[rr * ldp + c]);
          if (sub == 0) Pn[rr * ldp + jj] = l;
        }
        __syncthreads();
      }
      // 2. panel back to the working copy; the panel's row swaps on every column to its right
      for (int e = tid; e < rows * nbc; e += nthr) {
        const int r = e / nbc, c = e - r * nbc;
        A[(j0 + r) * ld + j0 + c] = Pn[r * ldp + c];
      }
      for (int c = tid; c < ncr; c += nthr)
        for (int jj = 0; jj < nbc; ++jj) {
          const int p = piv[j0 + jj];
          if (p != j0 + jj) {
            double* a = right(j0 + jj, c);
            double* b = right(p, c);
            const double t0 = *a;
            *a = *b;
            *b = t0;
          }
        }
      __syncthreads();
      // 3. U12 = L11^-1 A12 (unit lower), row t of L11 eliminated from the rows below it
      for (int t = 0; t + 1 < nbc; ++t) {
        const int nr = nbc - 1 - t;
        for (int e = tid; e < nr * ncr; e += nthr) {
          const int i = t + 1 + e / ncr, c = e % ncr;
          double* y = right(j0 + i, c);
          *y = fma(-Pn[i * ldp + t], *right(j0 + t, c), *y);
        }
        __syncthreads();
      }
      // 4. trailing update A22 -= L21 U12
      if (rows > nbc) {
        for (int e = tid; e < (rows - nbc) * ncr; e += nthr) {
          const int i = nbc + e / ncr, c = e % ncr;
          double* y = right(j0 + i, c);
          double acc = *y;
          for (int t = 0; t < nbc; ++t) acc = fma(-Pn[i * ldp + t], *right(j0 + t, c), acc);
          *y = acc;
        }
        __syncthreads();
      }
    }
    // back substitution U X = Y: step t removes the (final) row t from the rows above it; rows scaled by 1 / U_tt at the end
    for (int t = m - 1; t > 0; --t) {
      const double it = invd[t];
      for (int e = tid; e < t * m; e += nthr) {
        const int i = e / m, c = e - i * m;
        X[i * ld + c] = fma(-A[i * ld + t], X[t * ld + c] * it, X[i * ld + c]);
      }
      __syncthreads();
    }
    // finite input can still overflow during the elimination: a non-finite pivot or solution entry is failure 3
    // (fmin / fmax above drop NaN, so the pivot test alone would not see it)
    int nf = 0;
    for (int e = tid; e < m * m; e += nthr) {
      const int i = e / m, c = e - i * m;
      const double x = X[i * ld + c] * invd[i];
      X[i * ld + c] = x;
      if (!isfinite(x)) nf = 1;
    }
    if (nf) atomicOr(&s_bad, 1);
    __syncthreads();
    if (tid == 0) {
      const int code = (s_bad || pivot_nonfinite) ? 3 : !(pmin > (double)m * EPS_D * pmax) ? 2 : 0;
      s_bad = code;
      status->min_pivot_ratio = pmin;
      status->gram_dev = pmax;
      status->failed = code;
    }
    __syncthreads();
  } else if (tid == 0) {
    status->min_pivot_ratio = 0.0;
    status->gram_dev = 0.0;
    status->failed = 1;
  }
  if (tid == 0) {
    status->shifted = 0;
    status->offdiag = 0.0;
    status->sweeps = 0;
  }
  if (T) {   // zero padded to a multiple of 16 rows and columns, like a matrix uploaded from the host
    const int mp = min((m + 15) & ~15, ld);
    for (int e = tid; e < mp * mp; e += nthr) {
      const int i = e / mp, j = e - i * mp;
      T[i * ld + j] = (s_bad || i >= m || j >= m) ? 0.0 : 0.5 * (X[i * ld + j] + X[j * ld + i]);
    }
  }
}

int launch_lu_solve(hfmi_ctx* ctx, int m, int slot_w, int slot_z, int slot_a, int slot_x, int slot_t) {
  if (m < 1 || m > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "lu_solve: m=%d out of range [1,%d]", m, SM_MAXK);
  const small_plan p = lu_plan(m);
  const small_launch& L = p.launch[0];
  HFMI_TRY(small_raise_lds((const void*)k_lu_solve, L));
  hipLaunchKernelGGL(k_lu_solve, dim3(L.grid), dim3(L.threads), L.lds, ctx->stream, sm_ptr(ctx, slot_w), sm_ptr(ctx, slot_z), SM_LD, m, p.nb,
                     sm_ptr(ctx, slot_a), sm_ptr(ctx, slot_x), slot_t >= 0 ? sm_ptr(ctx, slot_t) : (double*)nullptr, ctx->status_dev);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
