// M^-1 on a block by Jacobi-preconditioned CHEBYSHEV iteration (prior.Msolver behind hp.Solver2Operator in
// hp.doublePassG(KLE_Operator, prior.M, prior.Msolver, ...), KLEProjector.py:163-164; the mass-orthogonal QR applies it
// once per solve to an N x k block), the smoother of the V-cycle (hfmi_amg.hip), and the per-column reductions over row-major
// arrays that both need.  The decisions -- the recurrence, how many steps, when a matrix goes to CG for good, the bracket of the
// spectrum, which step kernel on which grid -- are hfmi_spsolve_rules.h's; this unit launches what they say.
//
// Why not the block CG (hfmi_sparse.hip; kept: it is the fallback): per iteration CG needs two global reductions -- five
// launches, eleven passes over N x k blocks, a host look at the residual every fourth iteration -- and its SpMM with one
// thread per ROW gathers 8 bytes per lane from k different vectors (1.5 TB/s on config 2 while the elementwise kernels beside
// it run at 6 TB/s out of the Infinity Cache).  Chebyshev needs no inner products at all: ONE kernel per iteration, six
// passes, nothing for the host to wait for.
//
// Layout: the iteration works on a ROW-MAJOR copy of the block (entry (row, j) at [row * k + j]; two transposes per
// solve): with lanes mapped to the k columns of one row every access is a contiguous run of the row -- the gathers of
// the neighbour rows of a sparse-matrix row included -- and the matrix entries of that row are the same for all its
// lanes (broadcast loads).  Any CSR matrix, no ELL image needed.
//
//   x_0 = 0, x_1 = D^-1 b / theta;  x_{n+1} = x_n + c1 (x_n - x_{n-1}) + c2 D^-1 (b - A x_n)      (cheb_recurrence)
// -- the three-term form of the iteration: the residual is recomputed from b in every step (no residual or direction
// arrays, no drift), x_{n+1} overwrites x_{n-1} in place, and a step reads b, x_n (with its neighbour rows), x_{n-1} and
// writes x_{n+1}: FOUR passes over three N x k arrays -- 200 MB on config 2, resident in the 256 MB Infinity Cache.
// [lmin, lmax] bracket the spectrum of D^-1 A (cheb_estimate below: Gershgorin from above, Lanczos of a scalar CG run from
// below).
#include <algorithm>
#include <cmath>

#include "hfmi_internal.h"
#include "hfmi_rm_dev.h"

namespace {
// x_1 = D^-1 B / theta  (x_0 = 0 is never stored: the first step runs with c1 = 0 ... see launch_cheb_step)
__global__ __launch_bounds__(256) void k_cheb_first(const double* __restrict__ B, double* __restrict__ X1, double* __restrict__ X0,
                                                   const double* __restrict__ inv_diag, int64_t nrows, int k, double inv_theta) {
  const rm_map m = rm_thread(k);
  for (int64_t r0 = (int64_t)blockIdx.x * m.rows_per_pass; r0 < nrows; r0 += (int64_t)gridDim.x * m.rows_per_pass) {
    const int64_t row = r0 + m.rl;
    if (!m.live || row >= nrows) continue;
    const double s = inv_diag[row] * inv_theta;
    for (int j = m.j0; j < k; j += m.jstep) {
      const int64_t e = row * k + j;
      X1[e] = s * B[e];
      X0[e] = 0.0;
    }
  }
}

// One step of the three-term iteration, ONE WAVE PER ROW (k even): lane l holds columns 2l, 2l+1 as one 16-byte access, so the
// gather of a neighbour row is one instruction for up to 128 columns, and the row's (column, value) pairs are wave-uniform:
// scalar loads, no vector-memory traffic for the matrix.  UNR rows per wave for memory-level parallelism.
//   RESID = false:  Xp <- Xc + c1 (Xc - Xp) + c2 D^-1 (B - A Xc)      (Xp holds x_{n-1} on entry, x_{n+1} on exit)
//   RESID = true:   Xp <- B - A Xc                                     (the true residual, for the convergence check)
typedef double d2v __attribute__((ext_vector_type(2)));
template <bool RESID, int UNR>
__global__ __launch_bounds__(256) void k_cheb_step_wave(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                       const double* __restrict__ data, const double* __restrict__ inv_diag,
                                                       int64_t nrows, int k, const double* __restrict__ B, const double* __restrict__ Xc,
                                                       double* __restrict__ Xp, double c1, double c2) {
  // the matrix through the constant address space: with wave-uniform addresses the compiler then issues scalar loads (it will
  // not for plain global pointers once the kernel also stores, restrict or not)
  typedef const int64_t __attribute__((address_space(4)))* cptr64;
  typedef const int32_t __attribute__((address_space(4)))* cptr32;
  typedef const double __attribute__((address_space(4)))* cptrd;
  const cptr64 c_indptr = (cptr64)indptr;
  const cptr32 c_indices = (cptr32)indices;
  const cptrd c_data = (cptrd)data, c_inv_diag = (cptrd)inv_diag;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Workgroup b works on the band of
  // rows that belongs to ITS XCD (b % 8), so that the neighbour rows a sparse row gathers were fetched by the same L2.
  const int64_t per_xcd = gridDim.x / 8;                       // the grid is a multiple of 8
  const int64_t logical = (int64_t)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  const int64_t row0 = (logical * 4 + wave) * UNR;             // this wave's UNR consecutive rows
  if (row0 >= nrows) return;
  const int half = k >> 1;
  for (int l0 = 0; l0 < half; l0 += 64) {                      // k <= 128: one trip
    const int l = l0 + lane;
    const bool on = l < half;
    const int64_t col2 = on ? 2 * l : 0;
    d2v ax[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) ax[u] = d2v{0.0, 0.0};
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t row = row0 + u < nrows ? row0 + u : nrows - 1;
      const int64_t zb = c_indptr[row], ze = c_indptr[row + 1];
      for (int64_t z = zb; z < ze; ++z) {
        const double v = c_data[z];
        const d2v g = *reinterpret_cast<const d2v*>(Xc + (int64_t)c_indices[z] * k + col2);
        ax[u] += v * g;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int64_t row = row0 + u;
      if (row >= nrows || !on) continue;
      const int64_t e = row * k + col2;
      const d2v res = *reinterpret_cast<const d2v*>(B + e) - ax[u];
      if (RESID) {
        *reinterpret_cast<d2v*>(Xp + e) = res;
      } else {
        const d2v xc = *reinterpret_cast<const d2v*>(Xc + e);
        const d2v xp = *reinterpret_cast<const d2v*>(Xp + e);
        *reinterpret_cast<d2v*>(Xp + e) = xc + c1 * (xc - xp) + (c2 * c_inv_diag[row]) * res;
      }
    }
  }
}

// the same step with one thread per (row, column) -- odd k, or k > 128 columns
template <bool RESID>
__global__ __launch_bounds__(256) void k_cheb_step(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                  const double* __restrict__ data, const double* __restrict__ inv_diag,
                                                  int64_t nrows, int k, const double* __restrict__ B, const double* __restrict__ Xc,
                                                  double* __restrict__ Xp, double c1, double c2) {
  const rm_map m = rm_thread(k);
  if (!m.live) return;
  const int64_t per_xcd = gridDim.x / 8;
  const int64_t logical = (int64_t)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
  const int64_t row = logical * m.rows_per_pass + m.rl;
  if (row >= nrows) return;
  const int64_t zb = indptr[row], ze = indptr[row + 1];
  const double s = c2 * inv_diag[row];
  for (int j = m.j0; j < k; j += m.jstep) {
    double ax = 0.0;
    for (int64_t z = zb; z < ze; ++z) ax += data[z] * Xc[(int64_t)indices[z] * k + j];
    const int64_t e = row * k + j;
    const double res = B[e] - ax;
    if (RESID) {
      Xp[e] = res;
    } else {
      const double xc = Xc[e];
      Xp[e] = xc + c1 * (xc - Xp[e]) + s * res;
    }
  }
}

// Per-column reductions over row-major (nrows x k) arrays: one partial per (column, workgroup), RM_CHUNKS workgroups whatever the
// shape, so the summation order does not vary.
//   RM_SQUARES:    part = <A_j, A_j>  (A read once)
//   RM_DOTS:       part = <A_j, B_j>
//   RM_CG_UPDATE:  alpha_j = rz_j / pap_j (0 when pap_j is not > 0 or alpha is not finite: that column is reported by the host,
//                  and no inf / NaN enters x); X += alpha P, R -= alpha AP; part = <R_j, R_j> (new R)
enum { RM_SQUARES, RM_DOTS, RM_CG_UPDATE };
template <int MODE>
__global__ __launch_bounds__(256) void k_rm_colred(int64_t nrows, int k, const double* __restrict__ A, const double* __restrict__ B,
                                                  double* __restrict__ X, double* __restrict__ R, const double* __restrict__ P,
                                                  const double* __restrict__ AP, const double* __restrict__ rz,
                                                  const double* __restrict__ pap, double* __restrict__ part) {
  __shared__ double sh[256];
  const rm_map m = rm_thread(k);
  for (int jb = 0; jb < k; jb += 256) {                // k <= 256: one trip
    double acc = 0.0;
    const int j = (k <= 256) ? m.j0 : jb + (int)threadIdx.x;
    if (m.live && j < k) {
      double alpha = 0.0;
      if (MODE == RM_CG_UPDATE) {
        const double pp = pap[j];
        alpha = pp > 0.0 ? rz[j] / pp : 0.0;
        if (!std::isfinite(alpha)) alpha = 0.0;
      }
      for (int64_t row = (int64_t)blockIdx.x * m.rows_per_pass + m.rl; row < nrows; row += (int64_t)gridDim.x * m.rows_per_pass) {
        const int64_t e = row * k + j;
        if (MODE == RM_CG_UPDATE) {
          X[e] += alpha * P[e];
          const double r = R[e] - alpha * AP[e];
          R[e] = r;
          acc += r * r;
        } else if (MODE == RM_DOTS) {
          acc += A[e] * B[e];
        } else {
          const double v = A[e];
          acc += v * v;
        }
      }
    }
    rm_col_partial(m, k, j, acc, sh, part);
  }
}
}  // namespace

unsigned rm_grid(hfmi_ctx* ctx, int64_t nrows, int k, int per_cu) {
  const int rows_per_pass = rm_rows_per_pass(k);
  int64_t g = (nrows + rows_per_pass - 1) / rows_per_pass;
  const int64_t cap = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * per_cu;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}
int launch_cheb_first(hfmi_ctx* ctx, const double* B, double* X1, double* X0, const double* inv_diag, int64_t nrows, int k, double inv_theta) {
  hipLaunchKernelGGL(k_cheb_first, dim3(rm_grid(ctx, nrows, k, 64)), dim3(256), 0, ctx->stream, B, X1, X0, inv_diag, nrows, k, inv_theta);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// one step (resid = false) or the residual B - A Xc into Xp (resid = true)
int launch_cheb_step(hfmi_ctx* ctx, const hfmi_csr* M, const double* B, const double* Xc, double* Xp, int k, double c1, double c2, bool resid) {
  const cheb_step_launch L = cheb_step_plan(M->nrows, k, resid, spsolve_knobs_ref());
#define HFMI_CHEB_LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), dim3((unsigned)L.grid), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->solve.inv_diag, M->nrows, k, B, Xc, Xp, c1, c2)
  if (!L.wave && resid) HFMI_CHEB_LAUNCH(k_cheb_step<true>);
  else if (!L.wave) HFMI_CHEB_LAUNCH(k_cheb_step<false>);
  else if (resid) HFMI_CHEB_LAUNCH(k_cheb_step_wave<true, 1>);
  else if (L.unr == 2) HFMI_CHEB_LAUNCH(k_cheb_step_wave<false, 2>);
  else if (L.unr == 4) HFMI_CHEB_LAUNCH(k_cheb_step_wave<false, 4>);
  else HFMI_CHEB_LAUNCH(k_cheb_step_wave<false, 1>);
#undef HFMI_CHEB_LAUNCH
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// The reductions (deterministic: fixed partition, fixed order).  part: room for k * RM_CHUNKS partials, or null for the context's.
template <int MODE>
static int launch_rm_colred(hfmi_ctx* ctx, int64_t nrows, int k, const double* A, const double* B, double* X, double* R, const double* P,
                            const double* AP, const double* rz, const double* pap, double* part, double* out) {
  void* ws = part;
  if (!ws) HFMI_TRY(ctx_ws(ctx, WS_PART, (size_t)k * RM_CHUNKS * sizeof(double), &ws));
  hipLaunchKernelGGL(k_rm_colred<MODE>, dim3(RM_CHUNKS), dim3(256), 0, ctx->stream, nrows, k, A, B, X, R, P, AP, rz, pap, (double*)ws);
  HIP_TRY(hipGetLastError());
  return launch_dots_final(ctx, (const double*)ws, RM_CHUNKS, k, out);
}
int launch_rm_colsq(hfmi_ctx* ctx, const double* A, int64_t nrows, int k, double* part, double* out) {
  return launch_rm_colred<RM_SQUARES>(ctx, nrows, k, A, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, part, out);
}
int launch_rm_coldots(hfmi_ctx* ctx, const double* A, const double* B, int64_t nrows, int k, double* part, double* out) {
  return launch_rm_colred<RM_DOTS>(ctx, nrows, k, A, B, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, part, out);
}
int launch_rm_cg_update(hfmi_ctx* ctx, int64_t nrows, int k, double* X, double* R, const double* P, const double* AP, const double* rz,
                        const double* pap, double* part, double* rr) {
  return launch_rm_colred<RM_CG_UPDATE>(ctx, nrows, k, nullptr, nullptr, X, R, P, AP, rz, pap, part, rr);
}

// ------------------------------------------------------------------ host side of the Chebyshev solve
// One scalar Jacobi-CG run on a pseudo-random right-hand side, on the device, with its two inner products per iteration read
// back: lanczos_bracket makes the bracket of the spectrum of D^-1 A of its coefficients.  Once per matrix (~40 iterations of
// one-vector kernels).
static int cheb_estimate(hfmi_op* op) {
  hfmi_ctx* ctx = op->ctx;
  const hfmi_csr* M = op->csr;
  const int64_t N = M->nrows;
  M->solve.cheb_state = -1;
  if (!gersh_usable(M->solve.gersh_lmax)) return HFMI_OK;
  hfmi_block R, Z, P, AP;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_0, N, 1, &R));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_1, N, 1, &Z));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_2, N, 1, &P));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_3, N, 1, &AP));
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, 4 * sizeof(double), &sc));
  double *rz = (double*)sc, *pap = rz + 1, *rz_new = rz + 2;
  HFMI_TRY(launch_randn(ctx, R.p, N, 1, R.ld, 0x5eedc0deull, 77u, 1.0));
  HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->solve.inv_diag, N, 1));
  HFMI_TRY(launch_copy(ctx, P.p, P.ld, Z.p, Z.ld, N, 1));
  HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, 1, rz));
  double h_rz = 0;
  HFMI_TRY(read_back(ctx, rz, 1, &h_rz));
  const double rz0 = h_rz;
  lanczos_run run;
  for (int it = 0; it < 60 && h_rz > 1e-28 * rz0; ++it) {
    HFMI_TRY(launch_csr_spmm(ctx, M, P.p, P.ld, AP.p, AP.ld, 1, false));
    HFMI_TRY(launch_col_dots(ctx, P.p, P.ld, AP.p, AP.ld, N, 1, pap));
    HFMI_TRY(launch_col_axpy_dev(ctx, R.p, R.ld, AP.p, AP.ld, N, 1, rz, pap, -1.0));
    HFMI_TRY(launch_diag_scale(ctx, Z.p, Z.ld, R.p, R.ld, M->solve.inv_diag, N, 1));
    HFMI_TRY(launch_col_dots(ctx, R.p, R.ld, Z.p, Z.ld, N, 1, rz_new));
    HFMI_TRY(launch_col_xpby_dev(ctx, P.p, P.ld, Z.p, Z.ld, N, 1, rz_new, rz));
    double two[3];
    HFMI_TRY(read_back(ctx, rz, 3, two));
    if (!run.push(h_rz, two[1], two[2])) return HFMI_OK;     // not SPD: leave the Chebyshev route off
    HIP_TRY(hipMemcpyAsync(rz, rz_new, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    h_rz = two[2];
  }
  const cheb_bracket br = lanczos_bracket(run.alpha, run.beta, M->solve.gersh_lmax);
  if (br.refusal) return HFMI_OK;
  M->solve.cheb_lmin = br.lmin;
  M->solve.cheb_lmax = br.lmax;
  M->solve.cheb_state = 1;
  return HFMI_OK;
}

// Y = M^-1 W by Chebyshev iteration on row-major copies; *handled = false: the caller runs the block CG
int cheb_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, bool* handled) {
  hfmi_ctx* ctx = op->ctx;
  const hfmi_csr* M = op->csr;
  const int64_t N = W->N;
  const int k = W->nvec;
  *handled = false;
  if (spsolve_knobs_ref().pcg || M->solve.cheb_state < 0) return HFMI_OK;
  if (M->solve.cheb_state == 0) HFMI_TRY(cheb_estimate(op));
  if (M->solve.cheb_state != 1) return HFMI_OK;
  cheb_recurrence rec(M->solve.cheb_lmin, M->solve.cheb_lmax);
  hfmi_block Bb, X0b, X1b;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_0, N, k, &Bb));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_1, N, k, &X0b));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_KRYLOV_2, N, k, &X1b));
  double* B = Bb.p;                                                  // used as row-major N x k arrays (ld >= N: large enough)
  double* X[2] = {X0b.p, X1b.p};
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)2 * k * sizeof(double), &sc));
  double* bb = (double*)sc;
  double* rr = bb + k;
  HFMI_TRY(launch_block_to_dense(ctx, W->p, W->ld, B, N, k));
  HFMI_TRY(launch_rm_colsq(ctx, B, N, k, nullptr, bb));
  HFMI_TRY(launch_cheb_first(ctx, B, X[1], X[0], M->solve.inv_diag, N, k, rec.inv_theta()));     // x_0 = 0 in X[0], x_1 in X[1]
  int steps = 1, cur = 1;                                            // X[cur] = x_steps, X[cur ^ 1] = x_{steps-1}
  const cheb_plan plan = cheb_solve_plan(M->solve.cheb_lmin, M->solve.cheb_lmax, op->rel_tol, op->max_iter);
  if (plan.to_cg) {
    M->solve.cheb_state = -1;
    return HFMI_OK;
  }
  std::vector<double> h(2 * (size_t)k);
  for (int round = 0; round < plan.rounds; ++round) {
    for (int i = 0; i < plan.budget[round]; ++i, ++steps) {
      double c1, c2;
      rec.next(&c1, &c2);
      HFMI_TRY(launch_cheb_step(ctx, M, B, X[cur], X[cur ^ 1], k, c1, c2, false));
      cur ^= 1;
    }
    // the true residual b - A x into the spare array, its column norms against those of b
    void* rs = nullptr;
    HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)N * k * sizeof(double), &rs));
    HFMI_TRY(launch_cheb_step(ctx, M, B, X[cur], (double*)rs, k, 0.0, 0.0, true));
    HFMI_TRY(launch_rm_colsq(ctx, (const double*)rs, N, k, nullptr, rr));
    HFMI_TRY(read_back(ctx, bb, (size_t)2 * k, h.data()));
    bool done = true, diverged = false;
    for (int j = 0; j < k; ++j) {
      if (!std::isfinite(h[j]))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "csr solve: non-finite right-hand side in vector %d", j);
      // a residual that is not finite, or larger than the right-hand side it started from, means the polynomial grew: an
      // eigenvalue of D^-1 A lies outside the bracket (Ritz values of a short CG run from one random vector can miss the top of
      // the spectrum).  That is a failure of the ESTIMATE, not of the matrix: hand the solve to the block CG, which alone
      // reports a matrix that is not SPD (advisor r4)
      if (!std::isfinite(h[k + j]) || h[k + j] > h[j]) diverged = true;
      if (!(h[k + j] <= op->rel_tol * op->rel_tol * h[j])) done = false;
    }
    if (diverged) break;
    if (done) {
      op->last_iters = steps;
      op->last_method = 1;
      HFMI_TRY(launch_dense_to_block(ctx, X[cur], Y->p, Y->ld, N, k));
      *handled = true;
      return HFMI_OK;
    }
  }
  M->solve.cheb_state = -1;       // the bracket of the spectrum was not good enough: this matrix goes back to the block CG for good
  return HFMI_OK;
}
