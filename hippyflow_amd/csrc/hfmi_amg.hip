// A^-1 on a block by CG preconditioned with one smoothed-aggregation V-cycle (hippylib BiLaplacianPrior.Asolver: PETSc CG
// with amg_method(); every prior.Rsolver apply, R^-1 = A^-1 M A^-1, runs two of these solves -- the doublePassG(A, prior.R,
// prior.Rsolver, ...) of activeSubspaceProjector.py:447-453 and KLEProjector's Solver2Operator(prior.Rsolver)).  The hierarchy
// is built on the host (hippyflow_amd/amg.py) and handed over level by level; everything per solve runs here.
//
// Layout: ROW-MAJOR (entry (row, j) at [row * k + j]) for every array of the solve, on every level, with one transpose of
// the right-hand side in and one of the solution out.  Almost all the work is sparse products -- the smoother steps, the
// residual, restriction R = P^T, prolongation P, A p -- and with lanes across the k columns of one row the gathers of the
// neighbour rows are contiguous runs (hfmi_cheb.hip's header: 1.5 TB/s for the column-major one-thread-per-row SpMM of the
// block CG against the row-major step's rate).  A column-major CG (csr_pcg_solve, hfmi_sparse.hip) would transpose to row-major and
// back around every V-cycle: four extra passes per iteration on the fine level.  The per-column inner products of CG are
// the price: they reduce over the row groups of a workgroup in LDS, then over workgroups in a fixed order (deterministic).
//
// V-cycle on level l (A_l, P_l: level l+1 -> l, R_l = P_l^T, explicit, so no transposed product is needed):
//   x = cheb(0, b); r = b - A x; b_{l+1} = R r; x_{l+1} = V_{l+1}(b_{l+1}); x += P x_{l+1}; x = cheb(x, b)
// cheb(x0, b) is the Chebyshev iteration of hfmi_cheb.hip (launch_cheb_first / launch_cheb_step, one fused kernel per step:
// D^-1 (b - A x) and the three-term update, coefficients from cheb_recurrence of hfmi_spsolve_rules.h) of degree `degree` on
// [lmin, lmax] of D^-1 A_l; the same polynomial before and after, so the V-cycle is symmetric.  Coarsest level: x = A_L^-1 b
// with the explicit dense inverse (<= 500 rows, one small product).  tests/helpers/amg_vcycle_twin.py is the same sequence in
// numpy.
//
// Block PCG: independent recurrences per column (alpha_j, beta_j on the device), the V-cycle as preconditioner; a column is
// done when its recursive residual ||r_j|| <= rel_tol ||b_j||, and the solve when every column is -- then the TRUE residual
// b - A x is formed once and checked against the same bound (CG restarted once from it if it is not met).  p.Ap <= 0 or r.z <= 0
// in an unconverged column: HFMI_ERR_NUMERIC (not SPD); max_iter reached: HFMI_ERR_NOT_CONVERGED.  On every error the output
// block is zero-filled: never NaN, never a silently wrong answer.
#include <algorithm>
#include <cmath>

#include "hfmi_internal.h"
#include "hfmi_rm_dev.h"

struct amg_level {
  const hfmi_csr* A;      // this level's matrix (not owned); its Jacobi preconditioner is prepared at hfmi_amg_create / add_level
  const hfmi_csr* P;      // prolongation from level l+1 (n_l x n_{l+1}); null on the coarsest level
  const hfmi_csr* R;      // restriction P^T (n_{l+1} x n_l)
  double lmin, lmax;      // Chebyshev interval of D^-1 A (smoothed levels only)
  int64_t n;
  dev_buf<double> b, x, t, res;  // row-major n x kcap work arrays (level 0: t and res only; coarsest: b and x only)
};

struct hfmi_amg {
  ~hfmi_amg() {           // a V-cycle may still be queued
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  hfmi_ctx* ctx = nullptr;
  std::vector<amg_level> lv;
  int degree = 0;
  dev_buf<double> coarse_inv;   // dense n_L x n_L row-major
  int kcap = 0;
  dev_buf<double> pcg[6];       // row-major N x kcap: b, x, r, z, p, Ap
  dev_buf<double> part;         // per-(column, workgroup) partial sums of the reductions (kcap x RM_CHUNKS)
  dev_buf<double> sc;           // device scalars, 8 x kcap
};

namespace {
// Y (nrows x k) = M X (+ Y when ACC): restriction (R_l, ~30 entries a row) and prolongation with correction (P_l)
template <bool ACC>
__global__ __launch_bounds__(256) void k_amg_spmm_rm(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                    const double* __restrict__ data, int64_t nrows, int k,
                                                    const double* __restrict__ X, double* __restrict__ Y) {
  const rm_map m = rm_thread(k);
  if (!m.live) return;
  for (int64_t r0 = (int64_t)blockIdx.x * m.rows_per_pass; r0 < nrows; r0 += (int64_t)gridDim.x * m.rows_per_pass) {
    const int64_t row = r0 + m.rl;
    if (row >= nrows) continue;
    const int64_t zb = indptr[row], ze = indptr[row + 1];
    for (int j = m.j0; j < k; j += m.jstep) {
      double acc = 0.0;
      for (int64_t z = zb; z < ze; ++z) acc += data[z] * X[(int64_t)indices[z] * k + j];
      const int64_t e = row * k + j;
      Y[e] = ACC ? Y[e] + acc : acc;
    }
  }
}

// coarsest level: X (n x k) = Ainv (n x n, row-major) B (n x k)
__global__ __launch_bounds__(256) void k_amg_coarse_rm(const double* __restrict__ Ainv, int n, int k, const double* __restrict__ B,
                                                      double* __restrict__ X) {
  const rm_map m = rm_thread(k);
  if (!m.live) return;
  for (int64_t r0 = (int64_t)blockIdx.x * m.rows_per_pass; r0 < n; r0 += (int64_t)gridDim.x * m.rows_per_pass) {
    const int64_t row = r0 + m.rl;
    if (row >= n) continue;
    const double* a = Ainv + row * n;
    for (int j = m.j0; j < k; j += m.jstep) {
      double acc = 0.0;
      for (int l = 0; l < n; ++l) acc += a[l] * B[(int64_t)l * k + j];
      X[row * k + j] = acc;
    }
  }
}

// P = Z + beta_j P, beta_j = rz_new_j / rz_j (0 when rz_j is not > 0: a converged or broken-down column restarts from Z)
__global__ __launch_bounds__(256) void k_amg_pcg_dir(int64_t nrows, int k, double* __restrict__ P, const double* __restrict__ Z,
                                                    const double* __restrict__ rz_new, const double* __restrict__ rz) {
  const int64_t total = nrows * k;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % k);
    const double d = rz[j];
    double beta = d > 0.0 ? rz_new[j] / d : 0.0;
    if (!std::isfinite(beta)) beta = 0.0;
    P[e] = Z[e] + beta * P[e];
  }
}
}  // namespace

constexpr int AMG_WG_PER_CU = 16;   // cap of rm_grid for the V-cycle's products
static int launch_amg_spmm(hfmi_ctx* ctx, const hfmi_csr* M, const double* X, double* Y, int k, bool acc) {
  if (acc)
    hipLaunchKernelGGL((k_amg_spmm_rm<true>), dim3(rm_grid(ctx, M->nrows, k, AMG_WG_PER_CU)), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->nrows, k, X, Y);
  else
    hipLaunchKernelGGL((k_amg_spmm_rm<false>), dim3(rm_grid(ctx, M->nrows, k, AMG_WG_PER_CU)), dim3(256), 0, ctx->stream, M->indptr, M->indices, M->data, M->nrows, k, X, Y);
  HIP_TRY(hipGetLastError());
  return HFMI_OK;
}
// out[j] = <A_j, B_j> over row-major (nrows x k) arrays
static int amg_dots(hfmi_amg* g, const double* A, const double* B, int64_t nrows, int k, double* out) {
  return launch_rm_coldots(g->ctx, A, B, nrows, k, g->part, out);
}

static void amg_free_work(hfmi_amg* g) {
  for (auto& L : g->lv)
    for (dev_buf<double>* p : {&L.b, &L.x, &L.t, &L.res}) p->reset();
  for (dev_buf<double>& p : g->pcg) p.reset();
  g->part.reset();
  g->sc.reset();
  g->kcap = 0;
}
static int amg_alloc(hfmi_ctx* ctx, dev_buf<double>* p, size_t count) {
  OWN_TRY(p->alloc(count));
  HIP_TRY(hipMemsetAsync(*p, 0, count * sizeof(double), ctx->stream));   // the smoother's spare array must hold finite values
  return HFMI_OK;
}
// work arrays for blocks of up to k vectors
static int amg_reserve(hfmi_amg* g, int k) {
  if (k <= g->kcap) return HFMI_OK;
  hfmi_ctx* ctx = g->ctx;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  amg_free_work(g);
  const size_t kk = (size_t)k;
  const int last = (int)g->lv.size() - 1;
  for (int l = 0; l <= last; ++l) {
    amg_level& L = g->lv[l];
    const size_t cnt = (size_t)L.n * kk;
    if (l > 0) {
      HFMI_TRY(amg_alloc(ctx, &L.b, cnt));
      HFMI_TRY(amg_alloc(ctx, &L.x, cnt));
    }
    if (l < last) {
      HFMI_TRY(amg_alloc(ctx, &L.t, cnt));
      HFMI_TRY(amg_alloc(ctx, &L.res, cnt));
    }
  }
  for (dev_buf<double>& p : g->pcg) HFMI_TRY(amg_alloc(ctx, &p, (size_t)g->lv[0].n * kk));
  HFMI_TRY(amg_alloc(ctx, &g->part, kk * RM_CHUNKS));
  HFMI_TRY(amg_alloc(ctx, &g->sc, 8 * kk));
  g->kcap = k;
  return HFMI_OK;
}

// degree steps of the Chebyshev iteration from x0 = 0 (pre) or from the x held in *x (post); *x holds the result and *t a
// finite spare array on return (the pointers may be swapped)
static int amg_smooth(hfmi_amg* g, amg_level& L, const double* b, double** x, double** t, int k, bool from_zero) {
  hfmi_ctx* ctx = g->ctx;
  cheb_recurrence rec(L.lmin, L.lmax);
  double *cur, *prev;
  if (from_zero) {
    // x_1 = D^-1 b / theta into one array, x_0 = 0 into the other
    cur = *t;
    prev = *x;
    HFMI_TRY(launch_cheb_first(ctx, b, cur, prev, L.A->solve.inv_diag, L.n, k, rec.inv_theta()));
  } else {
    // x_1 = x_0 + D^-1 (b - A x_0) / theta (the spare array's old contents are multiplied by c1 = 0)
    HFMI_TRY(launch_cheb_step(ctx, L.A, b, *x, *t, k, 0.0, rec.inv_theta(), false));
    cur = *t;
    prev = *x;
  }
  for (int s = 1; s < g->degree; ++s) {
    double c1, c2;
    rec.next(&c1, &c2);
    HFMI_TRY(launch_cheb_step(ctx, L.A, b, cur, prev, k, c1, c2, false));
    std::swap(cur, prev);
  }
  *x = cur;
  *t = prev;
  return HFMI_OK;
}

// x = V_l(b); row-major n_l x k arrays.  On level 0 b and x are the caller's, the output pointer is fixed: a result that
// ends in the spare array is copied.
static int amg_vcycle_rm(hfmi_amg* g, int l, const double* b, double* xout, int k) {
  hfmi_ctx* ctx = g->ctx;
  amg_level& L = g->lv[l];
  if (l == (int)g->lv.size() - 1) {
    hipLaunchKernelGGL(k_amg_coarse_rm, dim3(rm_grid(ctx, L.n, k, AMG_WG_PER_CU)), dim3(256), 0, ctx->stream, g->coarse_inv, (int)L.n, k, b, xout);
    HIP_TRY(hipGetLastError());
    return HFMI_OK;
  }
  amg_level& C = g->lv[l + 1];
  double* x = xout;
  double* t = L.t;
  HFMI_TRY(amg_smooth(g, L, b, &x, &t, k, true));
  HFMI_TRY(launch_cheb_step(ctx, L.A, b, x, L.res, k, 0.0, 0.0, true));       // res = b - A x
  HFMI_TRY(launch_amg_spmm(ctx, L.R, L.res, C.b, k, false));                  // b_{l+1} = R res
  HFMI_TRY(amg_vcycle_rm(g, l + 1, C.b, C.x, k));
  HFMI_TRY(launch_amg_spmm(ctx, L.P, C.x, x, k, true));                       // x += P x_{l+1}
  HFMI_TRY(amg_smooth(g, L, b, &x, &t, k, false));
  if (x != xout) HIP_TRY(hipMemcpyAsync(xout, x, (size_t)L.n * k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  // the spare array of level l must be L.t again for the next cycle (xout is the caller's)
  return HFMI_OK;
}

static int amg_check_ready(const hfmi_amg* g) {
  if (!g->coarse_inv) HFMI_FAIL(HFMI_ERR_INVALID, "amg: no coarse solve set (hfmi_amg_set_coarse)");
  return HFMI_OK;
}

// ------------------------------------------------------------------ C ABI
static bool bracket_ok(double lmin, double lmax) { return std::isfinite(lmin) && std::isfinite(lmax) && lmin > 0.0 && lmax > lmin; }

extern "C" int hfmi_amg_create(hfmi_ctx* ctx, const hfmi_csr* A, double lmin, double lmax, int degree, hfmi_amg** out) {
  if (!ctx || !A || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->nrows != A->ncols) HFMI_FAIL(HFMI_ERR_INVALID, "amg_create: matrix must be square");
  if (degree < 1 || degree > 16) HFMI_FAIL(HFMI_ERR_INVALID, "amg_create: Chebyshev degree %d outside 1..16", degree);
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(csr_prepare_jacobi(ctx, A));
  hfmi_amg* g = new (std::nothrow) hfmi_amg();
  if (!g) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  g->ctx = ctx;
  g->degree = degree;
  amg_level L = {};
  L.A = A;
  L.lmin = lmin;
  L.lmax = lmax;
  L.n = A->nrows;
  g->lv.push_back(std::move(L));
  *out = g;
  return HFMI_OK;
}

extern "C" int hfmi_amg_add_level(hfmi_amg* g, const hfmi_csr* P, const hfmi_csr* R, const hfmi_csr* Ac, double lmin, double lmax) {
  if (!g || !P || !R || !Ac) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (g->coarse_inv) HFMI_FAIL(HFMI_ERR_INVALID, "amg_add_level: the coarse solve is already set");
  const int64_t nf = g->lv.back().n, nc = Ac->nrows;
  if (Ac->ncols != nc || P->nrows != nf || P->ncols != nc || R->nrows != nc || R->ncols != nf)
    HFMI_FAIL(HFMI_ERR_INVALID, "amg_add_level: shapes do not chain (fine %lld, P %lld x %lld, R %lld x %lld, A_c %lld x %lld)",
              (long long)nf, (long long)P->nrows, (long long)P->ncols, (long long)R->nrows, (long long)R->ncols, (long long)nc,
              (long long)Ac->ncols);
  HIP_TRY(hipSetDevice(g->ctx->device));
  HFMI_TRY(csr_prepare_jacobi(g->ctx, Ac));
  HIP_TRY(hipStreamSynchronize(g->ctx->stream));
  amg_free_work(g);                               // the level list changes: work arrays are sized again at the next solve
  g->lv.back().P = P;
  g->lv.back().R = R;
  amg_level L = {};
  L.A = Ac;
  L.lmin = lmin;
  L.lmax = lmax;
  L.n = nc;
  g->lv.push_back(std::move(L));
  return HFMI_OK;
}

extern "C" int hfmi_amg_set_coarse(hfmi_amg* g, int n, const double* host_inv) {
  if (!g || !host_inv) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (n != g->lv.back().n) HFMI_FAIL(HFMI_ERR_INVALID, "amg_set_coarse: the coarsest level has %lld rows, got %d", (long long)g->lv.back().n, n);
  if (n > 4096) HFMI_FAIL(HFMI_ERR_INVALID, "amg_set_coarse: %d rows is too many for a dense coarse solve (<= 4096)", n);
  for (size_t l = 0; l + 1 < g->lv.size(); ++l)
    if (!bracket_ok(g->lv[l].lmin, g->lv[l].lmax))
      HFMI_FAIL(HFMI_ERR_INVALID, "amg_set_coarse: level %d has no valid Chebyshev interval (0 < lmin < lmax: %g, %g)", (int)l,
                g->lv[l].lmin, g->lv[l].lmax);
  for (int64_t i = 0; i < (int64_t)n * n; ++i)
    if (!std::isfinite(host_inv[i])) HFMI_FAIL(HFMI_ERR_NUMERIC, "amg_set_coarse: non-finite entry in the coarse inverse");
  HIP_TRY(hipSetDevice(g->ctx->device));
  dev_buf<double> d;
  OWN_TRY(d.alloc((size_t)n * n));
  HIP_TRY(hipMemcpy(d, host_inv, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
  g->coarse_inv = std::move(d);
  return HFMI_OK;
}

extern "C" int hfmi_amg_info(const hfmi_amg* g, int* levels, int64_t* rows, int max_levels) {
  if (!g) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (levels) *levels = (int)g->lv.size();
  if (rows)
    for (int l = 0; l < (int)g->lv.size() && l < max_levels; ++l) rows[l] = g->lv[l].n;
  return HFMI_OK;
}

extern "C" int hfmi_amg_destroy(hfmi_amg* g) {
  delete g;
  return HFMI_OK;
}

static int check_block(const hfmi_amg* g, const hfmi_block* B, const hfmi_block* X, const char* what) {
  if (!B || !X) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  const int64_t n = g->lv[0].n;
  if (B->N != n || X->N != n)
    HFMI_FAIL(HFMI_ERR_INVALID, "%s: matrix has %lld rows, block vectors have %lld / %lld", what, (long long)n, (long long)B->N, (long long)X->N);
  if (B->nvec != X->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "%s: %d right-hand sides, %d solution vectors", what, B->nvec, X->nvec);
  if (B->p == X->p) HFMI_FAIL(HFMI_ERR_INVALID, "%s: input and output blocks must not alias", what);
  return HFMI_OK;
}

extern "C" int hfmi_amg_vcycle(hfmi_amg* g, const hfmi_block* B, hfmi_block* X) {
  if (!g) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(check_block(g, B, X, "amg_vcycle"));
  HFMI_TRY(amg_check_ready(g));
  const int k = B->nvec;
  if (k == 0) return HFMI_OK;
  hfmi_ctx* ctx = g->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(amg_reserve(g, k));
  const int64_t N = g->lv[0].n;
  double* b = g->pcg[0];
  double* z = g->pcg[3];
  HFMI_TRY(launch_block_to_dense(ctx, B->p, B->ld, b, N, k));
  HFMI_TRY(amg_vcycle_rm(g, 0, b, z, k));
  HFMI_TRY(launch_dense_to_block(ctx, z, X->p, X->ld, N, k));
  return HFMI_OK;
}

static int amg_pcg_core(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_amg* g = op->amg;
  hfmi_ctx* ctx = g->ctx;
  const int k = W->nvec;
  const int64_t N = g->lv[0].n;
  const hfmi_csr* A = g->lv[0].A;
  HFMI_TRY(amg_reserve(g, k));
  double *b = g->pcg[0], *x = g->pcg[1], *r = g->pcg[2], *z = g->pcg[3], *p = g->pcg[4], *ap = g->pcg[5];
  double* bb = g->sc;
  double* rz = bb + k;
  double* rz_new = rz + k;
  double* pr = rz_new + k;     // (pap, rr, r.z of this iteration) read back together, once per iteration
  double* pap = pr;
  double* rr = pr + k;
  double* rzc = pr + 2 * k;
  const size_t bytes = (size_t)N * k * sizeof(double);
  std::vector<double> h_bb(k), h_pr(3 * (size_t)k);
  std::vector<char> conv(k, 0);
  const double tol2 = op->rel_tol * op->rel_tol;

  HFMI_TRY(launch_block_to_dense(ctx, W->p, W->ld, b, N, k));
  HFMI_TRY(amg_dots(g, b, b, N, k, bb));
  HFMI_TRY(read_back(ctx, bb, k, h_bb.data()));
  for (int j = 0; j < k; ++j)
    if (!std::isfinite(h_bb[j])) HFMI_FAIL(HFMI_ERR_NUMERIC, "amg_pcg: non-finite right-hand side in vector %d", j);
  for (int j = 0; j < k; ++j) conv[j] = !(h_bb[j] > 0.0);                  // a zero right-hand side is solved by x = 0
  HIP_TRY(hipMemsetAsync(x, 0, bytes, ctx->stream));
  HIP_TRY(hipMemcpyAsync(r, b, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  int it = 0;
  bool restart = true, refined = false;
  while (true) {
    if (restart) {
      // z = V r, rz = <r, z>, p = z
      HFMI_TRY(amg_vcycle_rm(g, 0, r, z, k));
      HFMI_TRY(amg_dots(g, r, z, N, k, rz));
      HIP_TRY(hipMemcpyAsync(rzc, rz, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, ctx->stream));
      restart = false;
    }
    if (it >= op->max_iter) break;
    ++it;
    HFMI_TRY(launch_amg_spmm(ctx, A, p, ap, k, false));                       // ap = A p
    HFMI_TRY(amg_dots(g, p, ap, N, k, pap));
    HFMI_TRY(launch_rm_cg_update(ctx, N, k, x, r, p, ap, rz, pap, g->part, rr));
    HFMI_TRY(read_back(ctx, pr, 3 * (size_t)k, h_pr.data()));
    bool done = true;
    for (int j = 0; j < k; ++j) {
      const double pp = h_pr[j], rj = h_pr[k + j], rzj = h_pr[2 * k + j];
      if (!std::isfinite(rj) || !std::isfinite(pp))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "amg_pcg: non-finite residual in vector %d at iteration %d (matrix not SPD, or non-finite input)", j, it);
      if (!conv[j] && !(rzj > 0.0))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "amg_pcg: r.z = %.3e <= 0 in vector %d at iteration %d (matrix or V-cycle not SPD)", rzj, j, it);
      if (!conv[j] && !(pp > 0.0))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "amg_pcg: p.Ap = %.3e <= 0 in vector %d at iteration %d (matrix not SPD)", pp, j, it);
      conv[j] = rj <= tol2 * h_bb[j];
      if (!conv[j]) done = false;
    }
    if (done) {
      bool ok = true;
      if (!refined) {
        // the true residual against the same bound; if the recursion drifted, CG once more from the true residual.  Only
        // once: for a right-hand side far smaller than |A| |x| (the second solve of R^-1 = A^-1 M A^-1) fp64 cannot form
        // b - A x to rel_tol, and the recursive residual -- what PETSc's CG tests too -- decides.
        HFMI_TRY(launch_cheb_step(ctx, A, b, x, r, k, 0.0, 0.0, true));      // r = b - A x
        HFMI_TRY(amg_dots(g, r, r, N, k, rr));
        HFMI_TRY(read_back(ctx, rr, k, h_pr.data() + k));
        for (int j = 0; j < k; ++j) {
          conv[j] = h_pr[k + j] <= tol2 * h_bb[j];
          if (!conv[j]) ok = false;
        }
        refined = true;
      }
      if (ok) {
        op->last_iters = it;
        op->last_method = 2;
        return launch_dense_to_block(ctx, x, Y->p, Y->ld, N, k);
      }
      restart = true;
      continue;
    }
    HFMI_TRY(amg_vcycle_rm(g, 0, r, z, k));                                   // z = V r
    HFMI_TRY(amg_dots(g, r, z, N, k, rz_new));
    HIP_TRY(hipMemcpyAsync(rzc, rz_new, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_amg_pcg_dir, dim3(rm_grid(ctx, N, k, AMG_WG_PER_CU)), dim3(256), 0, ctx->stream, N, k, p, z, rz_new, rz);
    HIP_TRY(hipGetLastError());
    std::swap(rz, rz_new);
  }
  op->last_iters = it;
  op->last_method = 2;
  HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "amg_pcg: no convergence to %.1e in %d iterations", op->rel_tol, op->max_iter);
}

// Y = A^-1 W (hfmi_op_apply of an OP_AMG_PCG operator); on error Y is zero-filled
int amg_pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_amg* g = op->amg;
  HFMI_TRY(check_block(g, W, Y, "amg_pcg"));
  HFMI_TRY(amg_check_ready(g));
  if (W->nvec == 0) return HFMI_OK;
  const int rc = amg_pcg_core(op, W, Y);
  if (rc != HFMI_OK && rc != HFMI_ERR_HIP) {
    const std::string msg = hfmi_last_error();
    (void)launch_fill(g->ctx, Y->p, Y->N, Y->nvec, Y->ld, 0.0, false);
    (void)hipStreamSynchronize(g->ctx->stream);
    hfmi_set_error("%s", msg.c_str());
  }
  return rc;
}
