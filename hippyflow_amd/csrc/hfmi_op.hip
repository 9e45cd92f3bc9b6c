// Operators of libhfmi.so (include/hfmi.h): constructors and setters of the tagged operator object, the pipelined host
// callback, the panel-overlapped rank reduction and the application itself.  Host side only.
#include <float.h>
#include <math.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <memory>
#include <new>

#include "hfmi_internal.h"
#include "hfmi_kcov_nu.h"      // the layout of the table words

// ------------------------------------------------------------------ operators
static hfmi_op* op_new(hfmi_ctx* ctx, hfmi_op_kind kind) {
  hfmi_op* op = new (std::nothrow) hfmi_op();
  if (!op) return nullptr;
  op->ctx = ctx;
  op->kind = kind;
  return op;
}
extern "C" int hfmi_op_snapshot_gram(hfmi_ctx* ctx, const hfmi_block* X, double scale, hfmi_op** out) {
  if (!ctx || !X || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_SNAPSHOT_GRAM);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *X;
  op->X.owner = false;
  op->scale = scale;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_low_rank(hfmi_ctx* ctx, const hfmi_block* U, const double* host_d, hfmi_op** out) {
  if (!ctx || !U || !host_d || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  std::unique_ptr<hfmi_op> op(op_new(ctx, OP_SNAPSHOT_GRAM));
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *U;
  op->X.owner = false;
  op->scale = 1.0;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = (hipError_t)op->weights.alloc((size_t)U->nvec);
  if (e == hipSuccess) e = hipMemcpy(op->weights, host_d, (size_t)U->nvec * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) HFMI_FAIL(HFMI_ERR_HIP, "op_low_rank: %s", hipGetErrorString(e));
  *out = op.release();
  return HFMI_OK;
}
static int op_jac(hfmi_ctx* ctx, hfmi_op_kind kind, const hfmi_block* J, int ndata, int q, const double* host_gamma_inv,
                  double scale, hfmi_op** out) {
  if (!ctx || !J || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (ndata <= 0 || q <= 0 || (int64_t)ndata * q != J->nvec)
    HFMI_FAIL(HFMI_ERR_INVALID, "jacobian operator: ndata*q = %lld must equal the number of stored rows %d",
              (long long)ndata * q, J->nvec);
  std::unique_ptr<hfmi_op> op(op_new(ctx, kind));
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *J;
  op->X.owner = false;
  op->ndata = ndata;
  op->q = q;
  op->scale = scale;
  if (host_gamma_inv) {
    const int ld = (int)round_up(q, 16);
    OWN_TRY(op->gamma_inv.alloc((size_t)q * ld));
    HFMI_TRY(upload_small(ctx, host_gamma_inv, q, q, op->gamma_inv, ld));
  }
  *out = op.release();
  return HFMI_OK;
}
extern "C" int hfmi_op_jtj(hfmi_ctx* ctx, const hfmi_block* J, int ndata, int q, const double* host_gamma_inv,
                           double scale, hfmi_op** out) {
  return op_jac(ctx, OP_JTJ, J, ndata, q, host_gamma_inv, scale, out);
}
extern "C" int hfmi_op_jjt(hfmi_ctx* ctx, const hfmi_block* J, int ndata, int q, double scale, hfmi_op** out) {
  return op_jac(ctx, OP_JJT, J, ndata, q, nullptr, scale, out);
}
extern "C" int hfmi_op_dense_sym(hfmi_ctx* ctx, const hfmi_block* C, hfmi_op** out) {
  if (!ctx || !C || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (C->N != C->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "dense_sym: matrix must be square (%lld x %d)", (long long)C->N, C->nvec);
  hfmi_op* op = op_new(ctx, OP_DENSE_SYM);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *C;
  op->X.owner = false;
  *out = op;
  return HFMI_OK;
}
// the checks every kernel covariance constructor shares
// last_family: HFMI_KERNEL_SQEXP for the creators that take a bare family, HFMI_KERNEL_MATERN1 for those that take a hfmi_kernel_spec,
// HFMI_KERNEL_MATERN for those that take a hfmi_kernel_spec2
static int kcov_check(const char* who, int64_t N, int d, int family, double ell, double nugget, int last_family = HFMI_KERNEL_SQEXP) {
  if (N < 1) HFMI_FAIL(HFMI_ERR_INVALID, "%s: needs at least one point (N = %lld)", who, (long long)N);
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "%s: points have 1, 2 or 3 coordinates, got d = %d", who, d);
  if (family < HFMI_KERNEL_MATERN12 || family > last_family) HFMI_FAIL(HFMI_ERR_INVALID, "%s: unknown kernel family %d", who, family);
  if (!(ell > 0.0)) HFMI_FAIL(HFMI_ERR_INVALID, "%s: correlation length must be positive", who);
  if (!(nugget >= 0.0)) HFMI_FAIL(HFMI_ERR_INVALID, "%s: nugget must not be negative", who);
  return HFMI_OK;
}
// host points (n x d row-major) -> one array per coordinate on the device (the kernel reads x_c[j] for runs of consecutive j)
// mL: the lower Cholesky factor of the kernel's metric (d x d row-major) or null; with it the device gets x' = L^T x,
// x'_c = sum_{e >= c} L_ec x_e (e ascending), and |x'_i - x'_j|^2 = (x_i - x_j)^T G (x_i - x_j): the kernels see an isotropic problem
static int kcov_upload_points(hfmi_ctx* ctx, const double* host_points, int64_t n, int d, dev_buf<double>* out, const double* mL = nullptr) {
  std::vector<double> soa((size_t)n * d);
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < d; ++c) {
      const double* xi = host_points + (size_t)i * d;
      double v = xi[c];
      if (mL) {
        v = mL[c * d + c] * xi[c];
        for (int e = c + 1; e < d; ++e) v += mL[e * d + c] * xi[e];
      }
      soa[(size_t)c * n + i] = v;
    }
  dev_buf<double> x;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = (hipError_t)x.alloc(soa.size());
  if (e == hipSuccess) e = hipMemcpy(x, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) HFMI_FAIL(HFMI_ERR_HIP, "kernel covariance points: %s", hipGetErrorString(e));
  *out = std::move(x);
  return HFMI_OK;
}
// the table words of a general Matern kernel on the device, owned by `out`, and sqrt(2 nu) as the builder rounded it
int kcov_nu_upload(hfmi_ctx* ctx, double nu, dev_buf<double>* out, double* ca) {
  double words[HFMI_MATERN_TABLE_WORDS];
  HFMI_TRY(hfmi_kernel_matern_tables(nu, words));
  dev_buf<double> t;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = (hipError_t)t.alloc(HFMI_MATERN_TABLE_WORDS);
  if (e == hipSuccess) e = hipMemcpy(t, words, sizeof(words), hipMemcpyHostToDevice);
  if (e != hipSuccess) HFMI_FAIL(HFMI_ERR_HIP, "kernel covariance tables: %s", hipGetErrorString(e));
  *out = std::move(t);
  *ca = words[KNU_W_CA];
  return HFMI_OK;
}
static int kcov_op_new(hfmi_ctx* ctx, hfmi_op_kind kind, const double* host_points, int64_t N, int d, int family, double sigma, double ell,
                       double nugget, hfmi_op** out, const double* mL = nullptr, double nu = 0.0) {
  std::unique_ptr<hfmi_op> op(op_new(ctx, kind));
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  HFMI_TRY(kcov_upload_points(ctx, host_points, N, d, &op->kc_x, mL));
  if (family == HFMI_KERNEL_MATERN) {
    HFMI_TRY(kcov_nu_upload(ctx, nu, &op->kc_nutab, &op->kc_nuca));
    op->kc_nu = nu;
  }
  op->kc_N = N;
  op->kc_d = d;
  op->kc_family = family;
  op->kc_sigma = sigma;
  op->kc_ell = ell;
  op->kc_nugget = nugget;
  *out = op.release();
  return HFMI_OK;
}
// The creators behind both entry-point sets: a bare family (last_family = HFMI_KERNEL_SQEXP, no metric) or a hfmi_kernel_spec
// (last_family = HFMI_KERNEL_MATERN1; mL: the metric's lower factor or null) or a hfmi_kernel_spec2 (last_family = HFMI_KERNEL_MATERN;
// nu: the smoothness, read for that family only)
static int kcov_create(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, int family, double sigma, double ell, double nugget,
                       int last_family, const double* mL, hfmi_op** out, double nu = 0.0) {
  if (!ctx || !host_points || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(kcov_check("kernel_cov", N, d, family, ell, nugget, last_family));
  return kcov_op_new(ctx, OP_KERNEL_COV, host_points, N, d, family, sigma, ell, nugget, out, mL, nu);
}
static int kcov_cross_create(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d, int family,
                             double sigma, double ell, double nugget, int64_t diag_offset, int last_family, const double* mL, hfmi_op** out,
                             double nu = 0.0) {
  if (!ctx || !host_targets || !host_sources || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(kcov_check("kernel_cross_cov", N, d, family, ell, nugget, last_family));
  if (M < 1) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cross_cov: needs at least one target (M = %lld)", (long long)M);
  if (diag_offset == HFMI_KERNEL_NO_DIAGONAL) {
    if (nugget != 0.0) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cross_cov: a nugget needs targets that are sources (diag_offset >= 0)");
  } else if (diag_offset < 0 || diag_offset > N - M) {
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cross_cov: diag_offset = %lld with M = %lld targets does not lie inside the N = %lld sources",
              (long long)diag_offset, (long long)M, (long long)N);
  }
  hfmi_op* raw = nullptr;
  HFMI_TRY(kcov_op_new(ctx, OP_KERNEL_CROSS, host_sources, N, d, family, sigma, ell, nugget, &raw, mL, nu));
  std::unique_ptr<hfmi_op> op(raw);
  HFMI_TRY(kcov_upload_points(ctx, host_targets, M, d, &op->kc_t, mL));
  op->kc_M = M;
  op->kc_diag = diag_offset;
  op->kc_slab = false;
  *out = op.release();
  return HFMI_OK;
}
static int kcov_rows_create(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, int family, double sigma, double ell, double nugget,
                            int64_t row0, int64_t nrows, int last_family, const double* mL, hfmi_op** out, double nu = 0.0) {
  if (!ctx || !host_points || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(kcov_check("kernel_cov_rows", N, d, family, ell, nugget, last_family));
  if (row0 < 0 || nrows < 0 || row0 > N - nrows)
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov_rows: rows %lld .. %lld + %lld do not lie inside 0 .. N = %lld", (long long)row0, (long long)row0,
              (long long)nrows, (long long)N);
  hfmi_op* op = nullptr;
  HFMI_TRY(kcov_op_new(ctx, OP_KERNEL_CROSS, host_points, N, d, family, sigma, ell, nugget, &op, mL, nu));
  op->kc_M = nrows;
  op->kc_diag = row0;
  op->kc_slab = true;
  *out = op;
  return HFMI_OK;
}
// max_line > 0: the long route (hfmi_op_kernel_cov_grid_long)
static int kcov_grid_create(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N, int family,
                            double sigma, double ell, double nugget, int last_family, const double* mL, hfmi_op** out, int max_line = 0,
                            double nu = 0.0) {
  if (!ctx || !n || !h || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HFMI_TRY(kcov_check("kernel_cov_grid", N, d, family, ell, nugget, last_family));
  std::unique_ptr<hfmi_op> op(op_new(ctx, OP_KERNEL_COV_GRID));
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  HFMI_TRY(fftcov_create(ctx, d, n, h, host_nodes, N, family, sigma, ell, nugget, mL, &op->fc, max_line, nu));
  *out = op.release();
  return HFMI_OK;
}
extern "C" int hfmi_op_kernel_cov(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, int family, double sigma, double ell,
                                  double nugget, hfmi_op** out) {
  return kcov_create(ctx, host_points, N, d, family, sigma, ell, nugget, HFMI_KERNEL_SQEXP, nullptr, out);
}
extern "C" int hfmi_op_kernel_cross_cov(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d,
                                        int family, double sigma, double ell, double nugget, int64_t diag_offset, hfmi_op** out) {
  return kcov_cross_create(ctx, host_targets, M, host_sources, N, d, family, sigma, ell, nugget, diag_offset, HFMI_KERNEL_SQEXP, nullptr, out);
}
extern "C" int hfmi_op_kernel_cov_rows(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, int family, double sigma, double ell,
                                       double nugget, int64_t row0, int64_t nrows, hfmi_op** out) {
  return kcov_rows_create(ctx, host_points, N, d, family, sigma, ell, nugget, row0, nrows, HFMI_KERNEL_SQEXP, nullptr, out);
}
extern "C" int hfmi_op_kernel_cov_grid(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N,
                                       int family, double sigma, double ell, double nugget, hfmi_op** out) {
  return kcov_grid_create(ctx, d, n, h, host_nodes, N, family, sigma, ell, nugget, HFMI_KERNEL_SQEXP, nullptr, out);
}

// G = L L^T, unblocked, column by column (the metric of a kernel covariance: hfmi_kcov_eval.h)
int kcov_metric_factor(const double* G, int d, double* L) {
  if (!G || !L) HFMI_FAIL(HFMI_ERR_INVALID, "kernel metric: null argument");
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "kernel metric: d = %d is not 1, 2 or 3", d);
  double gmax = 0.0;
  for (int i = 0; i < d * d; ++i) {
    if (!isfinite(G[i])) HFMI_FAIL(HFMI_ERR_INVALID, "kernel metric: entry (%d, %d) is not finite", i / d, i % d);
    gmax = std::max(gmax, fabs(G[i]));
  }
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < i; ++j)
      if (fabs(G[i * d + j] - G[j * d + i]) > 4.0 * DBL_EPSILON * gmax)
        HFMI_FAIL(HFMI_ERR_INVALID, "kernel metric: not symmetric, G[%d][%d] = %.17g and G[%d][%d] = %.17g", i, j, G[i * d + j], j, i, G[j * d + i]);
  for (int i = 0; i < d * d; ++i) L[i] = 0.0;
  for (int j = 0; j < d; ++j) {
    double piv = G[j * d + j];
    for (int c = 0; c < j; ++c) piv -= L[j * d + c] * L[j * d + c];
    if (!(piv > 0.0)) HFMI_FAIL(HFMI_ERR_INVALID, "kernel metric: not positive definite (pivot %d is %.3e)", j, piv);
    const double root = sqrt(piv);
    L[j * d + j] = root;
    for (int i = j + 1; i < d; ++i) {
      double v = G[i * d + j];      // the lower triangle is the one read
      for (int c = 0; c < j; ++c) v -= L[i * d + c] * L[j * d + c];
      L[i * d + j] = v / root;
    }
  }
  return HFMI_OK;
}
extern "C" int hfmi_kernel_metric_factor(const double* G, int d, double* L) { return kcov_metric_factor(G, d, L); }

// a descriptor's metric: null (all nine entries zero: the identity) or its factor in `store`
static int kcov_spec_metric(const char* who, const hfmi_kernel_spec* spec, int d, double* store, const double** mL) {
  if (!spec) HFMI_FAIL(HFMI_ERR_INVALID, "%s: null kernel descriptor", who);
  if (d < 1 || d > 3) HFMI_FAIL(HFMI_ERR_INVALID, "%s: points have 1, 2 or 3 coordinates, got d = %d", who, d);
  if (spec->d != d) HFMI_FAIL(HFMI_ERR_INVALID, "%s: the kernel descriptor is for d = %d, the points have d = %d", who, spec->d, d);
  bool zero = true;
  for (int i = 0; i < 9; ++i) zero = zero && spec->metric[i] == 0.0;
  *mL = nullptr;
  if (zero) return HFMI_OK;
  HFMI_TRY(kcov_metric_factor(spec->metric, d, store));
  *mL = store;
  return HFMI_OK;
}
extern "C" int hfmi_op_kernel_cov_spec(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec* spec, hfmi_op** out) {
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec_metric("kernel_cov", spec, d, store, &mL));
  return kcov_create(ctx, host_points, N, d, spec->family, spec->sigma, spec->ell, spec->nugget, HFMI_KERNEL_MATERN1, mL, out);
}
extern "C" int hfmi_op_kernel_cross_cov_spec(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d,
                                             const hfmi_kernel_spec* spec, int64_t diag_offset, hfmi_op** out) {
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec_metric("kernel_cross_cov", spec, d, store, &mL));
  return kcov_cross_create(ctx, host_targets, M, host_sources, N, d, spec->family, spec->sigma, spec->ell, spec->nugget, diag_offset,
                           HFMI_KERNEL_MATERN1, mL, out);
}
extern "C" int hfmi_op_kernel_cov_rows_spec(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec* spec,
                                            int64_t row0, int64_t nrows, hfmi_op** out) {
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec_metric("kernel_cov_rows", spec, d, store, &mL));
  return kcov_rows_create(ctx, host_points, N, d, spec->family, spec->sigma, spec->ell, spec->nugget, row0, nrows, HFMI_KERNEL_MATERN1, mL, out);
}
extern "C" int hfmi_op_kernel_cov_grid_spec(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N,
                                            const hfmi_kernel_spec* spec, hfmi_op** out) {
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec_metric("kernel_cov_grid", spec, d, store, &mL));
  return kcov_grid_create(ctx, d, n, h, host_nodes, N, spec->family, spec->sigma, spec->ell, spec->nugget, HFMI_KERNEL_MATERN1, mL, out);
}
// the long route: split-line passes, longest line from the tuning key "fftcov_max_line" as it stands at creation
extern "C" int hfmi_op_kernel_cov_grid_long(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N,
                                            const hfmi_kernel_spec* spec, hfmi_op** out) {
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec_metric("kernel_cov_grid_long", spec, d, store, &mL));
  return kcov_grid_create(ctx, d, n, h, host_nodes, N, spec->family, spec->sigma, spec->ell, spec->nugget, HFMI_KERNEL_MATERN1, mL, out,
                          fftcov_max_line_knob());
}

// The hfmi_kernel_spec2 creators: the descriptor's first fields are a hfmi_kernel_spec, which goes the way it always went; nu is checked
// here (in range for HFMI_KERNEL_MATERN, 0 otherwise) and read by the creators for that family alone.
static int kcov_spec2_read(const char* who, const hfmi_kernel_spec2* spec2, int d, hfmi_kernel_spec* spec, double* store, const double** mL) {
  if (!spec2) HFMI_FAIL(HFMI_ERR_INVALID, "%s: null kernel descriptor", who);
  spec->family = spec2->family, spec->d = spec2->d;
  spec->sigma = spec2->sigma, spec->ell = spec2->ell, spec->nugget = spec2->nugget;
  for (int i = 0; i < 9; ++i) spec->metric[i] = spec2->metric[i];
  HFMI_TRY(kcov_spec_metric(who, spec, d, store, mL));
  if (spec2->family == HFMI_KERNEL_MATERN) {
    if (!isfinite(spec2->nu) || spec2->nu < HFMI_MATERN_NU_MIN || spec2->nu > HFMI_MATERN_NU_MAX)
      HFMI_FAIL(HFMI_ERR_INVALID, "%s: the smoothness nu = %g does not lie in [1/8, 8]", who, spec2->nu);
  } else if (spec2->nu != 0.0) {      // a NaN included
    HFMI_FAIL(HFMI_ERR_INVALID, "%s: nu = %g with kernel family %d: only HFMI_KERNEL_MATERN takes a smoothness", who, spec2->nu, spec2->family);
  }
  return HFMI_OK;
}
extern "C" int hfmi_op_kernel_cov_spec2(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec2* spec2, hfmi_op** out) {
  hfmi_kernel_spec spec;
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec2_read("kernel_cov", spec2, d, &spec, store, &mL));
  return kcov_create(ctx, host_points, N, d, spec.family, spec.sigma, spec.ell, spec.nugget, HFMI_KERNEL_MATERN, mL, out, spec2->nu);
}
extern "C" int hfmi_op_kernel_cross_cov_spec2(hfmi_ctx* ctx, const double* host_targets, int64_t M, const double* host_sources, int64_t N, int d,
                                              const hfmi_kernel_spec2* spec2, int64_t diag_offset, hfmi_op** out) {
  hfmi_kernel_spec spec;
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec2_read("kernel_cross_cov", spec2, d, &spec, store, &mL));
  return kcov_cross_create(ctx, host_targets, M, host_sources, N, d, spec.family, spec.sigma, spec.ell, spec.nugget, diag_offset,
                           HFMI_KERNEL_MATERN, mL, out, spec2->nu);
}
extern "C" int hfmi_op_kernel_cov_rows_spec2(hfmi_ctx* ctx, const double* host_points, int64_t N, int d, const hfmi_kernel_spec2* spec2,
                                             int64_t row0, int64_t nrows, hfmi_op** out) {
  hfmi_kernel_spec spec;
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec2_read("kernel_cov_rows", spec2, d, &spec, store, &mL));
  return kcov_rows_create(ctx, host_points, N, d, spec.family, spec.sigma, spec.ell, spec.nugget, row0, nrows, HFMI_KERNEL_MATERN, mL, out,
                          spec2->nu);
}
extern "C" int hfmi_op_kernel_cov_grid_spec2(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N,
                                             const hfmi_kernel_spec2* spec2, hfmi_op** out) {
  hfmi_kernel_spec spec;
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec2_read("kernel_cov_grid", spec2, d, &spec, store, &mL));
  return kcov_grid_create(ctx, d, n, h, host_nodes, N, spec.family, spec.sigma, spec.ell, spec.nugget, HFMI_KERNEL_MATERN, mL, out, 0, spec2->nu);
}
extern "C" int hfmi_op_kernel_cov_grid_long_spec2(hfmi_ctx* ctx, int d, const int64_t* n, const double* h, const int64_t* host_nodes, int64_t N,
                                                  const hfmi_kernel_spec2* spec2, hfmi_op** out) {
  hfmi_kernel_spec spec;
  double store[9];
  const double* mL = nullptr;
  HFMI_TRY(kcov_spec2_read("kernel_cov_grid_long", spec2, d, &spec, store, &mL));
  return kcov_grid_create(ctx, d, n, h, host_nodes, N, spec.family, spec.sigma, spec.ell, spec.nugget, HFMI_KERNEL_MATERN, mL, out,
                          fftcov_max_line_knob(), spec2->nu);
}
extern "C" int hfmi_op_csr(hfmi_ctx* ctx, const hfmi_csr* M, hfmi_op** out) {
  if (!ctx || !M || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_CSR);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->csr = M;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_csr_pcg(hfmi_ctx* ctx, const hfmi_csr* M, double rel_tol, int max_iter, hfmi_op** out) {
  if (!ctx || !M || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (M->nrows != M->ncols) HFMI_FAIL(HFMI_ERR_INVALID, "csr_pcg: matrix must be square");
  hfmi_op* op = op_new(ctx, OP_CSR_PCG);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->csr = M;
  op->rel_tol = rel_tol > 0 ? rel_tol : 1e-13;
  op->max_iter = max_iter > 0 ? max_iter : 500;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_amg_pcg(hfmi_ctx* ctx, hfmi_amg* amg, double rel_tol, int max_iter, hfmi_op** out) {
  if (!ctx || !amg || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_AMG_PCG);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->amg = amg;
  op->rel_tol = rel_tol > 0 ? rel_tol : 1e-12;
  op->max_iter = max_iter > 0 ? max_iter : 100;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_solver_info(const hfmi_op* op, int* iterations, int* method, double* lmin, double* lmax) {
  if (op && op->kind == OP_AMG_PCG) {
    if (iterations) *iterations = op->last_iters;
    if (method) *method = 2;
    if (lmin) *lmin = 0.0;
    if (lmax) *lmax = 0.0;
    return HFMI_OK;
  }
  if (!op || op->kind != OP_CSR_PCG) HFMI_FAIL(HFMI_ERR_INVALID, "op_solver_info: not a sparse solver operator");
  if (iterations) *iterations = op->last_iters;
  if (method) *method = op->last_method;
  if (lmin) *lmin = op->csr->solve.cheb_state == 1 ? op->csr->solve.cheb_lmin : 0.0;
  if (lmax) *lmax = op->csr->solve.cheb_state == 1 ? op->csr->solve.cheb_lmax : 0.0;
  return HFMI_OK;
}
extern "C" int hfmi_op_compose3(hfmi_ctx* ctx, hfmi_op* a, hfmi_op* b, hfmi_op* c, hfmi_op** out) {
  if (!ctx || !a || !b || !c || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_COMPOSE3);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->a = a;
  op->b = b;
  op->c = c;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_host_callback(hfmi_ctx* ctx, hfmi_host_apply_fn fn, void* user, int64_t N, hfmi_op** out) {
  if (!ctx || !fn || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_HOST);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->host_fn = fn;
  op->host_user = user;
  op->host_N = N;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_host_set_chunk(hfmi_op* op, int vectors) {
  if (!op || op->kind != OP_HOST) HFMI_FAIL(HFMI_ERR_INVALID, "op_host_set_chunk: not a host-callback operator");
  if (vectors < 0) HFMI_FAIL(HFMI_ERR_INVALID, "op_host_set_chunk: negative slab size");
  op->host_chunk = vectors;
  return HFMI_OK;
}
extern "C" int hfmi_op_set_post_apply(hfmi_op* op, hfmi_post_apply_fn fn, void* user) {
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "null op");
  op->post_fn = fn;
  op->post_user = user;
  return HFMI_OK;
}
extern "C" int hfmi_op_set_collective(hfmi_op* op, hfmi_comm* comm, int reduce_op) {
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "null op");
  if (comm && reduce_op != HFMI_REDUCE_SUM && reduce_op != HFMI_REDUCE_AVG)
    HFMI_FAIL(HFMI_ERR_INVALID, "op_set_collective: reduce_op must be HFMI_REDUCE_SUM or HFMI_REDUCE_AVG");
  op->comm = comm;
  op->comm_op = reduce_op;
  return HFMI_OK;
}
hfmi_op::~hfmi_op() {
  if (gamma_inv || weights || kc_x || kc_t || kc_nutab || fc || fac || ip || box) (void)hipStreamSynchronize(ctx->stream);   // a kernel may still read them
  fftcov_destroy(fc);
  interp_destroy(ip);
}
extern "C" int hfmi_op_destroy(hfmi_op* op) {
  delete op;
  return HFMI_OK;
}

// Host black box on a device block (hfmi_op_host_callback): W goes device -> pinned host, the callback fills Y on the
// host, Y goes pinned host -> device.  With a slab size (hfmi_op_host_set_chunk) the three legs are pipelined over
// slabs of vectors: while the host works on slab i, slab i+1 is already arriving on the auxiliary stream and slab i-1
// is on its way back on the main stream.  The host-side wall clock of the three legs is kept for the phase report.
static double wall_ms() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static int host_apply_pipelined(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_ctx* ctx = op->ctx;
  const int64_t N = W->N, NY = Y->N;
  const int k = W->nvec;
  const int chunk = (op->host_chunk > 0 && op->host_chunk < k) ? op->host_chunk : k;
  const int nchunks = (k + chunk - 1) / chunk;
  const size_t wslab = (size_t)chunk * N, yslab = (size_t)chunk * NY;
  const int nbuf = nchunks > 1 ? 2 : 1;
  OWN_TRY(grow(ctx->pinned_cb, (size_t)nbuf * (wslab + yslab), [&] { return (int)hipStreamSynchronize(ctx->stream); }));
  double* const cb = ctx->pinned_cb;
  double* wbuf[2] = {cb, cb + (nbuf - 1) * wslab};
  double* ybuf[2] = {cb + nbuf * wslab, cb + nbuf * wslab + (nbuf - 1) * yslab};
  auto fetch = [&](int c) -> int {      // slab c of W -> wbuf[c & 1] on the auxiliary stream
    const int c0 = c * chunk, nc = std::min(chunk, k - c0);
    HIP_TRY(hipMemcpy2DAsync(wbuf[c & 1], (size_t)N * sizeof(double), W->p + (int64_t)c0 * W->ld, (size_t)W->ld * sizeof(double),
                             (size_t)N * sizeof(double), (size_t)nc, hipMemcpyDeviceToHost, ctx->aux_stream));
    HIP_TRY(hipEventRecord(ctx->ev_cb[c & 1], ctx->aux_stream));
    return HFMI_OK;
  };
  // W is complete once the main stream reaches this point
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_status, 0));
  HFMI_TRY(fetch(0));
  double t_d2h = 0.0, t_fn = 0.0, t_h2d = 0.0;
  for (int c = 0; c < nchunks; ++c) {
    const int c0 = c * chunk, nc = std::min(chunk, k - c0);
    double t0 = wall_ms();
    HIP_TRY(hipEventSynchronize(ctx->ev_cb[c & 1]));                       // slab c has arrived
    if (c + 1 < nchunks) HFMI_TRY(fetch(c + 1));                           // wbuf[(c+1)&1] was consumed by call c-1
    double t1 = wall_ms();
    t_d2h += t1 - t0;
    if (c >= 2) HIP_TRY(hipEventSynchronize(ctx->ev_cb[2 + (c & 1)]));     // ybuf[c&1] has left for the device (slab c-2)
    double t2 = wall_ms();
    t_h2d += t2 - t1;
    memset(ybuf[c & 1], 0, (size_t)nc * NY * sizeof(double));
    const int rc = op->host_fn(op->host_user, wbuf[c & 1], ybuf[c & 1], N, nc);
    double t3 = wall_ms();
    t_fn += t3 - t2;
    if (rc != 0) {
      (void)hipStreamSynchronize(ctx->aux_stream);
      (void)hipStreamSynchronize(ctx->stream);
      HFMI_FAIL(HFMI_ERR_CALLBACK, "host operator callback returned %d", rc);
    }
    HIP_TRY(hipMemcpy2DAsync(Y->p + (int64_t)c0 * Y->ld, (size_t)Y->ld * sizeof(double), ybuf[c & 1], (size_t)NY * sizeof(double),
                             (size_t)NY * sizeof(double), (size_t)nc, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev_cb[2 + (c & 1)], ctx->stream));
    t_h2d += wall_ms() - t3;
  }
  double t0 = wall_ms();
  HIP_TRY(hipStreamSynchronize(ctx->stream));                              // the pinned slabs are free again
  t_h2d += wall_ms() - t0;
  if (ctx->profiling) {
    ctx->phase_ms[HFMI_PHASE_HOST_D2H] += t_d2h;
    ctx->phase_ms[HFMI_PHASE_HOST_FN] += t_fn;
    ctx->phase_ms[HFMI_PHASE_HOST_H2D] += t_h2d;
  }
  return HFMI_OK;
}

// Overlapped rank reduction of an operator application (collectiveOperator.py:73-80, collective.py:98-111): the
// last contraction of a Gram-form apply (Y = X^T G) is issued in row panels of whole rounds of tiles (hfmi_gemm_nn.hip), and
// as soon as a panel's rows are final they are packed into a contiguous buffer, all-reduced and unpacked on the AUXILIARY
// stream while the next panel is computed on the main one.  Only the last panel's reduction is exposed.  Same arithmetic per
// element as the one-launch product followed by one all-reduce of the block: bit-identical results (tests/test_gpu_comm.py).
struct panel_reduce {
  hfmi_op* op;
  int npanels;
  int64_t stage_off;     // doubles used in WS_COMM so far
  double* stage;
  int status;
};
static int panel_reduce_hook(void* user, double* Y, int64_t ldy, int r, int64_t row0, int64_t rows) {
  panel_reduce* pr = (panel_reduce*)user;
  hfmi_ctx* ctx = pr->op->ctx;
  if (pr->npanels >= 8) HFMI_FAIL(HFMI_ERR_INVALID, "panel_reduce: more than 8 row panels");
  hipEvent_t ev = ctx->ev_panel[pr->npanels++];
  HIP_TRY(hipEventRecord(ev, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ev, 0));
  double* st = pr->stage + pr->stage_off;
  const int64_t rld = round_up(rows, 2);
  pr->stage_off += rld * r;
  const int ph = phase_begin_on(ctx, HFMI_PHASE_ALLREDUCE_AUX, ctx->aux_stream);
  if (rld != rows) HIP_TRY(hipMemsetAsync(st, 0, (size_t)rld * r * sizeof(double), ctx->aux_stream));
  HIP_TRY(hipMemcpy2DAsync(st, (size_t)rld * sizeof(double), Y + row0, (size_t)ldy * sizeof(double), (size_t)rows * sizeof(double),
                           (size_t)r, hipMemcpyDeviceToDevice, ctx->aux_stream));
  HFMI_TRY(comm_allreduce_device_on(pr->op->comm, st, rld * r, pr->op->comm_op, ctx->aux_stream));
  HIP_TRY(hipMemcpy2DAsync(Y + row0, (size_t)ldy * sizeof(double), st, (size_t)rld * sizeof(double), (size_t)rows * sizeof(double),
                           (size_t)r, hipMemcpyDeviceToDevice, ctx->aux_stream));
  phase_end_on(ctx, ph, ctx->aux_stream);
  return HFMI_OK;
}

// the length of op's results on inputs of length in_len, for the kinds that can be rectangular and say so; in_len otherwise
static int64_t op_range_len(const hfmi_op* op, int64_t in_len) {
  switch (op->kind) {
    case OP_GRID_INTERP:
    case OP_INTERP_FACTOR: return interp_range_len(op);
    case OP_CSR: return op->csr->nrows;
    case OP_KERNEL_CROSS: return op->kc_slab ? in_len : op->kc_M;
    case OP_COMPOSE3: return op_range_len(op->c, op_range_len(op->b, op_range_len(op->a, in_len)));
    default: return in_len;
  }
}

static int op_apply_raw(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, double beta) {
  hfmi_ctx* ctx = op->ctx;
  const int k = W->nvec;
  // beta != 0 for an operator that cannot add to its output: the inner solve fills the temporary T, then Y <- beta Y + T
  auto accumulate = [&](hfmi_block& T, auto&& solve) -> int {
    HFMI_TRY(solve(&T));
    if (beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
    return launch_axpy(ctx, Y->p, Y->ld, 1.0, T.p, T.ld, Y->N, k);
  };
  switch (op->kind) {
    case OP_SNAPSHOT_GRAM:
    case OP_JTJ: {
      const hfmi_block& X = op->X;
      if (X.N != W->N) HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld", (long long)X.N, (long long)W->N);
      const int m = X.nvec;
      const int ldg = (int)round_up(k, 16);
      void* G = nullptr;
      HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)m * ldg * sizeof(double), &G));
      // G (m x k) = scale * X^T W ; then Y = X G
      HFMI_TRY(launch_tsgemm_tn(ctx, X.p, X.ld, m, W->p, W->ld, k, X.N, op->scale, 0.0, (double*)G, ldg, 1, 0));
      if (op->kind == OP_JTJ && op->gamma_inv)
        HFMI_TRY(launch_gamma_apply(ctx, (double*)G, ldg, op->ndata, op->q, k, op->gamma_inv, (int)round_up(op->q, 16)));
      if (op->weights) HFMI_TRY(launch_row_scale(ctx, (double*)G, ldg, m, k, op->weights));
      if (g_comm_panels < 0) {
        const char* e = getenv("HFMI_COMM_PANELS");
        g_comm_panels = e ? atoi(e) : 4;
        if (g_comm_panels < 0 || g_comm_panels > 8) g_comm_panels = 4;
      }
      if (op->comm && g_comm_panels > 1 && beta == 0.0 && comm_transport(op->comm) != 0 && k <= 256) {
        void* sv = nullptr;
        HFMI_TRY(ctx_ws(ctx, WS_COMM, ((size_t)Y->ld + 16) * k * sizeof(double), &sv));
        // the largest panel is at most the whole block: size the transport's staging area for that before the first panel is
        // in flight on the auxiliary stream (regrowing it later would close peers' mappings under a running reduction)
        HFMI_TRY(comm_reserve_stage(op->comm, ((size_t)Y->ld + 16) * k * sizeof(double)));
        panel_reduce pr = {op, 0, 0, (double*)sv, HFMI_OK};
        ctx->nn_hook = panel_reduce_hook;
        ctx->nn_hook_user = &pr;
        ctx->nn_hook_panels = g_comm_panels;
        ctx->nn_hook_called = false;
        const int s = launch_tsgemm_nn(ctx, X.p, X.ld, m, (const double*)G, ldg, k, 1.0, beta, Y->p, Y->ld, X.N);
        ctx->nn_hook = nullptr;
        if (s != HFMI_OK) return s;
        if (ctx->nn_hook_called) {
          // join: the main stream continues when the last panel is back
          const int ph = phase_begin(ctx, HFMI_PHASE_ALLREDUCE);
          HIP_TRY(hipEventRecord(ctx->ev_join, ctx->aux_stream));
          HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
          phase_end(ctx, ph);
          op->reduced_by_panels = true;
        }
        return HFMI_OK;
      }
      HFMI_TRY(launch_tsgemm_nn(ctx, X.p, X.ld, m, (const double*)G, ldg, k, 1.0, beta, Y->p, Y->ld, X.N));
      return HFMI_OK;
    }
    case OP_JJT: {
      // Y (q x k) = scale * sum_i J_i (J_i^T W): per sample  H_i (N x k) = J_i^T-as-block * W ; Y += J_i^T H_i
      const hfmi_block& J = op->X;
      const int q = op->q;
      if (W->N != q) HFMI_FAIL(HFMI_ERR_INVALID, "JJT acts on vectors of length %d, got %lld", q, (long long)W->N);
      hfmi_block H;
      HFMI_TRY(ctx_tmp_view(ctx, TMP_JJT_H, J.N, k, &H));
      // W as a small row-major (q x k) matrix: W block is column-major q x k with ld -> transpose into WS_G
      const int ldw = (int)round_up(k, 16);
      void* Ws = nullptr;
      HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)q * ldw * sizeof(double), &Ws));
      HIP_TRY(hipMemsetAsync(Ws, 0, (size_t)q * ldw * sizeof(double), ctx->stream));
      HFMI_TRY(launch_block_to_dense_ld(ctx, W->p, W->ld, (double*)Ws, ldw, q, k));
      for (int i = 0; i < op->ndata; ++i) {
        const double* Ji = J.p + (int64_t)i * q * J.ld;
        HFMI_TRY(launch_tsgemm_nn(ctx, Ji, J.ld, q, (const double*)Ws, ldw, k, 1.0, 0.0, H.p, H.ld, J.N));
        // Y[o][j] (+)= scale * <J_i row o, H_j>  -> column-major q x k output: rs = 1, cs = ld
        HFMI_TRY(launch_tsgemm_tn(ctx, Ji, J.ld, q, H.p, H.ld, k, J.N, op->scale, (i == 0) ? beta : 1.0, Y->p, 1, Y->ld, 0));
      }
      return HFMI_OK;
    }
    case OP_DENSE_SYM: {
      const hfmi_block& C = op->X;
      if (C.N != W->N) HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld", (long long)C.N, (long long)W->N);
      // Y = C W with C symmetric: Y[t][j] = <C_t, W_j>  (column-major output)
      return launch_tsgemm_tn(ctx, C.p, C.ld, C.nvec, W->p, W->ld, k, C.N, 1.0, beta, Y->p, 1, Y->ld, 0);
    }
    case OP_KERNEL_COV: {
      if (op->kc_N != W->N || op->kc_N != Y->N)
        HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld -> %lld", (long long)op->kc_N, (long long)W->N, (long long)Y->N);
      // Y (+)= C W: the kernel adds into Y itself
      return launch_kernel_cov(ctx, op->kc_x, op->kc_N, op->kc_d, op->kc_family, op->kc_sigma, op->kc_ell, op->kc_nugget, W->p, W->ld,
                               Y->p, Y->ld, k, beta != 0.0, op->kc_nu_ref());
    }
    case OP_KERNEL_COV_GRID: {
      const int64_t N = fftcov_points(op->fc);
      if (N != W->N || N != Y->N)
        HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld -> %lld", (long long)N, (long long)W->N, (long long)Y->N);
      // Y (+)= C W: the gather of the last pass adds into Y itself
      return fftcov_apply(ctx, op->fc, W->p, W->ld, Y->p, Y->ld, k, beta != 0.0);
    }
    case OP_GRID_FACTOR:
      // Y (+)= S W or S^T W: the last pass adds into Y itself
      return fftcov_factor_apply(ctx, op->fac.get(), op->fac_transpose, W, Y, beta != 0.0);
    case OP_BOX: {
      const int64_t N = boxcov_points(op->box.get());
      if (N != W->N || N != Y->N)
        HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld -> %lld", (long long)N, (long long)W->N, (long long)Y->N);
      // Y (+)= W^a T_s W^b X: the gather of the last pass adds into Y itself
      return boxcov_apply(ctx, op->box.get(), op->box_table, op->box_a, op->box_b, W->p, W->ld, Y->p, Y->ld, k, beta != 0.0);
    }
    case OP_GRID_INTERP:
    case OP_KERNEL_COV_INTERP:
      // Y (+)= W X, W^T X or K X: the last kernel adds into Y itself
      return interp_apply(op, W, Y, beta != 0.0);
    case OP_INTERP_FACTOR:
      // Y (+)= F W or F^T W: the gather, or the last pass and the tail kernel, add into Y themselves
      return interp_factor_apply(op, W, Y, beta != 0.0);
    case OP_KERNEL_CROSS: {
      const int64_t N = op->kc_N, M = op->kc_M;
      const int acc = beta != 0.0;
      if (!op->kc_slab) {
        if (N != W->N || M != Y->N)
          HFMI_FAIL(HFMI_ERR_INVALID, "operator maps vectors of length %lld to length %lld, got %lld -> %lld", (long long)N, (long long)M,
                    (long long)W->N, (long long)Y->N);
        return launch_kernel_cross_cov(ctx, op->kc_x, N, op->kc_t, M, M, op->kc_diag, op->kc_d, op->kc_family, op->kc_sigma, op->kc_ell,
                                       op->kc_nugget, W->p, W->ld, Y->p, Y->ld, k, acc, op->kc_nu_ref());
      }
      if (N != W->N || N != Y->N)
        HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld -> %lld", (long long)N, (long long)W->N, (long long)Y->N);
      // rows row0 .. row0 + M - 1 of C W; an overwriting apply leaves +0.0 in the other rows below N (the rows from N on are zero already)
      const int64_t row0 = op->kc_diag, row1 = row0 + M;
      if (!acc) {
        if (row0 > 0)
          HIP_TRY(hipMemset2DAsync(Y->p, (size_t)Y->ld * sizeof(double), 0, (size_t)row0 * sizeof(double), (size_t)k, ctx->stream));
        if (row1 < N)
          HIP_TRY(hipMemset2DAsync(Y->p + row1, (size_t)Y->ld * sizeof(double), 0, (size_t)(N - row1) * sizeof(double), (size_t)k, ctx->stream));
      }
      return launch_kernel_cross_cov(ctx, op->kc_x, N, op->kc_x + row0, M, N, row0, op->kc_d, op->kc_family, op->kc_sigma, op->kc_ell,
                                     op->kc_nugget, W->p, W->ld, Y->p + row0, Y->ld, k, acc, op->kc_nu_ref());
    }
    case OP_CSR: {
      if (op->csr->ncols != W->N || op->csr->nrows != Y->N) HFMI_FAIL(HFMI_ERR_INVALID, "csr operator / block shape mismatch");
      if (beta != 0.0 && beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
      return launch_csr_spmm(ctx, op->csr, W->p, W->ld, Y->p, Y->ld, k, beta != 0.0);
    }
    case OP_CSR_PCG:
    case OP_AMG_PCG: {
      auto solve = [&](hfmi_block* D) { return op->kind == OP_CSR_PCG ? csr_pcg_solve(op, W, D) : amg_pcg_solve(op, W, D); };
      if (beta == 0.0) return solve(Y);
      hfmi_block T;
      HFMI_TRY(ctx_tmp_view(ctx, TMP_ACCUM, W->N, k, &T));
      return accumulate(T, solve);
    }
    case OP_COMPOSE3: {
      // a composition inside a composition (M C M with C = A^-1 M A^-1 itself composed) takes its own pair of temporaries
      const int depth = ctx->compose_depth;
      if (depth >= 4) HFMI_FAIL(HFMI_ERR_INVALID, "compose3: operators nested more than 4 deep");
      struct depth_guard {
        hfmi_ctx* c;
        ~depth_guard() { --c->compose_depth; }
      } guard{ctx};
      ++ctx->compose_depth;
      hfmi_block v1, v2;
      // the temporaries take the length a part is known to map to (op_range_len: the input's length for every square kind)
      const int64_t n1 = op_range_len(op->a, W->N), n2 = op_range_len(op->b, n1);
      HFMI_TRY(ctx_tmp_view(ctx, tmp_compose_slot(depth), n1, k, &v1));
      HFMI_TRY(ctx_tmp_view(ctx, tmp_compose_slot(depth) + 1, n2, k, &v2));
      HFMI_TRY(hfmi_op_apply(op->a, W, &v1, 0));
      HFMI_TRY(hfmi_op_apply(op->b, &v1, &v2, 0));
      if (beta == 0.0) return hfmi_op_apply(op->c, &v2, Y, 0);
      if (v1.N != Y->N) HFMI_TRY(ctx_tmp_view(ctx, tmp_compose_slot(depth), Y->N, k, &v1));   // a rectangular chain: v1 has been consumed
      return accumulate(v1, [&](hfmi_block* D) { return hfmi_op_apply(op->c, &v2, D, 0); });
    }
    case OP_HOST: {
      const int64_t N = W->N;
      if (op->host_N > 0 && op->host_N != N) HFMI_FAIL(HFMI_ERR_INVALID, "host operator acts on vectors of length %lld, got %lld", (long long)op->host_N, (long long)N);
      if (beta == 0.0) return host_apply_pipelined(op, W, Y);
      hfmi_block T;
      HFMI_TRY(ctx_tmp_view(ctx, TMP_ACCUM, Y->N, k, &T));
      return accumulate(T, [&](hfmi_block* D) { return host_apply_pipelined(op, W, D); });
    }
  }
  HFMI_FAIL(HFMI_ERR_INVALID, "unknown operator kind");
}

extern "C" int hfmi_op_apply(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, int accumulate) {
  if (!op || !W || !Y) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (W->nvec != Y->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "x and y have non-matching number of vectors (%d vs %d)", W->nvec, Y->nvec);
  if (W->p == Y->p) HFMI_FAIL(HFMI_ERR_INVALID, "op_apply: input and output blocks must not alias");
  HIP_TRY(hipSetDevice(op->ctx->device));
  if (accumulate && (op->post_fn || op->comm)) HFMI_FAIL(HFMI_ERR_INVALID, "op_apply: accumulate with a rank reduction attached is ambiguous");
  op->reduced_by_panels = false;
  HFMI_TRY(op_apply_raw(op, W, Y, accumulate ? 1.0 : 0.0));
  if (op->comm && !op->reduced_by_panels) {
    const int ph = phase_begin(op->ctx, HFMI_PHASE_ALLREDUCE);
    HFMI_TRY(comm_allreduce_device(op->comm, Y->p, Y->ld * (int64_t)Y->nvec, op->comm_op));
    phase_end(op->ctx, ph);
  }
  if (op->post_fn) {
    const int rc = op->post_fn(op->post_user, Y);
    if (rc != 0) HFMI_FAIL(HFMI_ERR_CALLBACK, "post-apply hook returned %d", rc);
  }
  return HFMI_OK;
}
