// Small dense entry points and the fused randomized eigensolves of libhfmi.so (include/hfmi.h): Rayleigh-Ritz, SVD and LU
// on host matrices, the double pass, the single pass and the sketch core.  Host side only.
#include <string.h>

#include <cmath>

#include "hfmi_internal.h"

// ------------------------------------------------------------------ Rayleigh-Ritz
extern "C" int hfmi_sym_eig_small(hfmi_ctx* ctx, const double* host_T, int k, int sort_by_abs, double* host_d, double* host_V) {
  if (!ctx || !host_T || !host_d) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > HFMI_EIG_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "sym_eig_small: k=%d out of range [1,%d]", k, HFMI_EIG_MAXN);
  HIP_TRY(hipSetDevice(ctx->device));
  if (k > SM_MAXK) return sym_eig_large(ctx, host_T, k, sort_by_abs, host_d, host_V);   // whole-GPU blocked solver (checks its input on the device)
  for (size_t i = 0; i < (size_t)k * k; ++i)
    if (!std::isfinite(host_T[i])) HFMI_FAIL(HFMI_ERR_NUMERIC, "sym_eig (n=%d): the matrix has non-finite entries", k);
  HFMI_TRY(upload_small(ctx, host_T, k, k, sm_ptr(ctx, SM_T), SM_LD));
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  HFMI_TRY(launch_sym_eig(ctx, k, SM_T, SM_V, (double*)dv, sort_by_abs & 1, (sort_by_abs >> 1) & 1));
  hfmi_status_words st;
  HFMI_TRY(read_status(ctx, &st));
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "sym_eig_small: eigensolver did not converge (off-diagonal %.2e)", st.offdiag);
  HFMI_TRY(read_back(ctx, (const double*)dv, k, host_d));
  if (host_V) {
    std::vector<double> tmp((size_t)k * SM_LD);
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_V), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_V + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  return HFMI_OK;
}

// np.linalg.svd of the small triangular factor inside hp.accuracyEnhancedSVD
// the same with only the nvec leading eigenvectors (in output order) returned: host_V is k x nvec row-major.  What the deterministic
// POD needs of la.eigh(G) (PODProjector.py:821-826: U[:, :u_rank]); beyond 256 the back-transformation and the read-back then run
// over nvec columns instead of k
extern "C" int hfmi_sym_eig_leading(hfmi_ctx* ctx, const double* host_T, int k, int sort_by_abs, int nvec, double* host_d, double* host_V) {
  if (!ctx || !host_T || !host_d || !host_V) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > HFMI_EIG_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "sym_eig_leading: k=%d out of range [1,%d]", k, HFMI_EIG_MAXN);
  if (nvec < 1 || nvec > k) HFMI_FAIL(HFMI_ERR_INVALID, "sym_eig_leading: nvec=%d out of range [1,%d]", nvec, k);
  HIP_TRY(hipSetDevice(ctx->device));
  if (k > SM_MAXK) return sym_eig_large(ctx, host_T, k, sort_by_abs, host_d, host_V, nvec);
  std::vector<double> full((size_t)k * k);
  HFMI_TRY(hfmi_sym_eig_small(ctx, host_T, k, sort_by_abs, host_d, full.data()));
  for (int i = 0; i < k; ++i) memcpy(host_V + (size_t)i * nvec, full.data() + (size_t)i * k, (size_t)nvec * sizeof(double));
  return HFMI_OK;
}

// la.eigh(X^T (M X)) of the deterministic POD in one call (PODProjector.py:818-826: UtMU = u_data @ M @ u_data.T; eigh; U[:, :u_rank]):
// the n x n Gram matrix of two blocks is formed on the device and goes straight into the eigensolver -- no n x n matrix crosses
// PCIe in either direction, only the n eigenvalues and the nvec wanted eigenvectors come back (host_V: n x nvec row-major).
extern "C" int hfmi_block_gram_eig(const hfmi_block* A, const hfmi_block* B, int sort_by_abs, int nvec, double* host_d, double* host_V) {
  if (!A || !B || !host_d || !host_V) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->N != B->N) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: vector lengths differ (%lld vs %lld)", (long long)A->N, (long long)B->N);
  if (A->nvec != B->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: the blocks hold %d and %d vectors", A->nvec, B->nvec);
  const int n = A->nvec;
  if (n < 1 || n > HFMI_EIG_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: n=%d out of range [1,%d]", n, HFMI_EIG_MAXN);
  if (nvec < 1 || nvec > n) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: nvec=%d out of range [1,%d]", nvec, n);
  hfmi_ctx* ctx = A->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  void* out = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)n * n * sizeof(double), &out));
  HFMI_TRY(launch_tsgemm_tn(ctx, A->p, A->ld, n, B->p, B->ld, n, A->N, 1.0, 0.0, (double*)out, n, 1, 0));
  if (n > SM_MAXK) return sym_eig_large(ctx, nullptr, n, sort_by_abs, host_d, host_V, nvec, (const double*)out);
  std::vector<double> G((size_t)n * n);
  HFMI_TRY(read_back(ctx, (const double*)out, (size_t)n * n, G.data()));
  return hfmi_sym_eig_leading(ctx, G.data(), n, sort_by_abs, nvec, host_d, host_V);
}

extern "C" int hfmi_svd_small(hfmi_ctx* ctx, const double* host_R, int k, double* host_sigma, double* host_U, double* host_V) {
  if (!ctx || !host_R || !host_sigma) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "svd_small: k=%d out of range [1,%d]", k, SM_MAXK);
  HIP_TRY(hipSetDevice(ctx->device));
  for (size_t i = 0; i < (size_t)k * k; ++i)
    if (!std::isfinite(host_R[i])) HFMI_FAIL(HFMI_ERR_NUMERIC, "svd_small (k=%d): the matrix has non-finite entries", k);
  HFMI_TRY(upload_small(ctx, host_R, k, k, sm_ptr(ctx, SM_T), SM_LD));
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  HFMI_TRY(launch_jacobi_svd(ctx, k, SM_T, SM_R, SM_V, (double*)dv));
  hfmi_status_words st;
  HFMI_TRY(read_status(ctx, &st));
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "svd_small: one-sided Jacobi did not converge (max cosine %.2e)", st.offdiag);
  HFMI_TRY(read_back(ctx, (const double*)dv, k, host_sigma));
  std::vector<double> tmp((size_t)k * SM_LD);
  if (host_U) {
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_R), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_U + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  if (host_V) {
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_V), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_V + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  return HFMI_OK;
}

// ------------------------------------------------------------------ fused double pass
// Rayleigh quotient T = Q^T A Q for operators of Gram form A = scale * X^T Gamma X (snapshot Gram, mean J^T J):
//   T = scale * (X Q)^T Gamma (X Q)
// -- the same matrix as the reference's (A Q)^T Q by associativity, symmetric by construction, and it needs only the
// reduction GEMM G = X Q (no N x k block A Q, i.e. one of the four big contractions of the solve disappears).  A rank
// average attached to the operator (CollectiveOperator 'avg'/'sum') is linear, so the hook is applied to T itself: the
// second all-reduce of the solve shrinks from N x k to k x k.
static bool op_has_gram_form(const hfmi_op* A) { return (A->kind == OP_SNAPSHOT_GRAM && !A->weights) || A->kind == OP_JTJ; }

// fold_rinv: Q stands for Q R^-1 with R^-1 in SM_RINV (deferred last QR pass): X (Q R^-1) = (X Q) R^-1 is applied to
// the small m x k intermediate instead of the N x k block.
static int op_rayleigh_quotient_gram(hfmi_op* A, const hfmi_block* Q, int slot_T, bool fold_rinv = false) {
  hfmi_ctx* ctx = A->ctx;
  const hfmi_block& X = A->X;
  if (X.N != Q->N) HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld", (long long)X.N, (long long)Q->N);
  const int m = X.nvec, k = Q->nvec;
  const int64_t ldm = round_up(m, 32);
  const bool gam = (A->kind == OP_JTJ && A->gamma_inv != nullptr);
  void* gv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)ldm * k * sizeof(double) * (gam ? 2 : 1), &gv));
  double* Gc = (double*)gv;                          // (m x k), column-major: a block of k vectors of length m
  double* Gc2 = gam ? Gc + ldm * k : Gc;
  HFMI_TRY(launch_tsgemm_tn(ctx, X.p, X.ld, m, Q->p, Q->ld, k, X.N, 1.0, 0.0, Gc, 1, ldm, 0));
  HFMI_TRY(launch_zero_pad(ctx, Gc, m, k, ldm));
  if (fold_rinv) HFMI_TRY(launch_nn_upper(ctx, Gc, ldm, k, sm_ptr(ctx, SM_RINV), SM_LD, k, Gc, ldm, m));
  if (gam) {
    HFMI_TRY(launch_gamma_apply_cm(ctx, Gc, Gc2, ldm, A->ndata, A->q, k, A->gamma_inv, (int)round_up(A->q, 16)));
    HFMI_TRY(launch_zero_pad(ctx, Gc2, m, k, ldm));
  }
  HFMI_TRY(launch_tsgemm_tn(ctx, Gc, ldm, k, Gc2, ldm, k, m, A->scale, 0.0, sm_ptr(ctx, slot_T), SM_LD, 1, 0));
  if (A->comm) {
    const int ph = phase_begin(ctx, HFMI_PHASE_ALLREDUCE);
    HFMI_TRY(comm_allreduce_device(A->comm, sm_ptr(ctx, slot_T), (int64_t)SM_LD * k, A->comm_op));
    phase_end(ctx, ph);
  }
  if (A->post_fn) {
    hfmi_block t;
    t.ctx = ctx;
    t.p = sm_ptr(ctx, slot_T);
    t.N = SM_LD;
    t.nvec = k;
    t.ld = SM_LD;
    t.owner = false;
    const int rc = A->post_fn(A->post_user, &t);
    if (rc != 0) HFMI_FAIL(HFMI_ERR_CALLBACK, "post-apply hook returned %d", rc);
  }
  return HFMI_OK;
}

// Power iterations without orthogonalisation, X_0 = Omega (never modified), X_i = (B^-1) A X_{i-1}, for the double and the single
// pass at any width (panels of 256 beyond that).  The iterates alternate between X0 and X1; with B^-1 the product A X_{i-1} lands
// in Ybar, or, when the caller keeps none, in X1 -- every iterate is then X0.  prev / cur: X_{s-1} and X_s.
struct power_iter {
  hfmi_op *A, *Binv;
  const hfmi_block* Omega;
  int s;
  hfmi_block *X0, *X1, *Ybar;
  const hfmi_block *prev, *cur;
};
static int solve_power_iterations(power_iter& it) {
  hfmi_ctx* ctx = it.Omega->ctx;
  hfmi_block* const ax = it.Binv ? (it.Ybar ? it.Ybar : it.X1) : nullptr;
  it.prev = it.cur = it.Omega;
  for (int i = 0; i < it.s; ++i) {
    hfmi_block* dst = (it.cur == it.X0 && ax != it.X1) ? it.X1 : it.X0;
    int ph = phase_begin(ctx, HFMI_PHASE_APPLY);
    HFMI_TRY(op_apply_panels(it.A, it.cur, it.Binv ? ax : dst));
    phase_end(ctx, ph);
    if (it.Binv) {
      ph = phase_begin(ctx, HFMI_PHASE_BINV);
      HFMI_TRY(op_apply_panels(it.Binv, ax, dst));
      phase_end(ctx, ph);
    }
    it.prev = it.cur;
    it.cur = dst;
  }
  return HFMI_OK;
}

// Q = orth(X_s) in place: Gram-Schmidt with flag 2, else Cholesky-QR WITHOUT the safety copy hfmi_borth_qr(AUTO) keeps (a pass over
// N x k): if a column turns out to be numerically dependent, the block is recomputed from Omega (deterministic, every rank takes the
// same branch) and handed to the reference's Gram-Schmidt rule
static int solve_orthonormalise(power_iter& it, hfmi_op* B, int flags, qr_policy policy, qr_result* qr) {
  hfmi_block* Qp = const_cast<hfmi_block*>(it.cur);
  *qr = qr_result();
  if (flags & 2) return hfmi_borth_qr(Qp, B, nullptr, nullptr, HFMI_QR_MGS, nullptr);
  const int qs = qr_chol(Qp, B, nullptr, false, policy, qr);
  if (qs != HFMI_ERR_NUMERIC) return qs;
  *qr = qr_result();
  HFMI_TRY(solve_power_iterations(it));
  return hfmi_borth_qr(Qp, B, nullptr, nullptr, HFMI_QR_MGS, nullptr);
}

static int check_lu_words(const hfmi_status_words* lu_st, const char* who, bool has_B) {
  if (lu_st->failed == 1) HFMI_FAIL(HFMI_ERR_NUMERIC, "%s: the sketch products W = P^T Q / Z = Y^T Q have non-finite entries", who);
  if (lu_st->failed == 3) HFMI_FAIL(HFMI_ERR_NUMERIC, "%s: the solve W^-1 Z overflowed (non-finite pivot or solution)", who);
  if (lu_st->failed)
    HFMI_FAIL(HFMI_ERR_NUMERIC, "%s: rank-deficient sketch: W = P^T %sQ is singular (min |pivot| %.2e, max |pivot| %.2e); "
              "the probe block has dependent columns or the operator's range is smaller than the sketch", who, has_B ? "B " : "",
              lu_st->min_pivot_ratio, lu_st->gram_dev);
  return HFMI_OK;
}

// The tail of every fused solve of at most 256 vectors, T in SM_T: eigensolve; status words and eigenvalues to pinned memory on the
// auxiliary stream beside the back-transformation U = Q (S V[:, :r]) instead of behind it; both streams synchronised; then the
// checks in the order communicator, the caller's LU status words (lu_st, single pass), the orthogonalisation passes taken on trust
// (qr->late: *repeat_checked = true and HFMI_OK when they did not hold -- the caller repeats the solve on the checked path, which
// decides between the Gram-Schmidt fall-back and an error), the eigensolver.
// back: the small product S V that goes in front of U = Q ...; the two products also zero pad V[:, :r] to the 16 columns tsgemm_nn
// expects (the eigensolver leaves SM_V's pad columns as they were)
enum tail_back { BACK_V, BACK_RINV_V /* Q stands for Q R^-1, R^-1 in SM_RINV */, BACK_IDENTITY_V };
static int solve_tail(const hfmi_block* Q, int r, int flags, tail_back back, const qr_result* qr, const hfmi_status_words* lu_st, bool has_B,
                      const char* who, double* host_d, hfmi_block* U, bool* repeat_checked) {
  hfmi_ctx* ctx = Q->ctx;
  const int k = Q->nvec;
  const bool late = qr && qr->late;
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  int ph = phase_begin(ctx, HFMI_PHASE_EIG);
  if (late) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));   // the late-check copies read the status words (done ms ago)
  HFMI_TRY(launch_sym_eig(ctx, k, SM_T, SM_V, (double*)dv, flags & 1, (flags >> 3) & 1));
  phase_end(ctx, ph);
  void* dpin = nullptr;
  HFMI_TRY(ctx_pinned(ctx, (size_t)r * sizeof(double), &dpin));
  HFMI_TRY(side_copies_begin(ctx));        // no side_copies_end: nothing overwrites the sources before the synchronisation below
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HIP_TRY(hipMemcpyAsync(dpin, dv, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream));
  ph = phase_begin(ctx, HFMI_PHASE_BACK);
  if (back == BACK_IDENTITY_V) HFMI_TRY(launch_small_set_identity(ctx, k, SM_GRAM));
  if (back != BACK_V) HFMI_TRY(launch_small_matmul(ctx, k, r, back == BACK_RINV_V ? SM_RINV : SM_GRAM, SM_V, SM_TMP2));
  HFMI_TRY(launch_tsgemm_nn(ctx, Q->p, Q->ld, k, sm_ptr(ctx, back == BACK_V ? SM_V : SM_TMP2), SM_LD, r, 1.0, 0.0, U->p, U->ld, Q->N));
  phase_end(ctx, ph);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
  HFMI_TRY(ctx_check_comm(ctx));
  if (lu_st) HFMI_TRY(check_lu_words(lu_st, who, has_B));
  memcpy(host_d, dpin, (size_t)r * sizeof(double));
  const hfmi_status_words st = *ctx->status_host;
  print_status_dbg(&st);
  if (late && !qr_late_stands((const qr_late_buffer*)ctx->late_pinned.get(), k, qr->first_trusted)) {
    *repeat_checked = true;
    return HFMI_OK;
  }
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "%s: small eigensolve did not converge (off-diagonal %.2e)", who, st.offdiag);
  return HFMI_OK;
}

// Rayleigh-Ritz of the double pass in the fixed arena (k <= 256): T in Gram form (see above; qr.deferred folds R^-1 in) or literally
// (A Q)^T Q as the reference forms it, the one-CU eigensolver, U = Q V or Q (R^-1 V)
static int rayleigh_ritz_narrow(hfmi_op* A, const hfmi_block* Qp, hfmi_block* AQ, bool gram_path, const qr_result& qr, int r, int flags,
                                double* host_d, hfmi_block* U, bool* repeat_checked) {
  hfmi_ctx* ctx = Qp->ctx;
  const int k = Qp->nvec;
  const int ph = phase_begin(ctx, HFMI_PHASE_RAYLEIGH);
  if (gram_path) {
    HFMI_TRY(op_rayleigh_quotient_gram(A, Qp, SM_T, qr.deferred));
  } else {
    HFMI_TRY(hfmi_op_apply(A, Qp, AQ, 0));
    HFMI_TRY(launch_tsgemm_tn(ctx, AQ->p, AQ->ld, k, Qp->p, Qp->ld, k, Qp->N, 1.0, 0.0, sm_ptr(ctx, SM_T), SM_LD, 1, 0));
  }
  phase_end(ctx, ph);
  return solve_tail(Qp, r, flags, qr.deferred ? BACK_RINV_V : BACK_V, &qr, nullptr, false, "double_pass", host_d, U, repeat_checked);
}

// ... and in the wide arena (256 < k <= HFMI_WIDE_MAXK): ALWAYS the literal T = (A Q)^T Q, A applied in column panels of 256 -- the
// Gram-form shortcut and the trusted / deferred orthogonalisation passes stay narrow-only; T goes to the whole-GPU eigensolver
// (sym_eig_large, device input), whose k x r eigenvectors come back through the host and are uploaded for U = Q V
static int rayleigh_ritz_wide(hfmi_op* A, const hfmi_block* Qp, hfmi_block* AQ, int r, int flags, double* host_d, hfmi_block* U) {
  hfmi_ctx* ctx = Qp->ctx;
  const int64_t N = Qp->N;
  const int k = Qp->nvec;
  int ph = phase_begin(ctx, HFMI_PHASE_RAYLEIGH);
  double* T = wa_ptr(ctx, WA_T);                       // k x k, contiguous (ld = k): what sym_eig_large reads
  HFMI_TRY(op_apply_panels(A, Qp, AQ));
  HFMI_TRY(launch_tsgemm_tn(ctx, AQ->p, AQ->ld, k, Qp->p, Qp->ld, k, N, 1.0, 0.0, T, k, 1, 0));
  phase_end(ctx, ph);
  ph = phase_begin(ctx, HFMI_PHASE_EIG);
  std::vector<double> d(k), V((size_t)k * r);
  const int es = sym_eig_large(ctx, nullptr, k, flags & 1, d.data(), V.data(), r, T);
  phase_end(ctx, ph);
  HFMI_TRY(es);
  ph = phase_begin(ctx, HFMI_PHASE_BACK);
  const int ldv = (int)round_up(r, 32);                // <= round_up(k, 32): fits a slot of the arena
  HFMI_TRY(upload_small(ctx, V.data(), k, r, wa_ptr(ctx, WA_V), ldv));
  HFMI_TRY(launch_tsgemm_nn(ctx, Qp->p, Qp->ld, k, wa_ptr(ctx, WA_V), ldv, r, 1.0, 0.0, U->p, U->ld, N));
  phase_end(ctx, ph);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HFMI_TRY(ctx_check_comm(ctx));
  memcpy(host_d, d.data(), (size_t)r * sizeof(double));
  return HFMI_OK;
}

// hippylib's doublePass / doublePassG: power iterations, orthonormalisation, Rayleigh-Ritz in the arena the width calls for.
// late_checks: the first two Cholesky-QR passes of a Gram-form solve without B may be taken on trust (QR_TRUSTED); when they did not
// hold, the solve is repeated from Omega with every pass checked.
static int double_pass_impl(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                            double* host_d, hfmi_block* U, bool late_checks = true) {
  if (!A || !Omega || !host_d || !U) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = Omega->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t N = Omega->N;
  const int k = Omega->nvec;
  if (k < r) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: Omega has %d vectors, need at least the rank %d", k, r);
  if (r < 1) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: rank must be positive");
  if (U->N != N || U->nvec != r) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: U must be %lld x %d", (long long)N, r);
  if (k > HFMI_WIDE_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: at most %d probe vectors (got %d)", HFMI_WIDE_MAXK, k);
  if (s < 1) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: s must be >= 1");
  const bool wide = k > SM_MAXK;
  if (wide) HFMI_TRY(ctx_wide(ctx, k));
  hfmi_block Q, Y;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_SOLVE_Q, N, k, &Q));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_SOLVE_Y, N, k, &Y));
  power_iter it = {A, Binv, Omega, s, &Q, &Y, nullptr, Omega, Omega};
  HFMI_TRY(solve_power_iterations(it));
  hfmi_block* Qp = const_cast<hfmi_block*>(it.cur);        // holds the block to orthogonalise
  hfmi_block* AQ = (Qp == &Q) ? &Y : &Q;
  const bool gram_path = !wide && op_has_gram_form(A) && !(flags & 4);
  const qr_policy policy = !gram_path ? QR_CHECKED : (late_checks && !B) ? QR_TRUSTED : QR_DEFERRED;
  qr_result qr;
  const int ph = phase_begin(ctx, HFMI_PHASE_QR);
  HFMI_TRY(solve_orthonormalise(it, B, flags, policy, &qr));
  phase_end(ctx, ph);
  bool repeat_checked = false;
  if (wide) HFMI_TRY(rayleigh_ritz_wide(A, Qp, AQ, r, flags, host_d, U));
  else HFMI_TRY(rayleigh_ritz_narrow(A, Qp, AQ, gram_path, qr, r, flags, host_d, U, &repeat_checked));
  return repeat_checked ? double_pass_impl(A, B, Binv, Omega, r, s, flags, host_d, U, false) : HFMI_OK;
}

extern "C" int hfmi_double_pass(hfmi_op* A, const hfmi_block* Omega, int r, int s, int flags, double* host_d, hfmi_block* U) {
  return double_pass_impl(A, nullptr, nullptr, Omega, r, s, flags, host_d, U);
}
extern "C" int hfmi_double_pass_g(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                                  double* host_d, hfmi_block* U) {
  if (!B || !Binv) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass_g: B and Binv are required");
  return double_pass_impl(A, B, Binv, Omega, r, s, flags, host_d, U);
}

// ------------------------------------------------------------------ fused single pass
// hippylib's singlePass / singlePassG (randomizedEigensolver): the Rayleigh-Ritz matrix comes from the sketch itself instead of
// a further application of the operator.  With P = X_{s-1}, Y = X_s (X_0 = Omega, X_i = (B^-1) A X_{i-1}) and Q an
// orthonormal (B-orthonormal) basis of range(Y):
//   A ~ Q T Q^T (B Q T Q^T B)  =>  Q^T B Y = T (Q^T B P)  =>  Wt T^T = Zt,  Wt = P^T (B Q),  Zt = Ybar^T Q
// (Ybar = A X_{s-1}; Ybar = Y without B), so T^T = Wt^-1 Zt, symmetrised.  The core below works on a sketch the caller
// holds (hfmi_sketch_eig, streamed sketches) or the one single_pass_impl has just built: Q = orth(Y) with the same
// Cholesky-QR / Gram-Schmidt rule as the double pass, the two m x m products, the LU solve (k_lu_solve writes T straight
// into the eigensolver's slot), the eigensolve and U = Q V[:, :r], all on the context's stream.  The host waits only where the
// double pass's checked route does (the status words of each orthogonalisation pass) and once at the end.
// Q_work may alias Y for the generalized problem (Y itself is not needed after its orthogonalisation there).
static int sketch_eig_core(const hfmi_block* P, const hfmi_block* Y, const hfmi_block* Ybar, hfmi_op* B, hfmi_block* Q_work,
                           hfmi_block* BQ_work, int r, int flags, double* host_d, hfmi_block* U, const char* who) {
  hfmi_ctx* ctx = P->ctx;
  const int64_t N = P->N;
  const int k = P->nvec;
  if (Q_work->p != Y->p) HFMI_TRY(launch_copy(ctx, Q_work->p, Q_work->ld, Y->p, Y->ld, N, k));
  int ph = phase_begin(ctx, HFMI_PHASE_QR);
  // exact triangular factors in every pass (want_r, see borth_qr), nothing read back: U = Q V orthonormal to round-off
  HFMI_TRY(borth_qr(Q_work, B, B ? BQ_work : nullptr, nullptr, true, (flags & 2) ? HFMI_QR_MGS : HFMI_QR_AUTO, nullptr));
  phase_end(ctx, ph);
  ph = phase_begin(ctx, HFMI_PHASE_RAYLEIGH);
  const hfmi_block* right = B ? BQ_work : Q_work;
  const hfmi_block* left = B ? Ybar : Y;
  HFMI_TRY(launch_tsgemm_tn(ctx, P->p, P->ld, k, right->p, right->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_GRAM), SM_LD, 1, 0));
  HFMI_TRY(launch_tsgemm_tn(ctx, left->p, left->ld, k, Q_work->p, Q_work->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_R), SM_LD, 1, 0));
  HFMI_TRY(launch_lu_solve(ctx, k, SM_GRAM, SM_R, SM_TMP, SM_TMP2, SM_T));
  phase_end(ctx, ph);
  // the solve's status words leave for pinned memory (the late-check buffer's first slot) before the eigensolver reuses them
  qr_late_buffer* pin = nullptr;
  HFMI_TRY(ctx_late_pinned(ctx, &pin));
  HFMI_TRY(side_copies_begin(ctx));
  HIP_TRY(hipMemcpyAsync(&pin->st2, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HFMI_TRY(side_copies_end(ctx));
  HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));
  return solve_tail(Q_work, r, flags, BACK_IDENTITY_V, nullptr, &pin->st2, B != nullptr, who, host_d, U, nullptr);
}

static int check_sketch_args(const hfmi_block* Omega, int r, const hfmi_block* U, const char* who) {
  const int k = Omega->nvec;
  if (r < 1) HFMI_FAIL(HFMI_ERR_INVALID, "%s: rank must be positive", who);
  if (k < r) HFMI_FAIL(HFMI_ERR_INVALID, "%s: the sketch has %d vectors, need at least the rank %d", who, k, r);
  if (k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "%s: at most %d probe vectors (got %d)", who, SM_MAXK, k);
  if (U->N != Omega->N || U->nvec != r) HFMI_FAIL(HFMI_ERR_INVALID, "%s: U must be %lld x %d (got %lld x %d)", who, (long long)Omega->N, r,
                                                  (long long)U->N, U->nvec);
  return HFMI_OK;
}

static int single_pass_impl(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags, double* host_d,
                            hfmi_block* U) {
  const char* who = B ? "single_pass_g" : "single_pass";
  if (!A || !Omega || !host_d || !U) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = Omega->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(check_sketch_args(Omega, r, U, who));
  if (s < 1) HFMI_FAIL(HFMI_ERR_INVALID, "%s: s must be >= 1", who);
  const int64_t N = Omega->N;
  const int k = Omega->nvec;
  hfmi_block X0, X1, W2, W3;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_SOLVE_Q, N, k, &X0));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_SOLVE_Y, N, k, &X1));
  HFMI_TRY(ctx_tmp_view(ctx, TMP_SKETCH_Q, N, k, &W2));
  if (B) HFMI_TRY(ctx_tmp_view(ctx, TMP_SKETCH_BQ, N, k, &W3));
  power_iter it = {A, Binv, Omega, s, &X0, &X1, &W2, Omega, Omega};   // the last two iterates are kept, and Ybar = A X_{s-1} in W2
  HFMI_TRY(solve_power_iterations(it));
  hfmi_block* Yb = const_cast<hfmi_block*>(it.cur);
  if (B) return sketch_eig_core(it.prev, Yb, &W2, B, Yb, &W3, r, flags, host_d, U, who);   // Q in place of Y, B Q in W3
  return sketch_eig_core(it.prev, Yb, nullptr, nullptr, &W2, nullptr, r, flags, host_d, U, who);
}

extern "C" int hfmi_single_pass(hfmi_op* A, const hfmi_block* Omega, int r, int s, int flags, double* host_d, hfmi_block* U) {
  return single_pass_impl(A, nullptr, nullptr, Omega, r, s, flags, host_d, U);
}
extern "C" int hfmi_single_pass_g(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                                  double* host_d, hfmi_block* U) {
  if (!B || !Binv) HFMI_FAIL(HFMI_ERR_INVALID, "single_pass_g: B and Binv are required");
  return single_pass_impl(A, B, Binv, Omega, r, s, flags, host_d, U);
}

extern "C" int hfmi_sketch_eig(const hfmi_block* P, const hfmi_block* Y, const hfmi_block* Ybar, hfmi_op* B, int r, int flags,
                               double* host_d, hfmi_block* U) {
  if (!P || !Y || !host_d || !U) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (!Ybar != !B) HFMI_FAIL(HFMI_ERR_INVALID, "sketch_eig: Ybar and B go together (generalized problem) or are both absent");
  HFMI_TRY(check_same_shape(P, Y, "sketch_eig"));
  if (Ybar) HFMI_TRY(check_same_shape(P, Ybar, "sketch_eig"));
  hfmi_ctx* ctx = P->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(check_sketch_args(P, r, U, "sketch_eig"));
  const int64_t N = P->N;
  const int k = P->nvec;
  hfmi_block Qw, BQw;
  HFMI_TRY(ctx_tmp_view(ctx, TMP_SKETCH_Q, N, k, &Qw));
  if (B) HFMI_TRY(ctx_tmp_view(ctx, TMP_SKETCH_BQ, N, k, &BQw));
  return sketch_eig_core(P, Y, Ybar, B, &Qw, B ? &BQw : nullptr, r, flags, host_d, U, "sketch_eig");
}

// np.linalg.solve(W, Z) of the single-pass methods on the device, host in and host out (kernel tests): the one body of
// hfmi_small_solve and hfmi_test_lu_solve.  Upload, k_lu_solve launched as the single pass launches it (same slots; T into the
// eigensolver's slot when want_T), status words, then whatever the caller asks for -- host_X, host_LU (the factored working copy),
// host_T (the mp x mp region of the T slot, NaN filled before the launch).  The status is handed back, not judged.
static int small_copy_out(hfmi_ctx* ctx, int slot, int n, double* host) {
  std::vector<double> tmp((size_t)n * SM_LD);
  HFMI_TRY(read_back(ctx, sm_ptr(ctx, slot), tmp.size(), tmp.data()));
  for (int i = 0; i < n; ++i) memcpy(host + (size_t)i * n, tmp.data() + (size_t)i * SM_LD, (size_t)n * sizeof(double));
  return HFMI_OK;
}
static int lu_solve_host(hfmi_ctx* ctx, const double* host_W, const double* host_Z, int m, bool want_T, hfmi_status_words* st,
                         double* host_X, double* host_LU, double* host_T) {
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(upload_small(ctx, host_W, m, m, sm_ptr(ctx, SM_GRAM), SM_LD));
  HFMI_TRY(upload_small(ctx, host_Z, m, m, sm_ptr(ctx, SM_R), SM_LD));
  const int mp = (int)round_up(m, 16) < SM_LD ? (int)round_up(m, 16) : SM_LD;
  if (want_T) {
    const std::vector<double> nan_fill((size_t)mp * SM_LD, std::nan("7"));
    HFMI_TRY(upload_small(ctx, nan_fill.data(), mp, SM_LD, sm_ptr(ctx, SM_T), SM_LD));
  }
  HFMI_TRY(launch_lu_solve(ctx, m, SM_GRAM, SM_R, SM_TMP, SM_TMP2, want_T ? SM_T : -1));
  HFMI_TRY(read_status(ctx, st));
  if (host_X) HFMI_TRY(small_copy_out(ctx, SM_TMP2, m, host_X));
  if (host_LU) HFMI_TRY(small_copy_out(ctx, SM_TMP, m, host_LU));
  if (want_T && host_T) HFMI_TRY(small_copy_out(ctx, SM_T, mp, host_T));
  return HFMI_OK;
}

extern "C" int hfmi_small_solve(hfmi_ctx* ctx, const double* host_W, const double* host_Z, int m, double* host_X) {
  if (!ctx || !host_W || !host_Z || !host_X) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (m < 1 || m > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "small_solve: m=%d out of range [1,%d]", m, SM_MAXK);
  hfmi_status_words st;
  HFMI_TRY(lu_solve_host(ctx, host_W, host_Z, m, false, &st, nullptr, nullptr, nullptr));
  if (st.failed == 1) HFMI_FAIL(HFMI_ERR_NUMERIC, "small_solve (m=%d): non-finite input", m);
  if (st.failed == 3) HFMI_FAIL(HFMI_ERR_NUMERIC, "small_solve (m=%d): the elimination overflowed (non-finite pivot or solution)", m);
  if (st.failed) HFMI_FAIL(HFMI_ERR_NUMERIC, "small_solve (m=%d): the matrix is singular (min |pivot| %.2e, max |pivot| %.2e)", m,
                           st.min_pivot_ratio, st.gram_dev);
  return small_copy_out(ctx, SM_TMP2, m, host_X);
}

extern "C" int hfmi_test_lu_solve(hfmi_ctx* ctx, const double* host_W, const double* host_Z, int m, int want_T, double* host_X,
                                  double* host_LU, double* host_status, double* host_T) {
  if (!ctx || !host_W || !host_Z || !host_X || !host_LU || !host_status || (want_T && !host_T)) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (m < 1 || m > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "test_lu_solve: m=%d out of range [1,%d]", m, SM_MAXK);
  hfmi_status_words st;
  HFMI_TRY(lu_solve_host(ctx, host_W, host_Z, m, want_T != 0, &st, host_X, host_LU, host_T));
  host_status[0] = st.min_pivot_ratio;
  host_status[1] = st.gram_dev;
  host_status[2] = st.failed;
  return HFMI_OK;
}
