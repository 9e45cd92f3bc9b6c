// B-orthogonal thin QR of libhfmi.so (include/hfmi.h): repeated (shifted) Cholesky-QR (up to 256 vectors in the fixed small-matrix
// arena, up to 2048 in the wide one), the reference's Gram-Schmidt rule and the dispatcher between them.  Host side only; kernels
// live in hfmi_gemm.hip / hfmi_gemm_nn.hip / hfmi_chol_col.hip / hfmi_chol.hip / hfmi_chol_wide.hip.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "hfmi_internal.h"

// Y = A S with S upper triangular (R^-1 of a Cholesky-QR pass: every factorisation kernel writes its strict lower triangle as
// zeros): the hint lets the resident-S kernel skip the structurally zero column tiles; any other route ignores it
int launch_nn_upper(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* S, int ld, int r, double* Y, int64_t ldy,
                    int64_t N) {
  ctx->nn_upper_hint = true;
  const int s = launch_tsgemm_nn(ctx, A, lda, m, S, ld, r, 1.0, 0.0, Y, ldy, N);
  ctx->nn_upper_hint = false;
  return s;
}

// ------------------------------------------------------------------ QR
// Split read-back: `begin` snapshots the status words at the current point of the main stream (event + copy on the
// auxiliary stream), `finish` waits for that copy only -- kernels queued on the main stream in between keep running
// while the host looks at the words and decides what to launch next.
static int read_status_begin(hfmi_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_status, 0));
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  return HFMI_OK;
}
static int read_status_finish(hfmi_ctx* ctx, hfmi_status_words* out) {
  HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
  *out = *ctx->status_host;
  print_status_dbg(out);
  return HFMI_OK;
}
// aux_dev: [0, k): original column norms; [ld, ld + k): diag(Rtot)
static int check_dependent(hfmi_ctx* ctx, const double* aux_dev, int ld, int k) {
  std::vector<double> aux((size_t)ld + k);
  HFMI_TRY(read_back(ctx, aux_dev, (size_t)ld + k, aux.data()));
  const int j = qr_first_dependent(aux.data(), aux.data() + ld, k);
  if (j >= 0)
    HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: vector %d is numerically dependent on its predecessors (R_jj/||z_j|| = %.2e)", j,
              aux[j] > 0 ? aux[ld + j] / aux[j] : 0.0);
  return HFMI_OK;
}
// host_R (k x k row-major) <- the k x k matrix at dev (row-major, ld)
static int read_r(hfmi_ctx* ctx, const double* dev, int ld, int k, double* host_R) {
  std::vector<double> tmp((size_t)k * ld);
  HFMI_TRY(read_back(ctx, dev, (size_t)k * ld, tmp.data()));
  for (int i = 0; i < k; ++i) memcpy(host_R + (size_t)i * k, tmp.data() + (size_t)i * ld, (size_t)k * sizeof(double));
  return HFMI_OK;
}
static qr_status status_triple(const hfmi_status_words& w) { return {w.failed, w.shifted, w.gram_dev}; }
// the two failing verdicts of pass number `pass` (0-based) as errors
static int qr_fail(qr_next next, int pass, double gram_dev) {
  if (next == QR_FAIL_NOT_PD) HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: Gram matrix not positive definite even after shifting (pass %d)", pass + 1);
  HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: no convergence in %d Cholesky-QR passes (defect %.2e)", pass + 1, gram_dev);
}

int ctx_late_pinned(hfmi_ctx* ctx, qr_late_buffer** out) {
  if (!ctx->late_pinned) OWN_TRY(ctx->late_pinned.alloc(sizeof(qr_late_buffer)));
  *out = (qr_late_buffer*)ctx->late_pinned.get();
  return HFMI_OK;
}
// A second pass on trust: its status words (and those of a trusted first pass) and the R_jj / ||z_j|| table leave for pinned memory
// in stream order; the eigensolver (next writer of the status words) waits for ev_side.  The caller verifies them (qr_late_stands)
// after the synchronisation it needs anyway for the eigenvalues and repeats the solve on the checked path if the trust was misplaced.
// (Two host round trips of ~60 us each per solve: 1.4 % of the 64-sample shard step.)
static int late_copies(hfmi_ctx* ctx, qr_late_buffer* late, int k, bool first_trusted) {
  HFMI_TRY(side_copies_begin(ctx));
  if (first_trusted)
    HIP_TRY(hipMemcpyAsync(&late->st1, ctx->status_dev + 1, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HIP_TRY(hipMemcpyAsync(&late->st2, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HIP_TRY(hipMemcpyAsync(late->aux, sm_ptr(ctx, SM_AUX), ((size_t)SM_LD + k) * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream));
  return side_copies_end(ctx);
}
bool qr_late_stands(const qr_late_buffer* late, int k, bool first_trusted) {
  const qr_status st1 = status_triple(late->st1);
  return qr_late_verdict(status_triple(late->st2), first_trusted ? &st1 : nullptr, late->aux, late->aux + SM_LD, k);
}

int op_apply_panels(hfmi_op* op, const hfmi_block* X, hfmi_block* Y) {
  if (X->nvec <= SM_MAXK) return hfmi_op_apply(op, X, Y, 0);
  if (Y->nvec != X->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "operator application: the blocks hold %d and %d vectors", X->nvec, Y->nvec);
  for (int c0 = 0; c0 < X->nvec; c0 += SM_MAXK) {
    hfmi_block xv = *X, yv = *Y;
    xv.p = X->p + (int64_t)c0 * X->ld;
    yv.p = Y->p + (int64_t)c0 * Y->ld;
    xv.nvec = yv.nvec = std::min(SM_MAXK, X->nvec - c0);
    xv.owner = yv.owner = false;
    HFMI_TRY(hfmi_op_apply(op, &xv, &yv, 0));
  }
  return HFMI_OK;
}

// The checked loop for 256 < k <= 2048 columns (and, for tests, from the tuning key "qr_wide_min" on): Gram matrix, factors and
// status words in the wide arena (hfmi_chol_wide.hip), one host round trip per pass (inside launch_chol_wide: nothing is applied
// after a failed factorisation), and Q <- Q R^-1 OUT of place (a panel of the product reads columns of Q that an earlier panel would
// already have overwritten): the passes alternate between Q and a cached temporary, and an odd number of passes ends with a copy
// back.  Rtot is always the exact product of the passes' factors.
static int qr_chol_wide(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, qr_result* res) {
  hfmi_ctx* ctx = Q->ctx;
  const int64_t N = Q->N;
  const int k = Q->nvec;
  HFMI_TRY(ctx_wide(ctx, k));
  const int ld = (int)round_up(k, 32);
  hfmi_block* BZ = BQ;
  hfmi_block bz_view, pong;
  if (B && !BQ) {
    HFMI_TRY(ctx_tmp_view(ctx, TMP_QR_BZ, N, k, &bz_view));
    BZ = &bz_view;
  }
  HFMI_TRY(ctx_tmp_view(ctx, TMP_QR_WIDE, N, k, &pong));
  const chol_qr_rules rules(N, k);
  hfmi_block* cur = Q;
  hfmi_block* nxt = &pong;
  for (int pass = 0;; ++pass) {
    const hfmi_block* right = cur;
    if (B) {
      HFMI_TRY(op_apply_panels(B, cur, BZ));
      right = BZ;
    }
    HFMI_TRY(launch_tsgemm_tn(ctx, cur->p, cur->ld, k, right->p, right->ld, k, N, 1.0, 0.0, wa_ptr(ctx, WA_GRAM), ld, 1, 0));
    hfmi_status_words w;
    HFMI_TRY(launch_chol_wide(ctx, k, pass == 0 ? 1 : 2, rules.shift_rel, rules.pivot_tol, &w));
    const qr_next next = qr_verdict(qr_issue_checked(), pass, status_triple(w), rules.max_passes);
    if (next == QR_FAIL_NOT_PD) return qr_fail(next, pass, w.gram_dev);
    // Q R^-1 in column panels of 256 issued here, not inside launch_tsgemm_nn: columns r0 .. r0 + rp - 1 of the upper triangular R^-1
    // are zero below row r0 + rp, so the panel's reduction stops there (half the work, the same bits), and the upper-triangular
    // hint of launch_nn_upper -- which takes the small matrix's column 0 for the diagonal -- goes to the first panel only
    for (int r0 = 0; r0 < k; r0 += SM_MAXK) {
      const int rp = std::min(SM_MAXK, k - r0);
      const double* S = wa_ptr(ctx, WA_RINV) + r0;
      double* Yp = nxt->p + (int64_t)r0 * nxt->ld;
      if (r0 == 0) HFMI_TRY(launch_nn_upper(ctx, cur->p, cur->ld, rp, S, ld, rp, Yp, nxt->ld, N));
      else HFMI_TRY(launch_tsgemm_nn(ctx, cur->p, cur->ld, r0 + rp, S, ld, rp, 1.0, 0.0, Yp, nxt->ld, N));
    }
    std::swap(cur, nxt);
    res->passes = pass + 1;
    if (next == QR_FAIL_MAX_PASSES) return qr_fail(next, pass, w.gram_dev);
    if (next == QR_DONE) break;
  }
  if (cur != Q) HFMI_TRY(launch_copy(ctx, Q->p, Q->ld, cur->p, cur->ld, N, k));
  HFMI_TRY(check_dependent(ctx, wa_aux(ctx), ld, k));
  if (B && BQ) HFMI_TRY(op_apply_panels(B, Q, BQ));
  return HFMI_OK;
}

static bool qr_trust_first_knob() {    // tuning key "qr_trust_first", else HFMI_QR_TRUST_FIRST, else on
  if (g_qr_trust_first < 0) {
    const char* e = getenv("HFMI_QR_TRUST_FIRST");
    g_qr_trust_first = (e && e[0] == '0') ? 0 : 1;
  }
  return g_qr_trust_first != 0;
}
// Repeated Cholesky-QR of Q in place, in the fixed arena unless the route says wide.  Every pass: Gram matrix, factorisation (always
// tracking Rtot = R_p ... R_1: its diagonal exposes dependent columns), then what the rules say about issuing it and about its words.
int qr_chol(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, bool want_r, qr_policy policy, qr_result* res) {
  hfmi_ctx* ctx = Q->ctx;
  const int64_t N = Q->N;
  const int k = Q->nvec;
  *res = qr_result();
  if (k > HFMI_WIDE_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: at most %d vectors (got %d)", HFMI_WIDE_MAXK, k);
  res->wide = qr_route_wide(k, g_qr_wide_min, policy);
  if (res->wide) return qr_chol_wide(Q, B, BQ, res);
  hfmi_block* BZ = BQ;
  hfmi_block bz_view;
  if (B && !BQ) {
    HFMI_TRY(ctx_tmp_view(ctx, TMP_QR_BZ, N, k, &bz_view));
    BZ = &bz_view;
  }
  const chol_qr_rules rules(N, k);
  const bool trust_first = qr_trust_first_knob();
  qr_late_buffer* late = nullptr;
  if (policy == QR_TRUSTED && !B) HFMI_TRY(ctx_late_pinned(ctx, &late));
  const auto apply_rinv = [&] { return launch_nn_upper(ctx, Q->p, Q->ld, k, sm_ptr(ctx, SM_RINV), SM_LD, k, Q->p, Q->ld, N); };
  bool first_clean = false;
  for (int pass = 0;; ++pass) {
    const hfmi_block* right = Q;
    if (B) {
      HFMI_TRY(hfmi_op_apply(B, Q, BZ, 0));
      right = BZ;
    }
    HFMI_TRY(launch_tsgemm_tn(ctx, Q->p, Q->ld, k, right->p, right->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_GRAM), SM_LD, 1, 0));
    const qr_issue how = qr_issue_of(policy, B != nullptr, trust_first, pass, first_clean);
    hfmi_status_words* const keep = ctx->status_dev;
    if (how == QR_TRUST_FIRST) ctx->status_dev = keep + 1;   // its own slot: nothing overwrites the words before they are read
    const int cs = launch_chol_inv(ctx, k, SM_GRAM, SM_R, SM_RINV, SM_RTOT, pass == 0 ? 1 : 2, want_r ? 1 : 0, rules.shift_rel, rules.pivot_tol);
    ctx->status_dev = keep;
    HFMI_TRY(cs);
    hfmi_status_words w = {};
    switch (how) {
      case QR_TRUST_FIRST:       // no host round trip interrupts the solve: the host runs ahead of the device from here to the final
        HFMI_TRY(apply_rinv());  // synchronisation, so the small kernels of the tail are queued back to back
        res->first_trusted = true;
        break;
      case QR_TRUST_SECOND:
        HFMI_TRY(late_copies(ctx, late, k, res->first_trusted));
        res->late = true;
        break;
      case QR_READ_THEN_APPLY:   // the read-back is not hidden here; R^-1 is applied below, if another pass follows
        HFMI_TRY(read_status(ctx, &w));
        break;
      case QR_APPLY_THEN_READ:   // if the factorisation failed, R^-1 was never written by this pass and Q is about to be discarded
        HFMI_TRY(read_status_begin(ctx));   // anyway (the callers restore / recompute the block on HFMI_ERR_NUMERIC)
        HFMI_TRY(apply_rinv());
        HFMI_TRY(read_status_finish(ctx, &w));
        break;
    }
    const qr_status st = status_triple(w);
    const qr_next next = qr_verdict(how, pass, st, rules.max_passes);
    if (how == QR_READ_THEN_APPLY && (next == QR_AGAIN || next == QR_FAIL_MAX_PASSES)) HFMI_TRY(apply_rinv());
    if (pass == 0) first_clean = qr_first_clean(how, st);
    res->passes = pass + 1;
    if (next == QR_FAIL_NOT_PD || next == QR_FAIL_MAX_PASSES) return qr_fail(next, pass, st.gram_dev);
    res->deferred = next == QR_DONE_DEFERRED;
    if (next != QR_AGAIN) break;
  }
  if (res->late) return HFMI_OK;                         // the checks below are the caller's, after its own synchronisation
  HFMI_TRY(check_dependent(ctx, sm_ptr(ctx, SM_AUX), SM_LD, k));
  if (B && BQ) HFMI_TRY(hfmi_op_apply(B, Q, BQ, 0));
  return HFMI_OK;
}

// Column-by-column Gram-Schmidt with the reference's re-orthogonalisation rule (hippylib
// MultiVector._mgs_stable / _mgs_reortho as restated in oracle/hippylib_restated.py): each sweep projects
// column j against all previous columns at once (classical GS per sweep; with the "twice is enough"
// repetition this is as stable as the modified variant) and repeats while 10 eps t < ||q|| < t/10.
static int qr_mgs(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* R_host /* k*k or null */, int* passes_out) {
  hfmi_ctx* ctx = Q->ctx;
  const int64_t N = Q->N;
  const int k = Q->nvec;
  const double eps = 2.220446049250313e-16;
  hfmi_block* BZ = BQ;
  hfmi_block bz_view;
  if (B && !BQ) {
    HFMI_TRY(ctx_tmp_view(ctx, TMP_QR_BZ, N, k, &bz_view));
    BZ = &bz_view;
  }
  std::vector<double> R((size_t)k * k, 0.0), s(k);
  void* dv = nullptr;
  // its own slot: hfmi_op_apply(B, ...) inside the column loop may regrow WS_G (Gram-form / composed / PCG operators)
  HFMI_TRY(ctx_ws(ctx, WS_MGS, (size_t)(k + 16) * 16 * sizeof(double), &dv));
  double* dsmall = (double*)dv;  // device scratch: coefficient column (ld 16) / scalars
  int total_sweeps = 0;
  for (int j = 0; j < k; ++j) {
    hfmi_block qj = *Q;
    qj.p = Q->p + (int64_t)j * Q->ld;
    qj.nvec = 1;
    hfmi_block bqj = qj;
    if (B) {
      bqj = *BZ;
      bqj.p = BZ->p + (int64_t)j * BZ->ld;
      bqj.nvec = 1;
      HFMI_TRY(hfmi_op_apply(B, &qj, &bqj, 0));
    }
    double t2 = 0.0;
    HFMI_TRY(launch_col_dots(ctx, bqj.p, bqj.ld, qj.p, qj.ld, N, 1, dsmall));
    HFMI_TRY(read_back(ctx, dsmall, 1, &t2));
    double t = sqrt(std::max(t2, 0.0));
    double tt = t;
    bool again = true;
    while (again) {
      ++total_sweeps;
      if (j > 0) {
        // s = (B Q_prev)^T q_j
        const double* left = B ? BZ->p : Q->p;
        const int64_t ldl = B ? BZ->ld : Q->ld;
        HFMI_TRY(launch_tsgemm_tn(ctx, left, ldl, j, qj.p, qj.ld, 1, N, 1.0, 0.0, dsmall, 16, 1, 0));
        std::vector<double> tmp((size_t)j * 16);
        HFMI_TRY(read_back(ctx, dsmall, (size_t)j * 16, tmp.data()));
        for (int i = 0; i < j; ++i) {
          s[i] = tmp[(size_t)i * 16];
          R[(size_t)i * k + j] += s[i];
        }
        // q_j -= Q_prev s   (the device copy of s already sits in dsmall with ld 16)
        HFMI_TRY(launch_tsgemm_nn(ctx, Q->p, Q->ld, j, dsmall, 16, 1, -1.0, 1.0, qj.p, qj.ld, N));
      }
      if (B) HFMI_TRY(hfmi_op_apply(B, &qj, &bqj, 0));
      double tt2 = 0.0;
      HFMI_TRY(launch_col_dots(ctx, bqj.p, bqj.ld, qj.p, qj.ld, N, 1, dsmall));
      HFMI_TRY(read_back(ctx, dsmall, 1, &tt2));
      tt = sqrt(std::max(tt2, 0.0));
      if (tt > t * 10.0 * eps && tt < t / 10.0) {
        again = true;
        t = tt;
      } else {
        again = false;
        if (tt < 10.0 * eps * t) tt = 0.0;
      }
    }
    R[(size_t)j * k + j] = tt;
    const double inv = (fabs(tt * eps) > 0.0) ? 1.0 / tt : 0.0;
    HFMI_TRY(launch_scale(ctx, qj.p, qj.ld, N, 1, inv));
    if (B) HFMI_TRY(launch_scale(ctx, bqj.p, bqj.ld, N, 1, inv));
  }
  if (R_host) memcpy(R_host, R.data(), (size_t)k * k * sizeof(double));
  if (passes_out) *passes_out = total_sweeps;
  return HFMI_OK;
}

// want_r: exact triangular factors in every Cholesky pass.  Without it a pass whose input is already orthonormal to ~1e-7
// takes the kernel's first-order inverse square root, which left a 74-column single-pass sketch orthonormal to only ~1e-10.
int borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, bool want_r, int method, int* passes) {
  if (!Q) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  if (BQ) HFMI_TRY(check_same_shape(Q, BQ, "borth_qr"));
  if (BQ && !B) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: BQ requested without B");
  hfmi_ctx* ctx = Q->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int k = Q->nvec;
  if (method == HFMI_QR_MGS) return qr_mgs(Q, B, BQ, host_R, passes);
  if (method != HFMI_QR_CHOL && method != HFMI_QR_AUTO) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: unknown method %d", method);
  if (k > HFMI_WIDE_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: at most %d vectors (got %d)", HFMI_WIDE_MAXK, k);
  hfmi_block save;
  if (method == HFMI_QR_AUTO) {  // keep the input so that a breakdown can fall back to Gram-Schmidt
    HFMI_TRY(ctx_tmp_view(ctx, TMP_QR_SAVE, Q->N, k, &save));
    HFMI_TRY(launch_copy(ctx, save.p, save.ld, Q->p, Q->ld, Q->N, k));
  }
  qr_result res;
  const int s = qr_chol(Q, B, BQ, want_r, QR_CHECKED, &res);
  if (s == HFMI_ERR_NUMERIC && method == HFMI_QR_AUTO) {
    HFMI_TRY(launch_copy(ctx, Q->p, Q->ld, save.p, save.ld, Q->N, k));
    return qr_mgs(Q, B, BQ, host_R, passes);
  }
  if (s != HFMI_OK) return s;
  if (passes) *passes = res.passes;
  if (!host_R) return HFMI_OK;
  if (res.wide) return read_r(ctx, wa_ptr(ctx, WA_RTOT), (int)round_up(k, 32), k, host_R);
  return read_r(ctx, sm_ptr(ctx, SM_RTOT), SM_LD, k, host_R);
}
extern "C" int hfmi_borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, int method, int* passes) {
  return borth_qr(Q, B, BQ, host_R, host_R != nullptr, method, passes);
}

// the rules as the loops above ask them, for given values (hfmi_qr_rules.h); no context and no device
extern "C" int hfmi_qr_rules_predict(int policy, int has_B, int trust_first, int pass, int first_clean, int failed, int shifted, double gram_dev,
                                     int k, int qr_wide_min, int* words) {
  if (!words) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (policy < QR_CHECKED || policy > QR_TRUSTED || pass < 0 || k < 1) HFMI_FAIL(HFMI_ERR_INVALID, "qr_rules_predict: bad argument");
  const qr_issue how = qr_issue_of((qr_policy)policy, has_B != 0, trust_first != 0, pass, first_clean != 0);
  words[0] = how;
  words[1] = qr_verdict(how, pass, qr_status{failed, shifted, gram_dev}, chol_qr_rules(1, k).max_passes);
  words[2] = qr_route_wide(k, qr_wide_min, (qr_policy)policy);
  return HFMI_OK;
}
extern "C" int hfmi_qr_late_verdict_predict(int k, int failed2, int shifted2, double gram_dev2, int first_trusted, int failed1, int shifted1,
                                            const double* norm, const double* rdiag, int* stands) {
  if (!norm || !rdiag || !stands) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "qr_late_verdict_predict: k=%d out of range [1,%d]", k, SM_MAXK);
  const qr_status st1 = {failed1, shifted1, 0.0};
  *stands = qr_late_verdict(qr_status{failed2, shifted2, gram_dev2}, first_trusted ? &st1 : nullptr, norm, rdiag, k);
  return HFMI_OK;
}
