// The rules of repeated (shifted) Cholesky-QR, host only: no HIP, no context.  qr_chol / qr_chol_wide (hfmi_qr.hip) ask them per pass,
// launch what they say and hand the pass's status words back; the fused solve (hfmi_solve.hip) asks for the late verdict.
// hfmi_qr_rules_predict / hfmi_qr_late_verdict_predict (include/hfmi.h) evaluate them without a device; tests/test_qr_rules_cpu.py
// sweeps every state.
#pragma once
#include <stdint.h>

#include "hfmi.h"

// What the caller lets the loop leave undone.  One policy per call, fixed before the first pass:
//   checked  every pass's status words are read; Q is orthonormal on return (hfmi_borth_qr, the literal solves)
//   deferred the last pass (input orthonormal to 1e-2, no shift) is not applied: R^-1 stays in SM_RINV for the caller to fold in
//   trusted  deferred, and no host round trip: the status words go to pinned memory and the caller judges them late
// With B every policy runs checked passes (B Q is needed after every pass), but the route stays the one the caller's policy names.
enum qr_policy { QR_CHECKED = HFMI_QR_POLICY_CHECKED, QR_DEFERRED = HFMI_QR_POLICY_DEFERRED, QR_TRUSTED = HFMI_QR_POLICY_TRUSTED };
enum qr_issue {
  QR_TRUST_FIRST = HFMI_QR_ISSUE_TRUST_FIRST,          // first pass on trust: status words to slot 1, apply R^-1, no read
  QR_TRUST_SECOND = HFMI_QR_ISSUE_TRUST_SECOND,        // second pass on trust: three side copies, stop deferred; the checks are the caller's
  QR_READ_THEN_APPLY = HFMI_QR_ISSUE_READ_THEN_APPLY,  // candidate last pass: read the words first, apply R^-1 only if another pass follows
  QR_APPLY_THEN_READ = HFMI_QR_ISSUE_APPLY_THEN_READ   // snapshot the words, apply R^-1, then read: the round trip overlaps the contraction
};
enum qr_next {
  QR_FAIL_NOT_PD = HFMI_QR_NEXT_FAIL_NOT_PD,
  QR_DONE = HFMI_QR_NEXT_DONE,
  QR_DONE_DEFERRED = HFMI_QR_NEXT_DONE_DEFERRED,
  QR_AGAIN = HFMI_QR_NEXT_AGAIN,
  QR_FAIL_MAX_PASSES = HFMI_QR_NEXT_FAIL_MAX_PASSES
};
struct qr_status { int failed, shifted; double gram_dev; };   // of hfmi_status_words: what the rules read

// Thresholds, each named once.  The breakdown tolerance on pivot / (original diagonal), 64 k eps, lives in the factorisation
// kernels and is what pivot_tol = 0 selects: only pivots that are round-off noise trigger the shifted factorisation.  A pass with
// small but genuine pivots leaves a defect ~ eps / min pivot ratio, which the next pass measures (gram_dev) and removes -- a more
// cautious threshold (100 k sqrt(N) u) cost config 3 a whole extra pass (shifted first pass, cond(Q1) ~ 260) for no accuracy.
constexpr double QR_EPS = 2.220446049250313e-16;
constexpr double QR_DONE_DEFECT = 1e-2;            // input defect below which an unshifted pass leaves Q orthonormal to round-off
constexpr double QR_DEPENDENT_DROP = 100.0 * QR_EPS;
struct chol_qr_rules {
  double shift_rel;                // diagonal shift of a restarted factorisation, relative to trace(G): 11 (N k + k (k + 1)) u
  double pivot_tol = 0.0;          // the factorisations' default: 64 k eps
  int max_passes = 6;
  chol_qr_rules(int64_t N, int k) : shift_rel(11.0 * ((double)N * k + (double)k * (k + 1)) * (QR_EPS / 2)) {}
};

// narrow (fixed small-matrix arena, k <= 256) or wide arena; decided once per call.  The wide loop is always checked, so the fused
// solves' deferred / trusted calls stay narrow whatever the tuning key "qr_wide_min" says.
inline bool qr_route_wide(int k, int wide_min, qr_policy policy) { return k > 256 || (k >= wide_min && policy == QR_CHECKED); }

// how pass number `pass` (0-based) is issued; first_clean: pass 0 was trusted or reported no shift
inline qr_issue qr_issue_checked() { return QR_APPLY_THEN_READ; }
inline qr_issue qr_issue_deferred(int pass) { return pass >= 1 ? QR_READ_THEN_APPLY : QR_APPLY_THEN_READ; }
inline qr_issue qr_issue_trusted(int pass, bool trust_first, bool first_clean) {
  if (pass == 0 && trust_first) return QR_TRUST_FIRST;
  if (pass == 1 && first_clean) return QR_TRUST_SECOND;
  return qr_issue_deferred(pass);                    // a shifted first pass: the rest of the call goes by the deferred rules
}
inline qr_issue qr_issue_of(qr_policy policy, bool has_B, bool trust_first, int pass, bool first_clean) {
  if (has_B || policy == QR_CHECKED) return qr_issue_checked();
  return policy == QR_TRUSTED ? qr_issue_trusted(pass, trust_first, first_clean) : qr_issue_deferred(pass);
}
inline bool qr_first_clean(qr_issue how, const qr_status& st) { return how == QR_TRUST_FIRST || !st.shifted; }

// what follows from the status words of pass number `pass`, issued as `how` (the trusted issues carry no words: st is not read).
// The input of the pass had orthonormality defect gram_dev (column-scaled): if that was small and no shift was needed, the output
// is orthonormal to round-off.  A NaN defect reads as "not yet orthonormal".
inline qr_next qr_verdict(qr_issue how, int pass, const qr_status& st, int max_passes) {
  if (how == QR_TRUST_FIRST) return QR_AGAIN;
  if (how == QR_TRUST_SECOND) return QR_DONE_DEFERRED;
  if (st.failed) return QR_FAIL_NOT_PD;
  if (pass >= 1 && !st.shifted && st.gram_dev < QR_DONE_DEFECT) return how == QR_READ_THEN_APPLY ? QR_DONE_DEFERRED : QR_DONE;
  return pass + 1 >= max_passes ? QR_FAIL_MAX_PASSES : QR_AGAIN;
}

// The reference's MGS zeroes a column whose norm drops below 10 eps of its pre-sweep norm (numerically dependent); Cholesky-QR
// would instead normalise round-off noise.  R_jj / ||z_j|| is that drop: such blocks go to the Gram-Schmidt route, which
// reproduces the reference's behaviour.  norm: ||z_j|| of the original column, rdiag: diag(Rtot)_j.
inline bool qr_column_independent(double rdiag, double norm) { return rdiag > QR_DEPENDENT_DROP * norm; }
// first dependent column, or -1
inline int qr_first_dependent(const double* norm, const double* rdiag, int k) {
  for (int j = 0; j < k; ++j)
    if (!qr_column_independent(rdiag[j], norm[j])) return j;
  return -1;
}
// The late verdict on a call whose second pass was taken on trust: true = the result stands, false = repeat on the checked path
// (which decides between the Gram-Schmidt fall-back and an error).  st1: the first pass's words when that pass was trusted too.
inline bool qr_late_verdict(const qr_status& st2, const qr_status* st1, const double* norm, const double* rdiag, int k) {
  if (st2.failed || st2.shifted || !(st2.gram_dev < QR_DONE_DEFECT)) return false;
  if (st1 && (st1->failed || st1->shifted)) return false;
  return qr_first_dependent(norm, rdiag, k) < 0;
}
