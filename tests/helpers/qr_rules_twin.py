"""The decisions of the Cholesky-QR loop as they stood BEFORE they were collected in hippyflow_amd/csrc/hfmi_qr_rules.h: the ``if``
chain of ``qr_chol`` (hfmi_qr.hip of commit 07d2224), the late verdict of ``double_pass_impl`` (hfmi_solve.hip of the same commit)
and the route condition, restated literally -- one comment per branch names the line it restates.  tests/test_qr_rules_cpu.py holds
``hfmi_qr_rules_predict`` / ``hfmi_qr_late_verdict_predict`` (include/hfmi.h) to this twin on every state."""

CHECKED, DEFERRED, TRUSTED = 0, 1, 2                                         # HFMI_QR_POLICY_*
TRUST_FIRST, TRUST_SECOND, READ_THEN_APPLY, APPLY_THEN_READ = 0, 1, 2, 3     # HFMI_QR_ISSUE_*
FAIL_NOT_PD, DONE, DONE_DEFERRED, AGAIN, FAIL_MAX_PASSES = 0, 1, 2, 3, 4     # HFMI_QR_NEXT_*
TERMINAL = (FAIL_NOT_PD, DONE, DONE_DEFERRED, FAIL_MAX_PASSES)

MAX_PASSES = 6                       # hfmi_qr.hip:45  chol_qr_rules::max_passes
EPS = 2.220446049250313e-16
SM_MAXK = 256


def parent_pass(policy, B, trust_first, passes, first_pass_clean, failed, shifted, gram_dev):
    """(how pass number ``passes`` is issued, what follows from its status words).  The three policies were two optional pointers:
    borth_qr passed neither, the Gram-form solve ``deferred``, and ``opt`` too when late checks were on (hfmi_solve.hip:283)."""
    deferred = policy in (DEFERRED, TRUSTED)
    opt = policy == TRUSTED
    if deferred and not B and passes == 0 and opt and trust_first:           # hfmi_qr.hip:106
        return TRUST_FIRST, AGAIN                                            # :113-120  slot 1, apply, ++passes, continue
    if deferred and not B and passes == 1 and opt and first_pass_clean:      # :124
        return TRUST_SECOND, DONE_DEFERRED                                   # :125-136  side copies, *deferred = true, return
    if deferred and not B and passes >= 1:                                   # :138
        how = READ_THEN_APPLY                                                # :141  read_status first
        if failed:                                                           # :142
            return how, FAIL_NOT_PD
        if not shifted and gram_dev < 1e-2:                                  # :143  (NaN < 1e-2 is false)
            return how, DONE_DEFERRED                                        # :144-146
    else:                                                                    # :149
        how = APPLY_THEN_READ                                                # :153-155  snapshot, apply, read
        if failed:                                                           # :156
            return how, FAIL_NOT_PD
    passes += 1                                                              # :159
    if passes >= 2 and not shifted and gram_dev < 1e-2:                      # :162
        return how, DONE
    if passes >= MAX_PASSES:                                                 # :163
        return how, FAIL_MAX_PASSES
    return how, AGAIN


def parent_first_pass_clean(how, shifted):
    """first_pass_clean after pass 0: set on trust (hfmi_qr.hip:118) or from the words that were read (:157)"""
    return how == TRUST_FIRST or not shifted


def parent_route_wide(k, qr_wide_min, policy):
    """hfmi_qr.hip:83  k > SM_MAXK || (k >= g_qr_wide_min && !deferred && !opt)"""
    return k > SM_MAXK or (k >= qr_wide_min and policy == CHECKED)


def parent_late_verdict(k, failed2, shifted2, gram_dev2, first_trusted, failed1, shifted1, norm, rdiag):
    """hfmi_solve.hip:330-333: True = the trusted passes hold"""
    ok = (not failed2) and (not shifted2) and gram_dev2 < 1e-2               # :330
    if first_trusted and (failed1 or shifted1):                              # :331
        ok = False
    for j in range(k):                                                       # :332
        if not ok:
            break
        if not (rdiag[j] > 100.0 * 2.220446049250313e-16 * norm[j]):         # :333  (the rule of check_dependent, hfmi_qr.hip:56)
            ok = False
    return ok
