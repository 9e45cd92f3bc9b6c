"""CPU suite: the rules of repeated Cholesky-QR (hippyflow_amd/csrc/hfmi_qr_rules.h) through ``hfmi_qr_rules_predict`` and
``hfmi_qr_late_verdict_predict`` -- the functions qr_chol, qr_chol_wide and the fused solve's tail themselves ask, without a device --
against tests/helpers/qr_rules_twin.py, the ``if`` chain they replaced, on every state."""
import ctypes as C
import itertools

import numpy as np
import pytest

from hippyflow_amd import _lib as L
from tests.helpers import qr_rules_twin as twin

POLICIES = (twin.CHECKED, twin.DEFERRED, twin.TRUSTED)
GRAM_DEVS = (0.0, 9.99e-3, 1e-2, 1.0, float("nan"))
_D = C.POINTER(C.c_double)


def predict(policy, B, knob, p, clean, failed, shifted, gram_dev, k=60, wide_min=257):
    words = (C.c_int * 3)()
    L.call("hfmi_qr_rules_predict", policy, int(B), int(knob), p, int(clean), int(failed), int(shifted), float(gram_dev), k, wide_min, words)
    return tuple(words)


def late_verdict(k, failed2, shifted2, gram_dev2, first_trusted, failed1, shifted1, norm, rdiag):
    stands = C.c_int(-1)
    norm, rdiag = np.ascontiguousarray(norm, dtype=np.float64), np.ascontiguousarray(rdiag, dtype=np.float64)
    L.call("hfmi_qr_late_verdict_predict", k, int(failed2), int(shifted2), float(gram_dev2), int(first_trusted), int(failed1), int(shifted1),
           norm.ctypes.data_as(_D), rdiag.ctypes.data_as(_D), C.byref(stands))
    assert stands.value in (0, 1)
    return bool(stands.value)


GRID = list(itertools.product(POLICIES, (0, 1), (0, 1), range(7), (0, 1), (0, 1), (0, 1), GRAM_DEVS))


def test_every_state_decides_as_the_parent_did():
    assert len(GRID) == 3360
    trusted_first = 0
    for state in GRID:
        policy, B, knob, p, clean, failed, shifted, gram_dev = state
        how, nxt, wide = predict(*state)
        assert (how, nxt) == twin.parent_pass(*state), state
        assert wide == 0
        if how == twin.TRUST_FIRST:                      # only ever: trusted policy, no B, pass 0, knob 1
            assert (policy, B, p, knob) == (twin.TRUSTED, 0, 0, 1), state
            trusted_first += 1
        if how == twin.TRUST_SECOND:
            assert (policy, B, p, clean) == (twin.TRUSTED, 0, 1, 1), state
        if how == twin.READ_THEN_APPLY:
            assert policy != twin.CHECKED and not B and p >= 1, state
        if B or policy == twin.CHECKED:                  # every pass of a checked call is issued the same way
            assert how == twin.APPLY_THEN_READ, state
        if nxt in (twin.DONE, twin.DONE_DEFERRED) and how in (twin.READ_THEN_APPLY, twin.APPLY_THEN_READ):
            assert not failed and not shifted and gram_dev < 1e-2 and p >= 1, state
    assert trusted_first == 2 * 2 * 2 * len(GRAM_DEVS)   # first_clean x failed x shifted x gram_dev: the words are not read


def test_a_nan_defect_reads_as_not_yet_orthonormal():
    for policy in POLICIES:
        for p in range(1, 5):
            how, nxt, _ = predict(policy, 0, 0, p, 0, 0, 0, float("nan"))
            assert nxt == twin.AGAIN, (policy, p)
        assert predict(policy, 0, 0, 5, 0, 0, 0, float("nan"))[1] == twin.FAIL_MAX_PASSES


STATUSES = [(1, 0, 1.0), (0, 1, 1.0), (0, 0, 9.99e-3), (0, 0, 1e-2), (0, 0, float("nan")), (0, 1, 0.0)]


def _walk(policy, B, knob, p, clean, path, out):
    """every sequence of status words a call can meet, followed until the rules stop it"""
    for st in STATUSES:
        how, nxt, _ = predict(policy, B, knob, p, clean, *st)
        if nxt in twin.TERMINAL:
            out.append((path + [st], how, nxt, p + 1))
            continue
        assert nxt == twin.AGAIN
        assert p + 1 < twin.MAX_PASSES, "pass %d of %r goes on" % (p + 1, path + [st])
        _walk(policy, B, knob, p + 1, twin.parent_first_pass_clean(how, st[1]) if p == 0 else clean, path + [st], out)
        if how in (twin.TRUST_FIRST, twin.TRUST_SECOND):
            break                                        # the words are not read: one branch


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("B", (0, 1))
@pytest.mark.parametrize("knob", (0, 1))
def test_every_scripted_sequence_ends_by_pass_six(policy, B, knob):
    ends = []
    _walk(policy, B, knob, 0, 0, [], ends)
    both_trusted = policy == twin.TRUSTED and not B and knob     # the call ends at pass two whatever the passes report
    assert ends and max(n for _, _, _, n in ends) == (2 if both_trusted else twin.MAX_PASSES)
    for path, how, nxt, n in ends:
        assert 1 <= n <= twin.MAX_PASSES
        if nxt == twin.FAIL_MAX_PASSES:
            assert n == twin.MAX_PASSES
        if nxt == twin.DONE:                             # a checked stop: at least two passes, the last one clean
            assert n >= 2 and path[-1][:2] == (0, 0) and path[-1][2] < 1e-2
        if nxt == twin.DONE_DEFERRED:
            assert policy != twin.CHECKED and not B and n >= 2
    kinds = {nxt for _, _, nxt, _ in ends}
    want = {twin.FAIL_NOT_PD, twin.FAIL_MAX_PASSES, twin.DONE if (B or policy == twin.CHECKED) else twin.DONE_DEFERRED}
    if both_trusted:
        want = {twin.DONE_DEFERRED}
    assert kinds == want


def test_the_route_is_narrow_for_every_fused_policy():
    fn, words = L.load().hfmi_qr_rules_predict, (C.c_int * 3)()      # 1.5 million calls: without the wrapper's bookkeeping

    def wide(policy, k, wide_min):
        assert fn(policy, 0, 1, 0, 0, 0, 0, 0.0, k, wide_min, words) == 0
        return words[2]

    for wide_min in range(17, 258):
        for policy in POLICIES:
            got = [wide(policy, k, wide_min) for k in range(1, 2049)]
            want = [int(k > 256 or (k >= wide_min and policy == twin.CHECKED)) for k in range(1, 2049)]
            assert got == want, (wide_min, policy)
            assert want == [int(twin.parent_route_wide(k, wide_min, policy)) for k in range(1, 2049)]


def test_late_verdict_at_the_dependent_column_threshold():
    k = 48
    rng = np.random.default_rng(7)
    norm = rng.uniform(0.5, 2.0, k)
    rdiag = norm * rng.uniform(1e-3, 1.0, k)
    assert late_verdict(k, 0, 0, 1e-6, 1, 0, 0, norm, rdiag)
    for j in (0, 17, k - 1):
        thr = 100.0 * twin.EPS * norm[j]                 # R_jj > 100 eps ||z_j||, strictly
        for value, stands in ((np.nextafter(thr, np.inf), True), (thr, False), (np.nextafter(thr, 0.0), False), (0.0, False), (float("nan"), False)):
            rd = rdiag.copy()
            rd[j] = value
            for first_trusted in (0, 1):
                args = (k, 0, 0, 1e-6, first_trusted, 0, 0, norm, rd)
                assert late_verdict(*args) == stands == twin.parent_late_verdict(*args), (j, value)
    # a column beyond k is not looked at
    assert late_verdict(k - 1, 0, 0, 1e-6, 0, 0, 0, norm, np.concatenate([rdiag[:k - 1], [0.0]]))


def test_late_verdict_over_the_status_words():
    k = 5
    norm, rdiag = np.ones(k), np.full(k, 0.5)
    for failed2, shifted2, gram_dev2, first_trusted, failed1, shifted1 in itertools.product((0, 1), (0, 1), GRAM_DEVS, (0, 1), (0, 1), (0, 1)):
        args = (k, failed2, shifted2, gram_dev2, first_trusted, failed1, shifted1, norm, rdiag)
        want = not failed2 and not shifted2 and gram_dev2 < 1e-2 and not (first_trusted and (failed1 or shifted1))
        assert late_verdict(*args) == want == twin.parent_late_verdict(*args), args


def test_bad_arguments_are_refused():
    words = (C.c_int * 3)()
    for bad in ((3, 0, 0, 0, 0, 0, 0, 0.0, 60, 257), (-1, 0, 0, 0, 0, 0, 0, 0.0, 60, 257), (0, 0, 0, -1, 0, 0, 0, 0.0, 60, 257),
                (0, 0, 0, 0, 0, 0, 0, 0.0, 0, 257)):
        with pytest.raises(L.HfmiError):
            L.call("hfmi_qr_rules_predict", *bad, words)
    with pytest.raises(L.HfmiError):
        late_verdict(257, 0, 0, 0.0, 0, 0, 0, np.ones(257), np.ones(257))
