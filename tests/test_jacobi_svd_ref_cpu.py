"""CPU checks of the one-sided Jacobi reference (tests/helpers/jacobi_svd_ref.py) that the GPU tests of k_jacobi_svd
measure against: the longdouble run against a 50-digit SVD, the fp64 restatement against the longdouble run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import jacobi_svd_ref as jr  # noqa: E402

EPS = np.finfo(np.float64).eps
EPS_LD = float(np.finfo(np.longdouble).eps)


def _cases(k):
    rng = np.random.default_rng(100 + k)
    yield "gaussian", rng.standard_normal((k, k)), k
    for fam, (gen, kmin, rank) in jr.ACCURACY_FAMILIES.items():
        if k >= kmin:
            yield fam, gen(k, rng), rank(k)


@pytest.mark.parametrize("k", [1, 2, 3, 8, 17, 24])
def test_longdouble_reference_against_50_digits(k):
    """The reference's relative error in every non-zero singular value stays under k eps64 / 16: under 1 % of the
    smallest tolerance a GPU test derives from it (8 k eps64).  Its vectors are orthonormal and reconstruct R to a
    small multiple of its own eps."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    for name, R, rank in _cases(k):
        U, sig, V, sweeps = jr.jacobi_svd(R, np.longdouble)
        S = mpmath.svd_r(mpmath.matrix(R.tolist()), compute_uv=False)
        S = sorted((S[i] for i in range(k)), reverse=True)
        worst = 0.0
        for i in range(rank):
            hi = float(sig[i])
            got = mpmath.mpf(hi) + mpmath.mpf(float(sig[i] - np.longdouble(hi)))      # the 64-bit value, exactly
            worst = max(worst, float(abs(got - S[i]) / S[i]))
        print("k=%d %-12s sweeps %2d  rel err vs 50 digits %.2e  (allowed %.2e)" % (k, name, sweeps, worst, k * EPS / 16))
        assert worst <= k * EPS / 16, name
        assert np.all(sig[rank:] <= k * EPS_LD * sig[0]), name
        assert np.all(np.diff(sig) <= 0) and sweeps < jr.MAX_SWEEPS, name
        lead = U[:, sig > 0]                 # a singular value that is exactly zero has a zero column of U
        assert np.all(U[:, sig == 0] == 0), name
        assert np.abs(lead.T @ lead - np.eye(lead.shape[1])).max() <= 8 * k * EPS_LD, name
        assert np.abs(V.T @ V - np.eye(k)).max() <= 8 * k * EPS_LD, name
        assert np.abs((U * sig) @ V.T - R).max() <= 8 * k * EPS_LD * max(float(sig[0]), 1e-300), name
        if name == "zero-columns":
            assert np.all(sig[rank:] == 0) and np.all(U[:, rank:] == 0)


def test_restatement_tracks_the_reference():
    """fp64 against longdouble at k = 24: the errors the GPU tolerances are eight times of are of the size the table in
    the helper records (a few 1e-15 one-sided, about 1e-13 two-sided), far above the reference's own."""
    for fam, hi in (("triangular", 1e-13), ("two-sided", 2e-12), ("duplicated", 1e-13), ("zero-columns", 1e-13)):
        gen, _, rank = jr.ACCURACY_FAMILIES[fam]
        R = gen(24, np.random.default_rng(24))
        ref = jr.jacobi_svd(R, np.longdouble)[1]
        err = jr.restatement_error(R, rank(24), ref)
        print("%-12s restatement rel err %.2e, tolerance %.2e" % (fam, err, jr.accuracy_tolerance(R, rank(24), ref)))
        assert err <= hi
        assert jr.accuracy_tolerance(R, rank(24), ref) == max(8 * err, 8 * 24 * EPS)


def test_separate_square_roots_survive_extreme_scales():
    """sqrt(al) * sqrt(be), not sqrt(al * be): the same vectors and exactly scaled singular values at 2^+-500"""
    R = np.random.default_rng(5).standard_normal((24, 24))
    U0, s0, V0, _ = jr.jacobi_svd(R, np.float64)
    for e in (-500, 500):
        U, s, V, _ = jr.jacobi_svd(np.ldexp(R, e), np.float64)
        np.testing.assert_array_equal(U, U0)
        np.testing.assert_array_equal(V, V0)
        np.testing.assert_array_equal(s, np.ldexp(s0, e))
