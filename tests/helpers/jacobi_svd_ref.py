"""Plain one-sided (Hestenes) Jacobi SVD in numpy, R = U diag(sigma) V^T, with the working precision as an argument.

dtype=np.longdouble: the high-precision reference of the tests of k_jacobi_svd (hippyflow_amd/csrc/hfmi_jacobi.hip); on
x86 that is the 64-bit significand of the x87 format, eps 1.1e-19, and the CPU suite holds it against a 50-digit SVD.
dtype=np.float64: a restatement of the kernel's arithmetic -- the same orthogonality test and rotation formula, column
pairs met in a round-robin tournament -- whose error against the reference is the yardstick for the kernel's.  The
restatement sums each dot product in numpy's order and meets the pairs in its own tournament order; the kernel sums
in 16 lanes and follows Brent and Luk's seats.  Neither is bit-comparable with the other; both are backward stable
column by column, which is what the relative accuracy of small singular values rests on (Demmel and Veselic 1992).

The orthogonality test is |a.b| <= tol sqrt(a.a) sqrt(b.b), with the two square roots taken separately: the product
a.a * b.b is the fourth power of the data and leaves the exponent range for entries beyond 1e+-77.

A column that is exactly zero is never rotated and stays zero; its singular value is 0 and its column of U is zero, as
the kernel leaves it.  V is orthogonal always."""
import numpy as np

MAX_SWEEPS = 60


def _rounds(n):
    """the n - 1 rounds of a round-robin tournament on n (even) players: lists of n / 2 disjoint pairs"""
    ring = list(range(n))
    for _ in range(n - 1):
        yield np.array(ring[:n // 2]), np.array(ring[n // 2:][::-1])
        ring = [ring[0]] + [ring[-1]] + ring[1:-1]


def jacobi_svd(R, dtype=np.longdouble):
    """returns (U, sigma, V, sweeps): sigma descending, columns of U / V the left / right vectors, in `dtype`"""
    W = np.array(R, dtype=dtype)
    k = W.shape[0]
    n = (k + 1) & ~1
    eps = np.finfo(dtype).eps
    V = np.eye(k, dtype=dtype)
    sweeps = 0
    while sweeps < MAX_SWEEPS and k > 1:
        worst = dtype(0)
        for a, b in _rounds(n):
            live = (a < k) & (b < k)              # the dummy player of an odd k
            a, b = a[live], b[live]
            x, y = W[:, a], W[:, b]
            al, be, ga = (x * x).sum(0), (y * y).sum(0), (x * y).sum(0)
            lim = np.sqrt(al) * np.sqrt(be)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(lim > 0, np.abs(ga) / lim, dtype(0))
                worst = max(worst, ratio.max(initial=dtype(0)))
                rot = ratio > eps
                zeta = (be - al) / (2 * ga)
                t = np.where(zeta >= 0, dtype(1), dtype(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            t = np.where(rot, t, dtype(0))
            c = 1 / np.sqrt(1 + t * t)
            s = c * t
            W[:, a], W[:, b] = c * x - s * y, s * x + c * y
            va, vb = V[:, a], V[:, b]
            V[:, a], V[:, b] = c * va - s * vb, s * va + c * vb
        sweeps += 1
        if worst <= 4 * eps:
            break
    sig = np.sqrt((W * W).sum(0))
    order = np.argsort(-sig, kind="stable")
    sig, W, V = sig[order], W[:, order], V[:, order]
    with np.errstate(divide="ignore", invalid="ignore"):
        U = np.where(sig > 0, W / sig, dtype(0))
    return U, sig, V, sweeps


# ------------------------------------------------------------------ the graded and rank-deficient cases of the GPU tests
# rank(k): how many singular values are non-zero by construction; the duplicated column's last one is rounding noise
ACCURACY_SIZES = [1, 2, 3, 16, 17, 64, 65]


def _triangular(k, rng):
    return np.triu(rng.standard_normal((k, k))) @ np.diag(np.logspace(0, -10, k))


def _two_sided(k, rng):
    return np.diag(np.logspace(0, -6, k)) @ rng.standard_normal((k, k)) @ np.diag(np.logspace(0, -12, k))


def _duplicated(k, rng):
    R = rng.standard_normal((k, k))
    R[:, k - 1] = R[:, k // 3]
    return R


def _zero_columns(k, rng):
    R = rng.standard_normal((k, k))
    R[:, k - 2:] = 0.0
    return R


# family: (generator, smallest k, rank(k))
ACCURACY_FAMILIES = {
    "triangular": (_triangular, 1, lambda k: k),
    "two-sided": (_two_sided, 1, lambda k: k),
    "duplicated": (_duplicated, 2, lambda k: k - 1),
    "zero-columns": (_zero_columns, 3, lambda k: k - 2),
}

# Worst relative error of the non-zero singular values of the fp64 restatement against the longdouble reference,
# measured on the CPU (x86-64, numpy 2): what accuracy_tolerance() returns an eighth of, before the 8 k eps floor.
# The triangular family at k = 64, 65 is the odd one out: a Gaussian triangular matrix is itself ill conditioned
# (its condition number grows like 2^k), the small singular values are then not determined to any relative accuracy by
# fp64 data -- nor, beyond 1e19, by the longdouble reference -- and the relative bound there is vacuous.  What holds
# those cases is the absolute bound |sigma - ref| <= 8 k eps sigma_1 that the tests assert next to the relative one
# (Weyl's inequality with the backward error of the rotations), the descending order and the reconstruction.
#                k:     1        2        3        16       17       64       65
MEASURED = {
    "triangular":   (0.0,     6.2e-19, 1.3e-16, 4.1e-15, 3.9e-15, 7.5e-01, 5.9e-01),
    "two-sided":    (0.0,     6.9e-17, 5.7e-16, 3.1e-14, 6.6e-15, 2.3e-14, 3.5e-14),
    "duplicated":   (None,    1.7e-16, 1.4e-16, 1.5e-15, 2.8e-15, 8.7e-15, 8.1e-15),
    "zero-columns": (None,    None,    1.4e-16, 1.2e-15, 1.9e-15, 8.0e-15, 7.4e-15),
}


def accuracy_case(family, k):
    gen, kmin, rank = ACCURACY_FAMILIES[family]
    assert k >= kmin
    return gen(k, np.random.default_rng([k, sorted(ACCURACY_FAMILIES).index(family)])), rank(k)


def accuracy_cases():
    return [(f, k) for f, (_, kmin, _) in ACCURACY_FAMILIES.items() for k in ACCURACY_SIZES if k >= kmin]


def restatement_error(R, rank, ref_sigma):
    """worst relative error of the leading `rank` singular values of the fp64 restatement"""
    sig = jacobi_svd(R, np.float64)[1]
    ref = np.asarray(ref_sigma[:rank], dtype=np.longdouble)
    return float(np.max(np.abs(sig[:rank].astype(np.longdouble) - ref) / ref)) if rank else 0.0


def accuracy_tolerance(R, rank, ref_sigma):
    """what the kernel is allowed: 8 x the restatement's own error (margin for the other summation and pair order),
    at least 8 k eps"""
    k = R.shape[0]
    return max(8.0 * restatement_error(R, rank, ref_sigma), 8.0 * k * np.finfo(np.float64).eps)
