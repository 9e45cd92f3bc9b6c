"""Operands for the tests of k_lu_solve and of its numpy twin (lu_small_twin.py), and Higham's componentwise bounds.

Exact family: W = P (L U) with L unit lower triangular, entries in {0, +-1/2} below the diagonal, U upper triangular with
integer entries in [-2, 2] above a diagonal of +-{4, 8, 16}, P a seeded row permutation, X0 integer in [-3, 3] and
Z = W X0.  In column j of the reduced matrix the candidates are L_ij U_jj: the row of L's diagonal wins alone, so partial
pivoting undoes P, every pivot is a power of two and every intermediate is a short dyadic number -- the elimination is
exact in any order, with or without fma, and X == X0, L\\U == the twin's, bit for bit, at every panel width.

Ties: the same with a few sub-diagonal entries of L set to +-1, so that several rows tie for the pivot of a column, with
differing signs; P seats them in different waves of the kernel's pivot search (one row per thread, 64 rows per wave).
Column 0: the diagonal's row in seat 0, ties in seats 63, 64 and 200 (waves 0, 0, 1, 3) -- no exchange.  Column 40: the
diagonal's row in seat 104 and ties in seats 170 and 240 (waves 1, 2, 3), smaller entries in front of them -- an exchange
with a row no first wave sees.  "First row of largest |entry|" takes the diagonal's row both times and the
factorisation is still the one written down; any other rule (last row, largest signed value, first wave only, a
cross-wave merge that forgets the row index) takes another row and leaves other bits."""
import numpy as np

from lu_small_twin import EPS, lu_factors, lu_panel_width

# both ends of every rung of lu_panel_width's ladder (nb = m up to 141, then 128, 112, 96, 80, 64), and 64 +- 1, 16 + 1
SIZES = [1, 2, 3, 16, 17, 63, 64, 65, 141, 142, 154, 155, 176, 177, 205, 206, 246, 247, 255, 256]


def tie_seats(m):
    """{column: seats}: the first seat holds the row of L's diagonal, the others rows with +-1 in that column"""
    out = {}
    if m >= 2:
        out[0] = [0] + ([s for s in (63, 64, 200) if s < m] or [m - 1])
    if m > 105:
        out[40] = [104] + ([s for s in (170, 240) if s < m] or [m - 1])
    return out


def exact_case(m, seed=0, ties=False):
    """returns W, Z, X0, L, U, perm with W = (L U)[perm]"""
    rng = np.random.default_rng([m, seed, int(ties)])
    L = np.tril(rng.integers(-1, 2, (m, m)) * 0.5, -1) + np.eye(m)
    U = np.triu(rng.integers(-2, 3, (m, m)).astype(np.float64), 1)
    d = rng.choice([4.0, 8.0, 16.0], m) * rng.choice([-1.0, 1.0], m)
    if m >= 3:                                  # both extreme pivots occur: the status words are 4 and 16
        i4 = int(rng.integers(0, m))
        d[i4] = 4.0
        d[(i4 + 1 + int(rng.integers(0, m - 1))) % m] = -16.0
    U += np.diag(d)
    perm = rng.permutation(m)
    if ties:
        fixed = set()
        perm = np.arange(m)
        for j, seats in tie_seats(m).items():
            perm[[j, seats[0]]] = perm[[seats[0], j]]          # the diagonal's row into the first seat
            for r, sgn in zip(seats[1:], (-1.0, 1.0, -1.0)):
                L[r, j] = sgn                                  # seat r holds row r
            fixed |= {j} | set(seats)
        free = np.array(sorted(set(range(m)) - fixed), dtype=int)
        perm[free] = rng.permutation(free)      # every other row still has to be found by pivoting
    X0 = rng.integers(-3, 4, (m, m)).astype(np.float64)
    W = (L @ U)[perm]
    return W, W @ X0, X0, L, U, perm


def pivoting_case(m, kind):
    """Gaussian operands that need their row exchanges: 'tinydiag' (every diagonal entry times 1e-14), and the 'random'
    and 'graded' families of test_gpu_single_pass.py::test_small_solve_matches_numpy"""
    rng = np.random.default_rng(m)
    W = rng.standard_normal((m, m))
    if kind == "graded":
        W = W * np.exp(-0.04 * np.arange(m))[None, :] * np.exp(-0.02 * np.arange(m))[:, None]
    Z = rng.standard_normal((m, m))
    if kind == "tinydiag":
        W[np.arange(m), np.arange(m)] *= 1e-14
    return W, Z


def gamma(n):
    return n * (EPS / 2) / (1.0 - n * (EPS / 2))      # Higham's gamma_n with the unit roundoff u = eps / 2


def higham_ratios(W, Z, LU, piv, X, nb=None):
    """worst ratios (<= 1 for any correctly working Gaussian elimination in fp64, fma or not, blocked or not) of
       |P W - L U| <= gamma_m |L| |U|                       (Higham, Accuracy and Stability, Thm 9.3)
       |W X - Z|   <= gamma_3m P^T |L| |U| |X|              (Thm 9.4)
    componentwise, residuals in extended precision, and max |L|"""
    m = W.shape[0]
    L, U, perm = lu_factors(LU, piv, nb)
    ld = np.longdouble
    aL, aU = np.abs(L).astype(ld), np.abs(U).astype(ld)
    fac = np.abs(W[perm].astype(ld) - L.astype(ld) @ U.astype(ld))
    bound = aL @ aU
    r_fac = float(np.max(fac / (gamma(m) * bound + np.finfo(np.float64).tiny)))
    res = np.abs(W[perm].astype(ld) @ X.astype(ld) - Z[perm].astype(ld))
    bound = bound @ np.abs(X).astype(ld)
    r_res = float(np.max(res / (gamma(3 * m) * bound + np.finfo(np.float64).tiny)))
    return r_fac, r_res, float(np.abs(L).max())


__all__ = ["SIZES", "exact_case", "pivoting_case", "higham_ratios", "tie_seats", "lu_panel_width"]
