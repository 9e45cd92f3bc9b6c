"""Cases and order-free properties of a pivoted Cholesky factor of a kernel covariance, shared by the CPU suite (which runs them on the
numpy twin, tests/helpers/pchol_twin.py) and the GPU suite (which runs them on hfmi_pchol_create's result).  Every bound is the worst case
of the arithmetic, none is fitted to an implementation:

  * pivot columns: column p_j of C equals sum_c L[:, c] L[p_j, c], a sum of at most ``rank`` products in some order plus the rounding of
    the entry itself: (rank + 2) eps (|L| |L[piv, :]|^T + |C[:, piv]|), times 8 for the few-ulp difference between the device's exp / sqrt
    and numpy's (the convention of tests/test_gpu_kernel_cov.py);
  * trace identity: trace[j] = N d0 - ||L[:, :j]||_F^2, each of the N diagonal entries carrying j subtractions of squares <= d0;
  * eigenvalues: C - L L^T is positive semidefinite with trace trace[-1], so 0 <= lam_i(C) - lam_i(L L^T) <= trace[-1] (Weyl), up to the
    rounding of two symmetric eigensolves of order N (16 N eps lam_0).
"""
import numpy as np

from hippyflow_amd import _lib
from hippyflow_amd.operators import kernel_cov_host

EPS = np.finfo(np.float64).eps
SIGMA = 1.3
MAX_RANK, REL_TOL, FLOOR = 0, 1, 2

# N, d, family, ell, nugget, max_rank.  N: one point; below a wave; ragged and exact row tiles (63, 64, 65, 193, 257); several
# workgroups (1000, 1500); many (20000, 140000: 547 row tiles, still one tile per workgroup on a 256-CU device); 8 * 256 * 256 + 1 rows are
# 2049 row tiles, more than the 8 workgroups of four waves a compute unit can hold on 256 units, so the grid-stride loop takes a second tile
# with the default grid (the GPU suite asserts this of the device it runs on, and walks many tiles per workgroup at small N with the
# "pchol_grid" knob).  max_rank: min(max_rank, N) on both sides; 2 PC_CHUNK + 1 crosses the LDS chunk of the pivot's row twice.
CASES = [
    (1, 1, "matern12", 1.0, 0.3, 4),
    (2, 1, "sqexp", 0.5, 0.0, 2),
    (15, 2, "matern32", 0.05, 0.0, 15),
    (63, 3, "matern52", 1.0, 0.0, 40),
    (64, 2, "matern32", 0.3, 0.3, 64),
    (65, 2, "matern52", 0.5, 0.0, 65),
    (193, 1, "sqexp", 1.0, 0.0, 60),
    (257, 3, "matern12", 0.3, 0.0, 100),
    (1000, 2, "matern32", 0.3, 0.0, 138),
    (1500, 2, "matern12", 0.05, 0.0, 2 * _lib.PC_CHUNK + 1),
    (20000, 2, "matern32", 0.1, 0.2, 16),
    (140000, 2, "matern32", 0.1, 0.2, 3),
    (8 * 256 * 256 + 1, 2, "matern32", 0.1, 0.2, 3),
]
SECOND_TILE_CASE = CASES[-1]
ROWS_PER_TILE = 256                                                            # PC_THREADS of hfmi_pchol.hip
FLOOR_CASE = (193, 1, "sqexp", 1.0, 0.0, 60)                                  # stops with FLOOR well below max_rank
ENDS_EARLY = [(65, 2, "matern52", 0.5, 0.0, 65), (15, 2, "matern32", 0.05, 0.0, 15)]   # the coincident pair: N - 1 distinct points
PIVOTS_COMPARABLE = [c for c in CASES if c[0] in (63, 64, 257, 1000)]         # twin's gap between best and next diagonal >= MIN_GAP
MIN_GAP = 1e-6
# the (1000 ...) points and kernel; its max_rank of 138 leaves 5.3e-3 of the trace, so the stop test allows 400 steps (the twin needs 332)
REL_TOL_CASE, REL_TOL_VALUE = (1000, 2, "matern32", 0.3, 0.0, 400), 1e-3


def case_id(case):
    return "N%d-d%d-%s-ell%g-nug%g-k%d" % case


def scattered(N, d, seed):
    """seeded points in the unit cube, two of them coincident (as tests/test_gpu_kernel_cov.py)"""
    pts = np.random.default_rng(seed).random((N, d))
    if N > 3:
        pts[N - 1] = pts[1]
    return pts


def case_points(case):
    N, d = case[0], case[1]
    return scattered(N, d, seed=N + d)


def floor_of(case):
    N, _, _, _, nugget, max_rank = case
    return 4 * min(max_rank, N) * EPS * (SIGMA ** 2 + nugget)


def check_properties(case, L, pivots, trace, rank, stop_reason, label):
    """The order-free properties of one factorisation of ``case``; prints each measured figure before it asserts."""
    N, d, family, ell, nugget, max_rank = case
    pts = case_points(case)
    d0 = SIGMA ** 2 + nugget
    L, pivots, trace = np.asarray(L), np.asarray(pivots), np.asarray(trace)
    assert L.shape == (N, rank) and pivots.shape == (rank,) and trace.shape == (rank + 1,)
    assert 1 <= rank <= min(max_rank, N)
    assert pivots[0] == 0                                                          # all diagonals tie: lowest index
    assert len(set(pivots.tolist())) == rank and pivots.min() >= 0 and pivots.max() < N
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(trace))
    assert np.all(np.diff(trace) <= 0.0), "trace increases"
    if nugget == 0.0 and N > 3:
        assert not ({1, N - 1} <= set(pivots.tolist())), "both points of the coincident pair were chosen"
    # pivot columns
    Cp = kernel_cov_host(pts, family, SIGMA, ell, nugget, rows=pivots).T          # (N, rank): C is symmetric
    Lp = L[pivots, :]                                                              # (rank, rank)
    err = np.abs(Cp - L @ Lp.T)
    bound = 8 * (rank + 2) * EPS * (np.abs(L) @ np.abs(Lp).T + np.abs(Cp))
    print("%s %s: rank %d stop %d; pivot columns max err/bound = %.3g" % (label, case_id(case), rank, stop_reason,
                                                                        float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(err <= bound)
    # trace identity
    # column sums over the contiguous axis: numpy adds pairwise there (down the rows of an (N, rank) array it adds one row after the other,
    # and the rounding of THAT sum, about sqrt(N) eps, is beyond the bound below from N = 5e5 on)
    sq = np.concatenate([[0.0], np.cumsum(np.sum(np.ascontiguousarray(L.T) ** 2, axis=1))])
    terr = np.abs(trace - (N * d0 - sq))
    tbound = 8 * (np.arange(rank + 1) + 2) * N * EPS * d0
    print("%s %s: trace identity max err/bound = %.3g" % (label, case_id(case), float(np.max(terr / tbound))))
    assert np.all(terr <= tbound)
    # eigenvalues against the dense matrix
    if N <= 1500:
        lam = np.linalg.eigvalsh(kernel_cov_host(pts, family, SIGMA, ell, nugget))[::-1]
        mu = np.zeros(N)
        mu[:rank] = np.linalg.eigvalsh(L.T @ L)[::-1]
        slack = 16 * N * EPS * lam[0]
        gap = lam - mu
        print("%s %s: lam(C) - lam(L L^T) in [%.3g, %.3g], residual trace %.3g, slack %.3g" % (label, case_id(case), gap.min(), gap.max(),
                                                                                            trace[-1], slack))
        assert np.all(gap >= -slack) and np.all(gap <= trace[-1] + slack)
    if case == FLOOR_CASE:
        assert stop_reason == FLOOR and rank < max_rank and rank <= 12, (stop_reason, rank)
    if case in ENDS_EARLY:
        assert rank < N and trace[-1] <= N * floor_of(case), (rank, trace[-1], N * floor_of(case))
