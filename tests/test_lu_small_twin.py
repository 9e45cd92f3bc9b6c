"""CPU checks of the recurrences behind the single-pass LU solve kernel (tests/helpers/lu_small_twin.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from lu_small_twin import lu_factors, lu_panel_width, lu_solve_blocked  # noqa: E402
import lu_cases  # noqa: E402

SIZES = [1, 2, 17, 30, 64, 74, 84, 138, 139, 200, 256]


@pytest.mark.parametrize("m", SIZES)
def test_blocked_lu_solve_matches_numpy(m):
    rng = np.random.default_rng(m)
    W = rng.standard_normal((m, m))
    Z = rng.standard_normal((m, m))
    X, pmin, pmax, failed = lu_solve_blocked(W, Z)
    ref = np.linalg.solve(W, Z)
    assert failed == 0 and 0 < pmin <= pmax
    cond = np.linalg.cond(W)
    assert np.abs(X - ref).max() <= 1e-13 * cond * max(1.0, np.abs(ref).max())
    assert np.abs(W @ X - Z).max() <= 1e-12 * np.abs(W).max() * np.abs(X).max() * m


@pytest.mark.parametrize("m,nb", [(64, 16), (74, 32), (139, 16), (200, 48),
                                  (142, 16), (155, 16), (177, 16), (206, 16), (247, 16),          # every rung of the ladder ...
                                  (142, None), (155, None), (177, None), (206, None), (247, None)])  # ... at the plan's own width
def test_any_panel_width_gives_the_same_solution(m, nb):
    rng = np.random.default_rng(7 + m)
    W = rng.standard_normal((m, m)) * np.exp(-0.05 * np.arange(m))
    Z = rng.standard_normal((m, m))
    X1 = lu_solve_blocked(W, Z, nb=nb)[0]
    X2 = lu_solve_blocked(W, Z, nb=m)[0]
    assert np.abs(X1 - X2).max() <= 1e-9 * np.abs(X2).max()


def test_panel_width_ladder():
    """the rungs the GPU tests' sizes are the two ends of"""
    want = [(1, 141, None), (142, 154, 128), (155, 176, 112), (177, 205, 96), (206, 246, 80), (247, 256, 64)]
    for lo, hi, nb in want:
        for m in range(lo, hi + 1):
            assert lu_panel_width(m) == (m if nb is None else nb)
    assert all(m <= 141 or m == 256 or m % lu_panel_width(m) for m in lu_cases.SIZES)   # blocked sizes but 256: a ragged last panel


@pytest.mark.parametrize("ties", [False, True], ids=["unique", "ties"])
@pytest.mark.parametrize("m", lu_cases.SIZES)
def test_exact_family_is_exact_at_every_blocking(m, ties):
    """What the GPU tests rely on: on the dyadic family the twin returns X0, the L and U the case was built from and
    its permutation, bit for bit, at the plan's panel width, as one panel and in panels of 16 -- with unique pivots and
    with pivots tied across the waves of the kernel's search."""
    W, Z, X0, L, U, perm = lu_cases.exact_case(m, ties=ties)
    if ties:
        for j, seats in lu_cases.tie_seats(m).items():      # the ties sit in their seats, signs differ, no other row is as large
            col = L[perm][:, j]
            assert perm[seats[0]] == j and np.all(np.abs(col[seats]) == 1.0) and len(set(col[seats])) == 2
            assert np.all(np.abs(np.delete(col, seats)[np.delete(perm, seats) > j]) <= 0.5)
    first = None
    for nb in (None, m, 16):
        X, pmin, pmax, failed, LU, piv = lu_solve_blocked(W, Z, nb=nb, full=True)
        assert failed == 0
        np.testing.assert_array_equal(X, X0)
        Lf, Uf, pf = lu_factors(LU, piv, nb)
        np.testing.assert_array_equal(Lf, L)
        np.testing.assert_array_equal(Uf, U)
        np.testing.assert_array_equal(perm[pf], np.arange(m))
        assert pmin == np.abs(np.diag(U)).min() and pmax == np.abs(np.diag(U)).max()
        if m >= 3:
            assert (pmin, pmax) == (4.0, 16.0)
        first = piv if first is None else first
        np.testing.assert_array_equal(piv, first)


def test_higham_bounds_hold_for_the_twin():
    for kind in ("tinydiag", "random", "graded"):
        W, Z = lu_cases.pivoting_case(142, kind)
        X, _, _, failed, LU, piv = lu_solve_blocked(W, Z, full=True)
        r_fac, r_res, lmax = lu_cases.higham_ratios(W, Z, LU, piv, X)
        assert failed == 0 and lmax <= 1.0 and r_fac <= 1.0 and r_res <= 1.0


def test_panel_width_choice_fits_lds():
    for m in range(1, 257):
        nb = lu_panel_width(m)
        assert 1 <= nb <= m
        assert (64 + 64 + 256 + 128) * 8 + m * (nb | 1) * 8 + 64 <= 163840
        assert nb == m or nb % 16 == 0
    assert lu_panel_width(138) == 138 and lu_panel_width(256) == 64


def test_singular_and_nonfinite_are_reported():
    rng = np.random.default_rng(2)
    W = rng.standard_normal((30, 30))
    W[:, 5] = W[:, 9]
    assert lu_solve_blocked(W, np.eye(30))[3] == 2
    W[0, 0] = np.nan
    assert lu_solve_blocked(W, np.eye(30))[3] == 1


def test_overflow_during_elimination_is_reported():
    W = np.diag([1e-200, 1.0])                # finite input, the solution overflows
    Z = np.full((2, 2), 1e200)
    with np.errstate(over="ignore", invalid="ignore"):
        assert lu_solve_blocked(W, Z)[3] == 3
