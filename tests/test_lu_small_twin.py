"""CPU checks of the recurrences behind the single-pass LU solve kernel (tests/helpers/lu_small_twin.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from lu_small_twin import lu_panel_width, lu_solve_blocked  # noqa: E402

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


@pytest.mark.parametrize("m,nb", [(64, 16), (74, 32), (139, 16), (200, 48)])
def test_any_panel_width_gives_the_same_solution(m, nb):
    rng = np.random.default_rng(7 + m)
    W = rng.standard_normal((m, m)) * np.exp(-0.05 * np.arange(m))
    Z = rng.standard_normal((m, m))
    X1 = lu_solve_blocked(W, Z, nb=nb)[0]
    X2 = lu_solve_blocked(W, Z, nb=m)[0]
    assert np.abs(X1 - X2).max() <= 1e-9 * np.abs(X2).max()


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
