"""CPU checks of the numpy twin of the wide Cholesky + inverse (tests/helpers/chol_wide_twin.py, hippyflow_amd/csrc/hfmi_chol_wide.hip):
the blocked recurrences against LAPACK, and the shift / breakdown rule."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from chol_wide_twin import EPS, NB, chol_wide, diag_block, gram_with_condition, qr_shift_rel  # noqa: E402


@pytest.mark.parametrize("k", [257, 300, 512, 513, 1000])
def test_blocked_factor_and_inverse_match_lapack(k):
    """cond(G) = 1e4, cond(R) = 1e2: the factor to k eps cond(R) of LAPACK's, the inverse against solve_triangular, both triangular"""
    g = gram_with_condition(k, 1e4, seed=k)
    r, x, st = chol_wide(g, qr_shift_rel(2 * k, k))
    rl = np.linalg.cholesky(g).T
    xl = sl.solve_triangular(rl, np.eye(k), lower=False)
    assert st["shifted"] == 0 and st["failed"] == 0 and 0.0 < st["min_pivot_ratio"] <= 1.0
    assert np.abs(r - rl).max() <= 1e-12 * np.abs(rl).max()
    assert np.abs(x - xl).max() <= 1e-11 * np.abs(xl).max()
    assert not np.tril(r, -1).any() and not np.tril(x, -1).any() and np.all(np.diag(r) > 0)
    u = 0.5 * EPS
    gamma = (k + 1) * u / (1 - (k + 1) * u)
    assert np.linalg.norm(r.T @ r - g) <= gamma * np.trace(g)
    assert np.linalg.norm(r @ x - np.eye(k)) / np.sqrt(k) <= 8 * k * u * np.linalg.cond(r)
    d = np.sqrt(np.diag(g))
    assert abs(st["gram_dev"] - np.linalg.norm(g / np.outer(d, d) - np.eye(k))) <= 1e-12 * st["gram_dev"]


def test_diagonal_block_matches_lapack():
    rng = np.random.default_rng(5)
    for n in (1, 44, NB):
        b = rng.standard_normal((3 * n + 2, n))
        a = b.T @ b
        r, x, ratio = diag_block(a, np.diag(a).copy(), 64 * n * EPS)
        rl = np.linalg.cholesky(a).T
        assert np.abs(r - rl).max() <= 1e-13 * np.abs(rl).max()
        assert np.abs(r @ x - np.eye(n)).max() < 1e-12
        assert 0.0 < ratio <= 1.0


def test_duplicated_column_takes_the_shifted_attempt():
    """a pivot at round-off level restarts the factorisation once with shift_rel * trace(G) on the diagonal: R^T R = G + shift I"""
    k, n = 300, 600
    z = np.random.default_rng(0).standard_normal((n, k))
    z[:, 77] = z[:, 5]
    g = z.T @ z
    shift_rel = qr_shift_rel(n, k)
    r, x, st = chol_wide(g, shift_rel)
    assert st["shifted"] == 1 and st["failed"] == 0
    assert 0.0 < st["min_pivot_ratio"] < 1e-5          # the shifted pivot of the duplicate: ~ shift / G_jj
    gs = g + shift_rel * np.trace(g) * np.eye(k)
    assert np.linalg.norm(r.T @ r - gs) <= 1e-13 * np.linalg.norm(gs)
    assert np.abs(np.linalg.solve(r.T, gs) @ x - np.eye(k)).max() < 1e-6     # R x = I up to cond(R) ~ 1e7


@pytest.mark.parametrize("case", ["indefinite", "nan"])
def test_second_breakdown_is_a_failure(case):
    k = 300
    g = gram_with_condition(k, 1e4, seed=9)
    if case == "indefinite":
        g[200, 200] = -1.0
    else:
        g[70, 3] = np.nan
    r, x, st = chol_wide(g, qr_shift_rel(2 * k, k))
    assert st["shifted"] == 1 and st["failed"] == 1 and st["min_pivot_ratio"] == 0.0
    assert not r.any() and not x.any()
