"""CPU checks of the single-pass restatement (tests/helpers/single_pass_restated.py) against scipy.linalg.eigh."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from single_pass_restated import single_pass, single_pass_g, subspace_angle  # noqa: E402


def _low_rank(N, m, rng, decay=0.15):
    W, _ = np.linalg.qr(rng.standard_normal((N, m)))
    d = np.exp(-decay * np.arange(m)) * 3.0
    return (W * d) @ W.T, d


@pytest.mark.parametrize("m,s", [(10, 1), (30, 1), (30, 2)])
def test_exact_rank_hep_matches_eigh(m, s):
    rng = np.random.default_rng(m + s)
    A, d_true = _low_rank(400, m, rng)
    Omega = rng.standard_normal((400, m))
    k = m - 3
    d, U = single_pass(A, Omega, k, s=s)
    d_ref, V_ref = sla.eigh(A)
    d_ref, V_ref = d_ref[::-1][:k], V_ref[:, ::-1][:, :k]
    assert np.abs(d - d_ref).max() <= 1e-10 * np.abs(d_ref).max()
    assert np.abs(U.T @ U - np.eye(k)).max() < 1e-12
    assert subspace_angle(U[:, :5], V_ref[:, :5]) < 1e-8


@pytest.mark.parametrize("s", [1, 2])
def test_exact_rank_ghep_matches_eigh(s):
    rng = np.random.default_rng(11 + s)
    N, m, k = 300, 20, 15
    X = rng.standard_normal((N, m))
    A = X @ np.diag(np.exp(-0.2 * np.arange(m))) @ X.T
    G = rng.standard_normal((N, N))
    B = G @ G.T / N + np.eye(N)
    Omega = rng.standard_normal((N, m))
    d, U = single_pass_g(A, B, None, Omega, k, s=s)
    d_ref = sla.eigh(A, B, eigvals_only=True)[::-1][:k]
    assert np.abs(d - d_ref).max() <= 1e-10 * np.abs(d_ref).max()
    assert np.abs(U.T @ B @ U - np.eye(k)).max() < 1e-10


def test_decaying_spectrum_converges_as_m_grows():
    rng = np.random.default_rng(5)
    N = 600
    W, _ = np.linalg.qr(rng.standard_normal((N, N)))
    lam = 0.8 ** np.arange(N)
    A = (W * lam) @ W.T
    errs = []
    for m in (10, 20, 40, 80):
        Omega = np.random.default_rng(m).standard_normal((N, m))
        d, _ = single_pass(A, Omega, 5)
        errs.append(np.abs(d - lam[:5]).max() / lam[0])
    assert errs[-1] < 1e-6
    assert errs[-1] < 1e-3 * errs[0]
    assert all(b <= a * 1.5 + 1e-14 for a, b in zip(errs, errs[1:]))
