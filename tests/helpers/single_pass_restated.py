"""CPU restatement of the single-pass randomized eigensolvers (hippylib randomizedEigensolver.singlePass / singlePassG)
exactly as hippyflow_amd.randomized states them: power loop without orthogonalisation, (B-)orthonormal basis of the last
iterate, Wt = P^T (B) Q, Zt = Ybar^T Q, T = sym(Wt^-1 Zt), eigh, U = Q V[:, :k].  Dense numpy; test infrastructure only."""
import numpy as np
import scipy.linalg as sla


def _orth(Y):
    Q, R = np.linalg.qr(Y)
    return Q * np.sign(np.diag(R))          # positive diagonal: the QR the device computes


def _borth(Y, B):
    G = Y.T @ B @ Y
    R = np.linalg.cholesky(0.5 * (G + G.T)).T
    Q = sla.solve_triangular(R, Y.T, trans='T', lower=False).T
    return Q, B @ Q


def _finish(Q, Wt, Zt, k, sort_by_abs):
    Tt = np.linalg.solve(Wt, Zt)
    d, V = np.linalg.eigh(0.5 * (Tt + Tt.T))
    order = np.argsort(np.abs(d) if sort_by_abs else d)[::-1][:k]
    return d[order], Q @ V[:, order]


def single_pass(A, Omega, k, s=1, sort_by_abs=False):
    """A: dense symmetric N x N (or a callable X -> A X); Omega: N x m."""
    apply = A if callable(A) else (lambda X: A @ X)
    P, Y = None, np.array(Omega, dtype=np.float64)
    for _ in range(s):
        P, Y = Y, apply(Y)
    Q = _orth(Y)
    return _finish(Q, P.T @ Q, Y.T @ Q, k, sort_by_abs)


def single_pass_g(A, B, Binv, Omega, k, s=1, sort_by_abs=False):
    """A u = lambda B u: A, B dense symmetric (B SPD), Binv a callable (default: a dense solve with B)."""
    apply = A if callable(A) else (lambda X: A @ X)
    solve = Binv if Binv is not None else (lambda X: np.linalg.solve(B, X))
    P, Y, Ybar = None, np.array(Omega, dtype=np.float64), None
    for _ in range(s):
        Ybar = apply(Y)
        P, Y = Y, solve(Ybar)
    Q, BQ = _borth(Y, B)
    return _finish(Q, P.T @ BQ, Ybar.T @ Q, k, sort_by_abs)


def subspace_angle(U, V, B=None):
    """largest principal angle between range(U) and range(V) (B-inner product when B is given)"""
    if B is not None:
        L = np.linalg.cholesky(B)
        U, V = L.T @ U, L.T @ V
    Qu, _ = np.linalg.qr(U)
    Qv, _ = np.linalg.qr(V)
    # sine form (the arccos of the cosines cannot resolve angles below ~1e-8)
    return float(np.arcsin(min(1.0, np.linalg.norm(Qv - Qu @ (Qu.T @ Qv), 2))))
