"""Low-rank factor of a kernel covariance without a single apply: the greedy (diagonally pivoted) partial Cholesky factorisation
``C ~= L L^T`` of a ``KernelCovarianceOperator`` (hfmi_pchol_*, hippyflow_amd/csrc/hfmi_pchol.hip).

It reads the diagonal of ``C`` and the ``rank`` pivot columns only -- ``N rank^2`` flops against ``2 N^2 k`` for one apply of the
matrix-free operator -- and returns the trace of the residual ``C - L L^T`` after every step.  The residual is positive semidefinite, so
its trace bounds the error of every eigenvalue.  From ``L`` the KLE is a ``rank x rank`` eigenproblem (``MultiVector.gram_eig``) and prior
samples are ``L xi``.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .multivector import MatMvMult, MultiVector, MvDSmatMult
from .operators import CsrOperator, KernelCovarianceOperator, KernelCrossCovarianceOperator, as_device_operator


class _Factorisation:
    """Owner of an hfmi_pchol handle: the borrowed factor block keeps it alive, not the other way round."""

    def __init__(self, ctx):
        self.ctx = ctx                  # hfmi_pchol_destroy returns the storage to this context's pool: the context outlives the handle
        self.handle = C.c_void_p()

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                L.load().hfmi_pchol_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class PivotedCholesky:
    """Result of ``pivoted_cholesky``.  ``L``: the factor, a read-only ``MultiVector`` of ``rank`` vectors of length N borrowed from the
    library (it keeps the factorisation alive; its in-place members -- zero, scale, axpy, copy_from, swap, upload_async, orthogonalize --
    and those of its views raise; handing it to an operator as the OUTPUT block is not caught: do not); ``pivots`` (rank,), ``trace`` (rank + 1,): trace of ``C - L[:, :j] L[:, :j]^T`` for
    j = 0..rank; ``stop_reason``: 'max_rank', 'rel_tol' or 'floor' (the largest remaining diagonal entry is rounding)."""

    def __init__(self, op, max_rank, rel_tol=0.0):
        if not isinstance(op, KernelCovarianceOperator):
            raise ValueError("pivoted_cholesky: a KernelCovarianceOperator is required (got %s)" % type(op).__name__)
        self.ctx = op.ctx
        self._owner = _Factorisation(self.ctx)
        L.call("hfmi_pchol_create", op._op, int(max_rank), float(rel_tol), C.byref(self._owner.handle))
        self.handle = self._owner.handle
        rank, reason, trace0 = C.c_int(), C.c_int(), C.c_double()
        L.call("hfmi_pchol_info", self.handle, C.byref(rank), C.byref(reason), C.byref(trace0))
        self.rank = rank.value
        self.stop_reason = L.PCHOL_STOP_REASONS[reason.value]
        self.pivots = np.empty(self.rank, dtype=np.int64)
        self.trace = np.empty(self.rank + 1)
        L.call("hfmi_pchol_read", self.handle, L.ptr(self.pivots), L.ptr(self.trace))
        self.N = op.shape[0]
        self._L = None
        self._kernel = (op.points, op.family, op.sigma, op.ell, op.metric, getattr(op, "nu", None))     # what extend() evaluates K(., X_P) with
        self._LP_invT = None

    @property
    def L(self):
        if self._L is None:
            h = C.c_void_p()
            L.call("hfmi_pchol_factor", self.handle, C.byref(h))
            self._L = MultiVector(ctx=self.ctx, _handle=h, _parent=self._owner, _borrowed=True, _read_only=True)
        return self._L

    @property
    def residual_trace(self):
        return float(self.trace[-1])

    def eig(self, r, M=None):
        """The ``r`` leading eigenpairs of ``M (L L^T) M v = lambda M v`` with ``V^T M V = I`` (``L L^T v = lambda v`` for ``M = None``),
        from the rank x rank eigenproblem of ``L^T M L``: ``s, U = eigh(L^T M L)``, ``V = L U / sqrt(s)``, ``d = s``.  Returns
        ``(d, V, MV)``; ``MV`` is ``V`` itself without ``M``."""
        r = int(r)
        if not 1 <= r <= self.rank:
            raise ValueError("eig: r = %d outside 1..rank = %d" % (r, self.rank))
        Lf = self.L
        if M is None:
            ML = Lf
        else:
            M = as_device_operator(M, self.N, self.ctx)
            ML = MultiVector(self.N, self.rank, ctx=self.ctx)
            MatMvMult(M, Lf, ML)
        s, U = Lf.gram_eig(ML, r)
        d = s[:r].copy()
        if not d[-1] > 0.0:
            raise ValueError("eig: eigenvalue %d of the factor's Gram matrix is %g: ask for fewer than %d pairs" % (r, d[-1], r))
        Us = U / np.sqrt(d)[None, :]
        V = MultiVector(self.N, r, ctx=self.ctx)
        MvDSmatMult(Lf, Us, V)
        if M is None:
            return d, V, V
        MV = MultiVector(self.N, r, ctx=self.ctx)
        MvDSmatMult(ML, Us, MV)
        return d, V, MV

    def eigenvalue_error_bound(self, M=None):
        """Upper bound on ``lambda_i(exact) - lambda_i(eig)`` for every i (the lower bound is 0).  ``M = None``: the residual's trace.
        Otherwise ``||M||_inf`` times it: the pencil is similar to ``M^1/2 C M^1/2``, the perturbation ``M^1/2 E M^1/2`` is positive
        semidefinite and its norm is at most ``||M||_2 tr(E) <= ||M||_inf tr(E)``."""
        if M is None:
            return self.residual_trace
        M = as_device_operator(M, self.N, self.ctx)
        if not isinstance(M, CsrOperator):
            raise ValueError("eigenvalue_error_bound: the norm of M is read off its assembled (CSR) form")
        import scipy.sparse as sp
        absM = sp.csr_matrix((np.abs(M.csr.data), M.csr.indices, M.csr.indptr), shape=M.csr.shape)
        return float(absM.sum(axis=1).max()) * self.residual_trace

    def sample(self, n, seed):
        """``n`` draws ``X = L xi`` from N(0, L L^T): ``xi`` is a rank x n block of the device's Philox generator (hfmi_randn_fill, key
        ``seed``).  Returns ``(X, xi)``, two ``MultiVector``s.  ``xi`` crosses to the host and back as the small matrix of ``MvDSmatMult``
        (hfmi_block_gemm_small): meant for rank x n of that size, a few thousand columns at most per call."""
        xi = MultiVector(self.rank, int(n), ctx=self.ctx)
        L.call("hfmi_randn_fill", xi.handle, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(0), 1.0)
        X = MultiVector(self.N, int(n), ctx=self.ctx)
        MvDSmatMult(self.L, xi.to_dense(), X)
        return X, xi


    def extend(self, points):
        """The factor at other points: ``L* = K(points, X_P) L_P^-T`` with ``X_P`` the pivot points and ``L_P = L[pivots, :]`` (rank x
        rank, lower triangular in pivot order, inverted on the host).  A ``MultiVector`` of ``rank`` vectors with one row per point;
        at the operator's own points it reproduces ``L``.  No nugget enters: a nugget belongs to the point it sits on."""
        from scipy.linalg import solve_triangular
        if self.rank < 1:
            raise ValueError("extend: the factor has rank 0")
        pts, family, sigma, ell, metric, nu = self._kernel
        if self._LP_invT is None:
            LP = self.L.to_dense()[self.pivots, :]
            self._LP_invT = np.ascontiguousarray(solve_triangular(LP, np.eye(self.rank), lower=True).T)
        cross = KernelCrossCovarianceOperator(points, pts[self.pivots], family, sigma, ell, ctx=self.ctx, nu=nu, metric=metric)
        out = MultiVector(cross.shape[0], self.rank, ctx=self.ctx)
        cross.matMvMult(MultiVector.from_dense(self._LP_invT, ctx=self.ctx), out)
        return out

    def sample_at(self, points, xi):
        """``L* xi``: the draws ``sample`` returned as ``L xi``, evaluated at ``points`` (``xi``: its rank x n block)."""
        Ls = self.extend(points)
        X = MultiVector(Ls.size(), xi.nvec(), ctx=self.ctx)
        MvDSmatMult(Ls, xi.to_dense(), X)
        return X


def pivoted_cholesky(op, max_rank, rel_tol=0.0):
    """Factorise the covariance of a ``KernelCovarianceOperator``: at most ``max_rank`` (<= 16384) steps, stopping early when the
    residual's trace falls to ``rel_tol`` times the trace of ``C``."""
    return PivotedCholesky(op, max_rank, rel_tol)
