"""Randomized double- and single-pass eigensolvers and the probe draw: the device counterparts of the hippylib
entry points hippyflow calls (hippylib is absent from /root/reference; call sites:
modeling/PODProjector.py:376, modeling/KLEProjector.py:163-164,177,
modeling/activeSubspaceProjector.py:449-463,556-577,654).

``doublePass(A, Omega, k, s=1)``             -> (d, U),   U^T U = I
``doublePassG(A, B, Binv, Omega, k, s=1)``   -> (d, U),   U^T B U = I,  A U ~ B U diag(d)
``doublePassC(A, C, Omega, k, s=1)``         -> (d, U, E): doublePassG(A, C^-1, C) without C^-1; E = C^-1 U, E^T U = I
``singlePass(A, Omega, k, s=1)`` / ``singlePassG(A, B, Binv, Omega, k, s=1)``: the same results from s applications of
A instead of s + 1 (hippylib's randomizedEigensolver.singlePass[G]); ``StreamedSketch`` builds their sketch A Omega while
the samples are produced, without storing them
``parRandom.normal(sigma, out)``             -> N(0, sigma^2) fill of a Vector / MultiVector

Two execution routes, same arithmetic:
* fused: when A (and B, Binv) are device operators -- possibly wrapped in a CollectiveOperator --
  one call to ``hfmi_double_pass[_g]`` keeps every intermediate in HBM; with a ``NativeCollective`` the rank
  average is an RCCL all-reduce enqueued by the C solve itself (``hfmi_op_set_collective``), with any other
  collective object it is a post-apply hook that all-reduces the result block in place;
* generic: any object with the reference's ``mult`` / ``matMvMult`` protocol; the steps
  (MatMvMult, (B-)orthogonalize, dot_mv, small eigensolve, MvDSmatMult) are each a C-ABI call.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as L
from . import hostvec as H
from .collectives import CollectiveOperator, MatrixMultCollectiveOperator, NativeCollective, NullCollective
from .multivector import MatMvMult, MultiVector, MvDSmatMult, Vector
from .operators import DeviceOperator, as_device_operator


class _ParRandom:
    """hp.parRandom stand-in: counter-based Philox4x32-10 + Box-Muller on the device (hfmi_randn_fill).

    hp.parRandom is seeded per process and only Omega, drawn on rank 0, travels (activeSubspaceProjector.py:433-443).
    Here the Philox key is (seed, namespace) and there are two families of streams:

    * SHARED draws (namespace 0, counter ``shared_stream``): every rank that makes the same sequence of calls gets the
      same numbers, so a probe block needs no broadcast.  Default for blocks (``MultiVector``).
    * PRIVATE draws (namespace rank + 1, counter ``stream``): distinct on every rank and disjoint from every shared
      draw -- the Monte-Carlo noise of the sampling loops.  Default for vectors, device or host.

    A host (dolfin-like) vector is filled through a device block of its length and ``set_local``."""

    def __init__(self, seed=1, rank=None):
        self.seed = int(seed)
        self.rank = L.launcher_rank() if rank is None else int(rank)
        self.stream = 0
        self.shared_stream = 0
        self._keyed = False

    def reseed(self, seed, stream=0):
        self.seed, self.stream, self.shared_stream = int(seed), int(stream), int(stream)

    def split(self, rank, by_collective=False):
        """Re-key the private draws for this rank of a sample-parallel run.  Called explicitly it always applies.  The FIRST
        collective a process constructs calls it with ``by_collective=True`` (the world / sample-parallel communicator, as in
        the reference, where hp.parRandom is seeded per MPI rank); collectives built later -- e.g. over a sub-group in which
        several processes hold the same group rank -- leave the key alone: re-keying there would collapse private streams
        onto one key and change the draws in the middle of a run."""
        if by_collective and self._keyed:
            return
        self.rank = int(rank)
        self._keyed = True          # an explicit split is final too: a collective constructed afterwards must not override it

    def key(self, shared):
        return (self.seed & 0xFFFFFFFF) | ((0 if shared else (self.rank + 1) & 0xFFFFFFFF) << 32)

    def normal(self, sigma, out, shared=None):
        host = H.is_host_vector(out)
        if shared is None:
            shared = isinstance(out, MultiVector)
        if shared:
            stream, self.shared_stream = self.shared_stream, self.shared_stream + 1
        else:
            stream, self.stream = self.stream, self.stream + 1
        if host:
            mv = MultiVector(int(len(out.get_local())), 1)
        else:
            mv = out._mv if isinstance(out, Vector) else out
        L.call("hfmi_randn_fill", mv.handle, C.c_uint64(self.key(shared)), C.c_uint32(stream & 0xFFFFFFFF), float(sigma))
        if host:
            out.set_local(mv.to_vectors()[0])
            out.apply("")

    def normal_perturb(self, sigma, out):
        if H.is_host_vector(out):
            tmp = H._copy_vector(out)
            self.normal(sigma, tmp)
            out.axpy(1.0, tmp)
            return
        tmp = MultiVector(out._mv if isinstance(out, Vector) else out)
        self.normal(sigma, Vector(ctx=tmp.ctx, _mv=tmp) if isinstance(out, Vector) else tmp)
        (out._mv if isinstance(out, Vector) else out).axpy(1.0, tmp)


parRandom = _ParRandom()


def sym_eig_small(T, sort_by_abs=False, ctx=None, method="dc", nvec=None):
    """np.linalg.eigh(T) + descending sort, on the device.  ``method="dc"``: Householder tridiagonalisation + divide
    and conquer (the algorithm family of the LAPACK routine behind np.linalg.eigh; up to 256 rows on one compute unit,
    up to 16384 over the whole GPU); ``"jacobi"``: one-workgroup cyclic Jacobi (high relative accuracy of small
    eigenvalues of graded positive definite matrices).  ``nvec``: return only the leading ``nvec`` eigenvectors
    (all eigenvalues still) -- ``la.eigh(G)[1][:, :u_rank]`` of PODProjector.py:821-826 without back-transforming
    and reading back the rest."""
    if method not in ("dc", "jacobi"):
        raise ValueError("sym_eig_small: method must be 'dc' or 'jacobi'")
    T = L.as_f64(T)
    k = T.shape[0]
    flags = (1 if sort_by_abs else 0) | (2 if method == "jacobi" else 0)
    handle = (ctx or L.Context.default()).handle
    if nvec is not None and int(nvec) < k:
        nvec = int(nvec)
        d, V = np.empty(k), np.empty((k, nvec))
        L.call("hfmi_sym_eig_leading", handle, L.ptr(T), k, flags, nvec, L.ptr(d), L.ptr(V))
        return d, V
    d, V = np.empty(k), np.empty((k, k))
    L.call("hfmi_sym_eig_small", handle, L.ptr(T), k, flags, L.ptr(d), L.ptr(V))
    return d, V


def _unwrap_collective(A):
    """(local device operator, collective, mpi_op) if A is a (possibly wrapped) device operator."""
    if isinstance(A, (CollectiveOperator, MatrixMultCollectiveOperator)):
        local = A.local_op
        dev = local if isinstance(local, DeviceOperator) else (local._device_operator() if hasattr(local, "_device_operator") else None)
        return dev, A.collective, A.mpi_op
    if isinstance(A, DeviceOperator):
        return A, None, None
    if hasattr(A, "_device_operator"):
        return A._device_operator(), None, None
    return None, None, None


class _PostApplyHook:
    """All-reduce of the operator's result block, called from inside the fused C solve."""

    def __init__(self, dev_op, collective, mpi_op):
        self.error = None

        def _cb(user, block_handle):
            try:
                mv = MultiVector(ctx=dev_op.ctx, _handle=C.c_void_p(block_handle), _borrowed=True)
                collective.allReduce(mv, mpi_op)
                return 0
            except Exception as exc:
                self.error = exc
                return 1

        self.cb = L.POST_APPLY_FN(_cb)
        self.dev_op = dev_op

    def __enter__(self):
        L.call("hfmi_op_set_post_apply", self.dev_op._op, self.cb, None)
        return self

    def __exit__(self, *exc):
        L.call("hfmi_op_set_post_apply", self.dev_op._op, L.POST_APPLY_FN(), None)
        return False


def _fused(A_dev, collective, mpi_op, B_dev, Binv_dev, Omega, k, s, sort_by_abs, use_mgs, literal_T=False, entry="hfmi_double_pass"):
    d = np.empty(k)
    U = MultiVector(Omega.size(), k, ctx=Omega.ctx)
    flags = (1 if sort_by_abs else 0) | (2 if use_mgs else 0) | (4 if literal_T else 0)

    def run():
        if B_dev is None:
            L.call(entry, A_dev._op, Omega.handle, int(k), int(s), flags, L.ptr(d), U.handle)
        else:
            L.call(entry + "_g", A_dev._op, B_dev._op, Binv_dev._op, Omega.handle, int(k), int(s), flags, L.ptr(d), U.handle)

    if isinstance(collective, NativeCollective):
        # the rank average runs inside the C solve on the context's stream (RCCL): no Python between the kernels
        code = {"sum": L.REDUCE_SUM, "avg": L.REDUCE_AVG}.get(str(mpi_op).lower())
        if code is None:
            raise NotImplementedError("reduction %r is not available (use 'sum' or 'avg')" % (mpi_op,))
        L.call("hfmi_op_set_collective", A_dev._op, collective._comm, code)
        try:
            run()
        finally:
            L.call("hfmi_op_set_collective", A_dev._op, None, 0)
    elif collective is not None and not isinstance(collective, NullCollective):
        hook = _PostApplyHook(A_dev, collective, mpi_op)
        with hook:
            try:
                run()
            except L.HfmiError:
                if hook.error is not None:
                    raise hook.error
                raise
    else:
        run()
    return d, U


def doublePass(A, Omega, k, s=1, check=False, sort_by_abs=False, use_mgs=False, fused=True, literal_T=False):
    """Randomized double pass for the dominant k eigenpairs of a Hermitian operator A.
    Omega: MultiVector with nvec >= k Gaussian probe vectors (not modified).
    ``literal_T=True`` forms T = (A Q)^T Q exactly as the reference does; by default the fused route forms the same
    matrix as scale (X Q)^T Gamma (X Q) for Gram-form operators (one fewer N x k product, k x k rank average).
    Up to ``WIDE_MAX_VECTORS`` = 2048 probe vectors.  Beyond 256 the fused route applies A in column panels of at most 256,
    always forms the literal T, and solves the Rayleigh-Ritz problem with the whole-GPU eigensolver."""
    nvec = Omega.nvec()
    assert nvec >= k
    A_dev, coll, mpi_op = _unwrap_collective(A)
    if fused and A_dev is not None:
        return _fused(A_dev, coll, mpi_op, None, None, Omega, k, s, sort_by_abs, use_mgs, literal_T)
    Q = MultiVector(Omega)
    Y = MultiVector(Omega.size(), nvec, ctx=Omega.ctx)
    for i in range(s):
        if i:
            Y.zero()          # block operators of the reference accumulate into y (activeSubspaceProjector.py:214-221)
        MatMvMult(A, Q, Y)
        Q.swap(Y)
    Q.orthogonalize(L.QR_MGS if use_mgs else L.QR_AUTO)
    AQ = MultiVector(Omega.size(), nvec, ctx=Omega.ctx)
    MatMvMult(A, Q, AQ)
    T = AQ.dot_mv(Q)
    d, V = sym_eig_small(T, sort_by_abs, Omega.ctx)
    d = d[:k].copy()
    U = MultiVector(Omega.size(), k, ctx=Omega.ctx)
    MvDSmatMult(Q, np.ascontiguousarray(V[:, :k]), U)
    return d, U


def _as_solver_operator(Binv, N, ctx, B=None):
    """B^-1 as an operator.  An object that is both the operator and its own solver (``prior.Hlr``: ``mult`` applies B,
    ``solve`` applies B^-1; activeSubspaceProjector.py:455-459) contributes its ``inverse()``.  A host solver whose
    vectors cannot be shaped from the solver itself borrows ``B.init_vector`` (hippylib wraps it the same way)."""
    if isinstance(Binv, DeviceOperator) and hasattr(Binv, "inverse"):
        return Binv.inverse()
    shaper = None
    if not isinstance(Binv, DeviceOperator) and H.find_init_vector(Binv) is None and B is not None:
        if not isinstance(B, DeviceOperator):
            shaper = H.find_init_vector(B)
        else:
            shaper = getattr(B, "_shaper", None)          # a host operator already wrapped: the init_vector it was wrapped with
    return as_device_operator(Binv, N, ctx, init_vector=shaper)


def doublePassG(A, B, Binv, Omega, k, s=1, check=False, sort_by_abs=False, use_mgs=False, fused=True, literal_T=False):
    """Randomized double pass for A u = lambda B u (B SPD), U^T B U = I.
    ``Binv`` is a solver object (``solve(y, x)``) as in the reference, or an operator.
    Up to 2048 probe vectors, as ``doublePass``; beyond 256, A, B and B^-1 are applied in column panels of at most 256."""
    nvec = Omega.nvec()
    assert nvec >= k
    N = Omega.size()
    A_dev, coll, mpi_op = _unwrap_collective(A)
    if fused and A_dev is not None:
        B_dev = as_device_operator(B, N, Omega.ctx)
        Binv_dev = _as_solver_operator(Binv, N, Omega.ctx, B)
        return _fused(A_dev, coll, mpi_op, B_dev, Binv_dev, Omega, k, s, sort_by_abs, use_mgs, literal_T)
    # B^{-1}: a device operator / solver as is; a host solver object (solve(y, x) on numpy arrays, like the
    # PETSc solvers of the reference) is reached through a host-callback operator
    Binv_op = _as_solver_operator(Binv, N, Omega.ctx, B)
    Ybar = MultiVector(N, nvec, ctx=Omega.ctx)
    Q = MultiVector(Omega)
    for i in range(s):
        if i:
            Ybar.zero()
        MatMvMult(A, Q, Ybar)
        MatMvMult(Binv_op, Ybar, Q)
    Q.Borthogonalize(B, L.QR_MGS if use_mgs else L.QR_AUTO)
    AQ = MultiVector(N, nvec, ctx=Omega.ctx)
    MatMvMult(A, Q, AQ)
    T = AQ.dot_mv(Q)
    d, V = sym_eig_small(T, sort_by_abs, Omega.ctx)
    d = d[:k].copy()
    U = MultiVector(N, k, ctx=Omega.ctx)
    MvDSmatMult(Q, np.ascontiguousarray(V[:, :k]), U)
    return d, U


def doublePassC(A, C, Omega, k, s=1, sort_by_abs=False, use_mgs=False):
    """``doublePassG(A, R, Rsolver, Omega, k, s)`` for a prior given by its COVARIANCE C = R^-1 alone: the same (d, U) and the encoder
    E = R U on top, with no R and no solve.  doublePassG builds Ybar = C A Omega, R-orthonormalises it to Q and forms T = Q^T A Q.
    Write Q = C Qv: Qv is the C-orthonormalisation of Yv = A Omega (Qv^T C Qv = I) and Q = C Qv is the ``BQ`` block that the
    B-orthogonalisation with B = C returns anyway.  So
        Yv = (A C)^(s-1) A Omega,  (Qv, BQ) = C-orth(Yv),  T = BQ^T A BQ,  eigh(T) descending, W = its k leading vectors,
        U = BQ W (decoder, U^T R U = I),  E = Qv W (encoder R U, E^T U = I).
    In exact arithmetic this is doublePassG's (d, U) for the same Omega.  A may be wrapped in a ``CollectiveOperator`` /
    ``MatrixMultCollectiveOperator`` as for doublePassG (the local device operator is applied, the block is all-reduced); C is an
    operator on every rank (``GridKernelCovarianceOperator``, or anything ``as_device_operator`` takes).  Returns (d, U, E)."""
    nvec = Omega.nvec()
    assert nvec >= k
    N = Omega.size()
    A_dev, coll, mpi_op = _unwrap_collective(A)

    def apply_A(X, Y):
        if A_dev is not None and coll is not None:
            A_dev.matMvMult(X, Y)
            coll.allReduce(Y, mpi_op)
        else:
            MatMvMult(A_dev if A_dev is not None else A, X, Y)

    C_dev = as_device_operator(C, N, Omega.ctx)
    Yv = MultiVector(N, nvec, ctx=Omega.ctx)
    apply_A(Omega, Yv)
    if s > 1:
        CY = MultiVector(N, nvec, ctx=Omega.ctx)
        for _ in range(s - 1):
            MatMvMult(C_dev, Yv, CY)
            apply_A(CY, Yv)
    BQ, _ = Yv.Borthogonalize(C_dev, L.QR_MGS if use_mgs else L.QR_AUTO)     # Yv becomes Qv
    ABQ = MultiVector(N, nvec, ctx=Omega.ctx)
    apply_A(BQ, ABQ)
    T = ABQ.dot_mv(BQ)
    d, V = sym_eig_small(T, sort_by_abs, Omega.ctx)
    W = np.ascontiguousarray(V[:, :k])
    U = MultiVector(N, k, ctx=Omega.ctx)
    E = MultiVector(N, k, ctx=Omega.ctx)
    MvDSmatMult(BQ, W, U)
    MvDSmatMult(Yv, W, E)
    return d[:k].copy(), U, E


def svd_small(R, ctx=None):
    """np.linalg.svd(R) of a small square matrix (k <= 256) on the device (one-sided Jacobi): R = U diag(s) V^T, s
    descending.  V is orthogonal always.  A column of U that belongs to an exactly zero singular value is zero (there is
    nothing to normalise, as ``orthogonalize`` leaves a zero column of Q); the other columns are orthonormal and
    (U * s) @ V.T reproduces R.  Singular values are relatively accurate where the data determine them (R = B D with a
    well-conditioned B).  The result does not depend on the scale of R: 2^e R gives the same U and V and 2^e s, bit for
    bit.  A non-finite entry raises HfmiError."""
    R = L.as_f64(R)
    k = R.shape[0]
    sv, U, V = np.empty(k), np.empty((k, k)), np.empty((k, k))
    L.call("hfmi_svd_small", (ctx or L.Context.default()).handle, L.ptr(R), k, L.ptr(sv), L.ptr(U), L.ptr(V))
    return U, sv, V


def accuracyEnhancedSVD(A, Omega, k, s=1, check=False):
    """hp.accuracyEnhancedSVD: randomized SVD A ~ U diag(d) V^T of a rectangular operator with ``mult`` /
    ``transpmult`` (or the block forms ``matMvMult`` / ``matMvTranspmult``) and ``init_vector(x, dim)``
    (call sites: activeSubspaceProjector.py:813-834,1026).  Omega lives in the domain.  Returns (U, d, V)."""
    from .multivector import MatMvTranspmult
    nvec = Omega.nvec()
    assert nvec >= k
    y_vec = Vector(ctx=Omega.ctx)
    A.init_vector(y_vec, 0)
    Z = MultiVector(Omega)
    Y = MultiVector(y_vec, nvec)
    MatMvMult(A, Omega, Y)
    for _ in range(s):
        MatMvTranspmult(A, Y, Z)
        MatMvMult(A, Z, Y)
    Q = MultiVector(Y)
    Q.orthogonalize()
    BT = MultiVector(Omega.size(), nvec, ctx=Omega.ctx)
    MatMvTranspmult(A, Q, BT)
    R = BT.orthogonalize()
    V_hat, d, U_hatT = svd_small(R, Omega.ctx)        # R = V_hat diag(d) U_hatT^T
    U = MultiVector(y_vec, k)
    MvDSmatMult(Q, np.ascontiguousarray(U_hatT[:, :k]), U)
    V = MultiVector(Omega.size(), k, ctx=Omega.ctx)
    MvDSmatMult(BT, np.ascontiguousarray(V_hat[:, :k]), V)
    return U, d[:k].copy(), V


# ---------------------------------------------------------------- single pass
# hp.singlePass / hp.singlePassG (hippylib randomizedEigensolver).  Omega (N x m, m >= k) is not modified.
#   X_0 = Omega,  X_i = A X_{i-1}  (generalized: Ybar = A X_{i-1}, X_i = B^-1 Ybar),  i = 1..s,  no orthogonalisation;
#   P = X_{s-1},  Y = X_s,  Q = orth(Y)  (generalized: Q, BQ = B-orth(Y), Q^T B Q = I)  -- the double pass's QR rule;
#   Wt = P^T Q (generalized: P^T BQ),  Zt = Y^T Q (generalized: Ybar^T Q),  both m x m;
#   Tt = Wt^-1 Zt,  T = (Tt + Tt^T) / 2,  eigh(T) sorted descending (by |d| with sort_by_abs), keep k:  d,  U = Q V[:, :k].
# (A ~ Q T Q^T gives Q^T Y = T Q^T P, i.e. Wt T^T = Zt; generalized: Q^T B Y = Q^T Ybar = T Q^T B P.)  A is applied s times
# (the double pass: s + 1).  Exact when rank(B^-1 A) = m; a singular Wt (rank-deficient sketch, e.g. dependent probe
# vectors) raises HfmiError where hippylib's np.linalg.solve raises LinAlgError.

def small_solve(W, Z, ctx=None):
    """np.linalg.solve(W, Z) for square m x m operands (m <= 256) on the device: one-workgroup LU with partial pivoting,
    the kernel behind the single-pass Rayleigh-Ritz matrix.  A singular W raises HfmiError."""
    W, Z = L.as_f64(W), L.as_f64(Z)
    m = W.shape[0]
    if W.shape != (m, m) or Z.shape != (m, m):
        raise ValueError("small_solve: W and Z must both be m x m (got %s and %s)" % (W.shape, Z.shape))
    X = np.empty((m, m))
    L.call("hfmi_small_solve", (ctx or L.Context.default()).handle, L.ptr(W), L.ptr(Z), m, L.ptr(X))
    return X


def _check_sketch_args(Omega, k, s):
    """the C entry points' argument checks, for the generic route (HFMI_ERR_INVALID = -1)"""
    if int(s) < 1:
        raise L.HfmiError(-1, "single_pass: s must be >= 1 (got %d)" % int(s))
    if not 1 <= int(k) <= Omega.nvec():
        raise L.HfmiError(-1, "single_pass: the rank must be in [1, %d] (the number of probe vectors), got %d" % (Omega.nvec(), int(k)))
    if Omega.nvec() > 256:
        raise L.HfmiError(-1, "single_pass: at most 256 probe vectors (got %d)" % Omega.nvec())


def _sketch_tail(P, Q, Wt, Zt, k, sort_by_abs, ctx):
    """The generic route's Rayleigh-Ritz step: T from the device LU solve, eigh, U = Q V[:, :k]."""
    Tt = small_solve(Wt, Zt, ctx)
    d, V = sym_eig_small(0.5 * (Tt + Tt.T), sort_by_abs, ctx)
    U = MultiVector(P.size(), k, ctx=ctx)
    MvDSmatMult(Q, np.ascontiguousarray(V[:, :k]), U)
    return d[:k].copy(), U


def singlePass(A, Omega, k, s=1, check=False, sort_by_abs=False, use_mgs=False, fused=True):
    """Randomized single pass for the dominant k eigenpairs of a Hermitian operator A (hp.singlePass): A is applied
    s times.  Omega: MultiVector with nvec >= k probe vectors (not modified).  Returns (d, U), U^T U = I."""
    nvec = Omega.nvec()
    _check_sketch_args(Omega, k, s)
    A_dev, coll, mpi_op = _unwrap_collective(A)
    if fused and A_dev is not None:
        return _fused(A_dev, coll, mpi_op, None, None, Omega, k, s, sort_by_abs, use_mgs, entry="hfmi_single_pass")
    P = MultiVector(Omega)
    Y = MultiVector(Omega.size(), nvec, ctx=Omega.ctx)
    for i in range(s):
        if i:
            P.swap(Y)
            Y.zero()          # block operators of the reference accumulate into y
        MatMvMult(A, P, Y)
    Q = MultiVector(Y)
    Q.orthogonalize(L.QR_MGS if use_mgs else L.QR_AUTO)
    return _sketch_tail(P, Q, P.dot_mv(Q), Y.dot_mv(Q), k, sort_by_abs, Omega.ctx)


def singlePassG(A, B, Binv, Omega, k, s=1, check=False, sort_by_abs=False, use_mgs=False, fused=True):
    """Randomized single pass for A u = lambda B u (B SPD; hp.singlePassG): A and B^-1 are applied s times each.
    ``Binv`` is a solver object (``solve(y, x)``) as in the reference, or an operator.  Returns (d, U), U^T B U = I."""
    nvec = Omega.nvec()
    _check_sketch_args(Omega, k, s)
    N = Omega.size()
    A_dev, coll, mpi_op = _unwrap_collective(A)
    if fused and A_dev is not None:
        B_dev = as_device_operator(B, N, Omega.ctx)
        Binv_dev = _as_solver_operator(Binv, N, Omega.ctx, B)
        return _fused(A_dev, coll, mpi_op, B_dev, Binv_dev, Omega, k, s, sort_by_abs, use_mgs, entry="hfmi_single_pass")
    Binv_op = _as_solver_operator(Binv, N, Omega.ctx, B)
    P = MultiVector(Omega)
    Ybar = MultiVector(N, nvec, ctx=Omega.ctx)
    Y = MultiVector(N, nvec, ctx=Omega.ctx)
    for i in range(s):
        if i:
            P.swap(Y)
            Ybar.zero()
        MatMvMult(A, P, Ybar)
        MatMvMult(Binv_op, Ybar, Y)
    BQ, _ = Y.Borthogonalize(B, L.QR_MGS if use_mgs else L.QR_AUTO)      # Y becomes Q
    return _sketch_tail(P, Y, P.dot_mv(BQ), Ybar.dot_mv(Y), k, sort_by_abs, Omega.ctx)


class StreamedSketch:
    """The single-pass sketch Y = A Omega summed while the samples are produced, one batch at a time, and never stored.

    ``kind="snapshots"``: ``add(X_b)`` with a (b, N) block of snapshots adds X_b^T (X_b Omega) -- A is the snapshot Gram
    operator (1/n) sum_i x_i x_i^T (PODProjector);  ``kind="jacobian"``: ``add(J)`` with one (q, N) Jacobian adds
    J^T Gamma^-1 J Omega -- A is the mean J^T Gamma^-1 J (active subspace), ``noise_cov_inv`` the q x q Gamma^-1 (None:
    identity).  Batch sizes may vary.  Each batch is copied into one of two pinned buffers and uploaded on the ingest
    stream while the producer makes the next one; the product is accumulated on the device by the snapshot-Gram / J^T J
    kernels.  Nothing waits for the GPU except the reuse of a pinned buffer.  The scale is 1 / (number of samples over all
    ranks); with a ``collective`` the sketch and the count are all-reduced once, at the end.  Device memory: Omega, Y,
    the Q / BQ work blocks of the solve and two batch buffers, O(N (3 m + 2 b)), whatever the number of samples.

    ``singlePass(k)`` / ``singlePassG(k, B, Binv)`` return (d, U) from the finished sketch (hfmi_sketch_eig)."""

    def __init__(self, Omega, kind="snapshots", noise_cov_inv=None, collective=None):
        if kind not in ("snapshots", "jacobian"):
            raise ValueError("StreamedSketch: kind must be 'snapshots' or 'jacobian'")
        self.Omega = Omega
        self.ctx = Omega.ctx
        self.N, self.m = Omega.size(), Omega.nvec()
        self.kind = kind
        self.collective = collective
        self.noise_cov_inv = None if noise_cov_inv is None else L.as_f64(np.asarray(noise_cov_inv, dtype=np.float64))
        self.q = None if self.noise_cov_inv is None else self.noise_cov_inv.shape[0]
        if self.noise_cov_inv is not None and self.noise_cov_inv.shape != (self.q, self.q):
            raise ValueError("StreamedSketch: noise_cov_inv must be square")
        self._Y = MultiVector(self.N, self.m, ctx=self.ctx)
        self._Y.zero()
        self._count = 0
        self._final = None
        self._pinned = [None, None]
        self._dev = [None, None]
        self._tickets = [None, None]
        self._ops = [{}, {}]       # batch rows -> (view, operator) over device buffer i (operators keep their own state)
        self._nbatch = 0

    @property
    def count(self):
        """samples added on this rank"""
        return self._count

    def add(self, batch):
        if self._final is not None:
            raise RuntimeError("StreamedSketch.add: the sketch has been finished (singlePass / sketch was called)")
        arr = np.asarray(batch, dtype=np.float64)
        if arr.ndim == 1 and self.kind == "snapshots":
            arr = arr.reshape(1, -1)
        if arr.ndim != 2 or arr.shape[1] != self.N or arr.shape[0] < 1:
            raise ValueError("StreamedSketch.add: a (rows, %d) array expected, got shape %s" % (self.N, arr.shape))
        b = arr.shape[0]
        if self.kind == "jacobian":
            if self.q is None:
                self.q = b
            elif b != self.q:
                raise ValueError("StreamedSketch.add: a Jacobian of %d rows expected, got %d" % (self.q, b))
        i = self._nbatch % 2
        if self._tickets[i] is not None:
            self.ctx.ingest_wait(self._tickets[i])
            self._tickets[i] = None
        if self._pinned[i] is None or self._pinned[i].shape[0] < b:
            cap = max(b, 0 if self._pinned[i] is None else self._pinned[i].shape[0])
            self._pinned[i] = L.pinned_empty((cap, self.N))
            self._dev[i] = MultiVector(self.N, cap, ctx=self.ctx)
            self._ops[i] = {}
        rows = self._pinned[i][:b]
        np.copyto(rows, arr)
        entry = self._ops[i].get(b)
        if entry is None:
            view = self._dev[i].view(0, b)
            if self.kind == "snapshots":
                from .operators import SnapshotGramOperator
                op = SnapshotGramOperator(view, scale=1.0)
            else:
                from .operators import MeanJTJfromDataOperator
                op = MeanJTJfromDataOperator.from_block(view, 1, b, noise_cov_inv=self.noise_cov_inv, scale=1.0)
            entry = self._ops[i][b] = (view, op)
        view, op = entry
        self._tickets[i] = view.upload_async(rows)
        self.ctx.ingest_fence()
        op.matMvMult(self.Omega, self._Y, accumulate=True)
        self._count += b if self.kind == "snapshots" else 1
        self._nbatch += 1

    def _finish(self):
        if self._final is None:
            total = self._count
            if self.collective is not None:
                self.collective.allReduce(self._Y, "sum")
                total = int(round(self.collective.allReduce(float(self._count), "sum")))
            if total < 1:
                raise ValueError("StreamedSketch: no samples were added")
            self._Y.scale(1.0 / total)
            for t in self._tickets:
                if t is not None:
                    self.ctx.ingest_wait(t)
            self._tickets = [None, None]
            self._final = total
        return self._Y

    def sketch(self):
        """The finished sketch A Omega (MultiVector, N x m; finishes the sketch)."""
        return self._finish()

    def singlePass(self, k, sort_by_abs=False, use_mgs=False):
        Y = self._finish()
        if not 1 <= k <= self.m:
            raise L.HfmiError(-1, "StreamedSketch.singlePass: k must be in [1, %d] (got %d)" % (self.m, k))
        d = np.empty(k)
        U = MultiVector(self.N, k, ctx=self.ctx)
        flags = (1 if sort_by_abs else 0) | (2 if use_mgs else 0)
        L.call("hfmi_sketch_eig", self.Omega.handle, Y.handle, None, None, int(k), flags, L.ptr(d), U.handle)
        return d, U

    def singlePassG(self, k, B, Binv, sort_by_abs=False, use_mgs=False):
        Ybar = self._finish()
        if not 1 <= k <= self.m:
            raise L.HfmiError(-1, "StreamedSketch.singlePassG: k must be in [1, %d] (got %d)" % (self.m, k))
        B_dev = as_device_operator(B, self.N, self.ctx)
        Binv_dev = _as_solver_operator(Binv, self.N, self.ctx, B)
        Y = MultiVector(self.N, self.m, ctx=self.ctx)
        Binv_dev.matMvMult(Ybar, Y)
        d = np.empty(k)
        U = MultiVector(self.N, k, ctx=self.ctx)
        flags = (1 if sort_by_abs else 0) | (2 if use_mgs else 0)
        L.call("hfmi_sketch_eig", self.Omega.handle, Y.handle, Ybar.handle, B_dev._op, int(k), flags, L.ptr(d), U.handle)
        return d, U
