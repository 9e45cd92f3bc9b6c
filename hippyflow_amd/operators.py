"""Linear operators behind the reference's duck-typed protocol
(``mult(x, y)``, optional ``matMvMult(X, Y)``, ``init_vector(x, dim)``),
each backed by an ``hfmi_op`` (include/hfmi.h) so that its block application is a
HIP kernel sequence on the GPU.

Reference counterparts (file:line under /root/reference/hippyflow):

* ``LowRankOperator`` / ``SnapshotGramOperator``  hp.LowRankOperator(ones/n, snapshots)      modeling/PODProjector.py:359-361
* ``MeanJTJfromDataOperator``                     modeling/operatorWrappers.py:55-121
* ``MeanJJTfromDataOperator``                     JJT summed/averaged: modeling/jacobian.py:169-193, activeSubspaceProjector.py:640-645
* ``npToDeviceOperator``                          npToDolfinOperator, modeling/operatorWrappers.py:19-52 (symmetric case)
* ``KernelCovarianceOperator``                    the same role for a kernel covariance given by node coordinates, never assembled
* ``GridKernelCovarianceOperator``                that covariance on the nodes of a regular grid, applied by FFT (hfmi_fftcov.hip)
* ``GridCovarianceFactor`` / ``GridKernelPrior``  its factor C = S S^T (hfmi_op_grid_factor) and the prior protocol over it: ``sample(noise, m)``
                                                  with the caller's noise, ``Rsolver``, no ``R`` (``randomized.doublePassC`` needs none)
* ``InterpolatedCovarianceFactor`` / ``InterpolatedKernelPrior``  the same two over SCATTERED points (mesh nodes): the factor K = F F^T,
                                                  F = [W S | diag(sqrt(delta))] (hfmi_op_interp_factor), of the interpolated grid covariance
* ``BoxSpectralCovariance`` / ``BoxSpectralPrior``  the Whittle-Matern prior on a box by DCT / FFT (hfmi_op_box): C, R = C^-1 and both roots
                                                  exact, the full prior protocol (hippylib BiLaplacianPrior on a tensor grid, lumped mass)
* ``KernelCrossCovarianceOperator``               K(T, S) between two point sets (Nystrom extension); ``KernelCovarianceOperator.rows`` /
                                                  ``.sharded``: a row slab of C per rank, completed by the collective's SUM
* ``CsrOperator`` / ``CsrPCGSolver``              prior.M / prior.R and prior.Msolver (used at KLEProjector.py:163-168)
* ``CsrAMGSolver`` / ``BiLaplacianRsolver``       hippylib BiLaplacianPrior.Asolver (CG + AMG) and prior.Rsolver = A^-1 M A^-1
                                                  (activeSubspaceProjector.py:447-453, KLEProjector.py:163-168)
* ``Solver2Operator``                             hp.Solver2Operator, modeling/KLEProjector.py:103,176
* ``MassPreconditionedCovarianceOperator``        modeling/KLEProjector.py:47-69
* ``SummedListOperator``                          modeling/activeSubspaceProjector.py:69-95
* ``HostCallbackOperator``                        any host black box (FEniCS Jacobian actions, sparse LU):
                                                  the role of ObservableJacobian/JTJ, modeling/jacobian.py:62-166
* ``PriorPreconditionedProjector``                modeling/priorPreconditionedProjector.py:19-55
* ``LowRankRectangularOperator``                  modeling/lowRankRectangularOperator.py:17-66
"""
import ctypes as C

import numpy as np

from . import _lib as L
from . import hostvec as H
from .multivector import MultiVector, Vector


class DeviceOperator:
    """Base: owns an hfmi_op handle.  ``matMvMult`` overwrites Y unless ``accumulate=True``
    (the reference's block operators accumulate into a zero-filled Y,
    activeSubspaceProjector.py:219-221; overwrite is the intended behaviour)."""

    def __init__(self, ctx, n_range, n_domain=None):
        self.ctx = ctx or L.Context.default()
        self._op = C.c_void_p()
        self._shape = (int(n_range), int(n_range if n_domain is None else n_domain))
        self._keep = []   # python objects the C side points into

    @property
    def shape(self):
        return self._shape

    def mpi_comm(self):
        from .multivector import _NullComm
        return _NullComm()

    def init_vector(self, x, dim=0):
        """dim 0: range, dim 1: domain (jacobian.py:96-115)."""
        if dim not in (0, 1):
            raise ValueError("dim must be 0 or 1")
        x.init(self._shape[dim])

    def matMvMult(self, X, Y, accumulate=False):
        assert X.nvec() == Y.nvec(), "x and y have non-matching number of vectors"
        L.call("hfmi_op_apply", self._op, X.handle, Y.handle, 1 if accumulate else 0)

    def mult(self, x, y):
        L.call("hfmi_op_apply", self._op, x._mv.handle, y._mv.handle, 0)

    def transpmult(self, x, y):   # every operator on this path is self-adjoint
        self.mult(x, y)

    def __del__(self):
        try:
            if getattr(self, "_op", None):
                L.load().hfmi_op_destroy(self._op)
                self._op = None
        except Exception:
            pass


class SnapshotGramOperator(DeviceOperator):
    """y = scale * X X^T x with X the block of snapshots (one vector per snapshot);
    ``scale = 1/n`` reproduces hp.LowRankOperator(ones/n, LocalObservables) (PODProjector.py:359-361)."""

    def __init__(self, snapshots, scale=None, ctx=None):
        if not isinstance(snapshots, MultiVector):
            snapshots = MultiVector.from_vectors(snapshots, ctx=ctx)
        super().__init__(ctx or snapshots.ctx, snapshots.size())
        self.snapshots = snapshots
        self.scale = 1.0 / snapshots.nvec() if scale is None else float(scale)
        L.call("hfmi_op_snapshot_gram", self.ctx.handle, snapshots.handle, self.scale, C.byref(self._op))


class LowRankOperator(DeviceOperator):
    """hp.LowRankOperator(d, U, init_vector): ``mult`` y = U diag(d) U^T x (``dot_v`` + ``reduce`` in hippylib, two
    contractions with a row scaling between them here) and ``solve(y, x)`` y = U diag(1/d) U^T x -- the object hippylib's
    priors expose as ``prior.Hlr`` and hippyflow passes as both B and B^-1 (activeSubspaceProjector.py:455-459).  The
    constant diagonal ``ones/n`` of PODProjector.py:359-361 is the snapshot-Gram operator."""

    def __init__(self, d, U, init_vector=None, ctx=None):
        if not isinstance(U, MultiVector):
            U = MultiVector.from_vectors(U, ctx=ctx)
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(d, dtype=np.float64), (U.nvec(),)))
        super().__init__(ctx or U.ctx, U.size())
        self.U, self.d = U, d
        self._init_vector = init_vector
        self._inverse = None
        L.call("hfmi_op_low_rank", self.ctx.handle, U.handle, L.ptr(d), C.byref(self._op))

    def init_vector(self, x, dim=0):
        if self._init_vector is not None:
            return self._init_vector(x, dim)
        return DeviceOperator.init_vector(self, x, dim)

    def inverse(self):
        """U diag(1/d) U^T as an operator (what ``solve`` applies)."""
        if self._inverse is None:
            if np.any(self.d == 0.0):
                raise ZeroDivisionError("LowRankOperator.solve: zero entry in d")
            self._inverse = LowRankOperator(1.0 / self.d, self.U, self._init_vector)
        return self._inverse

    def solve(self, y, x):
        self.inverse().mult(x, y)


class MeanJTJfromDataOperator(DeviceOperator):
    """y = mean_i J_i^T Gamma^{-1} J_i x from a stored (ndata, q, dM) Jacobian array
    (operatorWrappers.py:55-121).  ``scale`` defaults to 1/ndata (the np.mean at :114); pass
    ``scale=1/(ndata*P)`` style values to pre-fold a rank average."""

    def __init__(self, J, prior=None, noise_cov_inv=None, scale=None, ctx=None):
        if isinstance(J, MultiVector):
            raise TypeError("pass (J_block, ndata, q) through MeanJTJfromDataOperator.from_block")
        J = np.asarray(J, dtype=np.float64)
        assert J.ndim == 3, "J.shape must be (ndata, rank, dM)"
        ndata, q, dM = J.shape
        block = MultiVector.from_vectors(J.reshape(ndata * q, dM), ctx=ctx)
        self._setup(block, ndata, q, noise_cov_inv, scale, prior, ctx)

    @classmethod
    def from_block(cls, J_block, ndata, q, noise_cov_inv=None, scale=None, prior=None):
        self = cls.__new__(cls)
        self._setup(J_block, ndata, q, noise_cov_inv, scale, prior, J_block.ctx)
        return self

    def _setup(self, block, ndata, q, noise_cov_inv, scale, prior, ctx):
        DeviceOperator.__init__(self, ctx or block.ctx, block.size())
        self._J, self.ndata, self.r, self.dM = block, int(ndata), int(q), block.size()
        self._prior = prior
        self._noise_cov_inv = None
        gptr = None
        if noise_cov_inv is not None:
            assert hasattr(noise_cov_inv, "__matmul__")
            self._noise_cov_inv = L.as_f64(np.asarray(noise_cov_inv, dtype=np.float64))
            assert self._noise_cov_inv.shape == (q, q)
            gptr = L.ptr(self._noise_cov_inv)
        self.scale = 1.0 / ndata if scale is None else float(scale)
        L.call("hfmi_op_jtj", self.ctx.handle, block.handle, int(ndata), int(q), gptr, self.scale, C.byref(self._op))

    @property
    def J(self):
        return self._J

    @property
    def prior(self):
        return self._prior

    @property
    def noise_cov_inv(self):
        return self._noise_cov_inv


class MeanJJTfromDataOperator(DeviceOperator):
    """Output-space counterpart y = mean_i J_i J_i^T x (acts on vectors of length q)."""

    def __init__(self, J, scale=None, ctx=None):
        if isinstance(J, tuple):
            block, ndata, q = J
        else:
            J = np.asarray(J, dtype=np.float64)
            ndata, q, dM = J.shape
            block = MultiVector.from_vectors(J.reshape(ndata * q, dM), ctx=ctx)
        super().__init__(ctx or block.ctx, q)
        self._J, self.ndata, self.r = block, int(ndata), int(q)
        self.scale = 1.0 / ndata if scale is None else float(scale)
        L.call("hfmi_op_jjt", self.ctx.handle, block.handle, int(ndata), int(q), self.scale, C.byref(self._op))


class npToDeviceOperator(DeviceOperator):
    """Dense SYMMETRIC matrix behind the protocol (npToDolfinOperator, operatorWrappers.py:19-52, for the
    self-adjoint operators of this path; config 2's explicit covariance)."""

    def __init__(self, npArray, ctx=None):
        if isinstance(npArray, MultiVector):
            block = npArray
        else:
            npArray = np.asarray(npArray, dtype=np.float64)
            assert len(npArray.shape) == 2 and npArray.shape[0] == npArray.shape[1]
            block = MultiVector.from_vectors(npArray, ctx=ctx)      # symmetric: rows == columns
        super().__init__(ctx or block.ctx, block.size())
        self.matrix = block
        L.call("hfmi_op_dense_sym", self.ctx.handle, block.handle, C.byref(self._op))


def _points_array(points):
    """(N, d) C-ordered float64 array of node coordinates (a 1-D array is N points on a line)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts[:, None]
    if pts.ndim != 2:
        raise ValueError("points must be an (N, d) array, got shape %r" % (pts.shape,))
    return L.as_f64(pts)


def _unknown_family(family):
    return ValueError("unknown kernel family %r (one of %s)" % (family, ", ".join(sorted(L.KERNEL_FAMILIES))))


def _check_metric(metric, d):
    """None, or the metric as a (d, d) float64 array after the checks of hfmi_kernel_metric_factor: finite, symmetric to 4 eps max|G|,
    positive definite.  A scalar is a 1 x 1 metric."""
    if metric is None:
        return None
    G = np.array(metric, dtype=np.float64)
    if G.ndim == 0:
        G = G.reshape(1, 1)
    if G.shape != (d, d):
        raise ValueError("metric: a symmetric positive definite %d x %d matrix is required, got shape %r" % (d, d, G.shape))
    if not np.all(np.isfinite(G)):
        raise ValueError("metric: every entry must be finite")
    if np.max(np.abs(G - G.T)) > 4.0 * np.finfo(np.float64).eps * np.max(np.abs(G)):
        raise ValueError("metric: not symmetric")
    try:
        np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        raise ValueError("metric: not positive definite") from None
    return np.ascontiguousarray(G)


def _metric_points(pts, G):
    """``pts @ L`` with G = L L^T: the coordinates in which the metric is the identity (``pts`` itself without a metric)"""
    return pts if G is None else np.ascontiguousarray(pts @ np.linalg.cholesky(G))


def _kernel_spec(family, d, sigma, ell, nugget, G, nu=None):
    """The hfmi_kernel_spec of a kernel: what Matern-1 and every kernel with a metric are created from.  With ``nu`` (family
    "matern") it is the hfmi_kernel_spec2 that the ``_spec2`` creators take."""
    if nu is None:
        spec = L.KernelSpec(L.KERNEL_FAMILIES[family], int(d), float(sigma), float(ell), float(nugget))
    else:
        spec = L.KernelSpec2(L.KERNEL_FAMILIES[family], int(d), float(sigma), float(ell), float(nugget))
        spec.nu = float(nu)
    if G is not None:
        for i, v in enumerate(G.ravel()):
            spec.metric[i] = v
    return spec


def _check_nu(family, nu):
    """The smoothness of a kernel as a float, None for every family but "matern": ``family="matern"`` needs ``nu`` in
    [MATERN_NU_MIN, MATERN_NU_MAX] = [1/8, 8]; every other family refuses one."""
    if family == "matern":
        if nu is None:
            raise ValueError('family="matern" needs its smoothness nu (1/8 <= nu <= 8)')
        nu = float(nu)
        if not (np.isfinite(nu) and L.MATERN_NU_MIN <= nu <= L.MATERN_NU_MAX):
            raise ValueError("nu = %r does not lie in [%g, %g]" % (nu, L.MATERN_NU_MIN, L.MATERN_NU_MAX))
        return nu
    if nu is not None:
        raise ValueError('nu is the smoothness of family="matern"; family %r has none' % (family,))
    return None


def _spec_suffix(nu):
    """the creators a kernel goes through: ``_spec2`` with a smoothness, ``_spec`` otherwise"""
    return "_spec" if nu is None else "_spec2"


def _kernel_phi(family, dist, ell, nu=None):
    """phi(dist / ell) of ``kernel_cov_host`` for an array of distances"""
    if family == "matern":
        # 2^(1-nu) / Gamma(nu) a^nu K_nu(a) through scipy's scaled K_nu: independent of the device's arithmetic
        from scipy.special import gamma, kve
        a = np.sqrt(2.0 * nu) * dist / ell
        with np.errstate(invalid="ignore", under="ignore", divide="ignore", over="ignore"):
            v = ((2.0 ** (1.0 - nu) / gamma(nu)) * a ** nu) * kve(nu, a) * np.exp(-a)
            # a^nu K_nu(a) is 0 * inf for a tiny a (phi is 1 there to rounding) and inf * 0 for a huge one (phi is 0)
            return np.where(a > 0.0, np.where(np.isfinite(v), v, np.where(a < 1.0, 1.0, 0.0)), 1.0)
    if family == "matern12":
        return np.exp(-dist / ell)
    if family == "matern32":
        a = np.sqrt(3.0) * dist / ell
        return (1.0 + a) * np.exp(-a)
    if family == "matern52":
        a = np.sqrt(5.0) * dist / ell
        return (1.0 + a + a * a / 3.0) * np.exp(-a)
    if family == "matern1":
        from scipy.special import k1e
        a = np.sqrt(2.0) * dist / ell
        with np.errstate(invalid="ignore", under="ignore"):
            return np.where(a > 0.0, a * k1e(a) * np.exp(-a), 1.0)
    return np.exp(-0.5 * (dist / ell) ** 2)


def kernel_cov_host(points, family, sigma, ell, nugget=0.0, rows=None, *, nu=None, metric=None):
    """Dense host evaluation of the covariance ``KernelCovarianceOperator`` applies: C_ij = sigma^2 phi(|x_i - x_j| / ell)
    + nugget delta_ij (the delta is on the point INDEX), all rows or the rows ``rows``.  With r the scaled distance:
    'matern12' exp(-r); 'matern32' (1 + a) exp(-a), a = sqrt(3) r; 'matern52' (1 + a + a^2/3) exp(-a), a = sqrt(5) r;
    'sqexp' exp(-r^2 / 2); 'matern1' a K_1(a), a = sqrt(2) r (1 at r = 0; ``scipy.special.k1e``).  ``metric``: a symmetric positive
    definite d x d matrix G, r = sqrt(delta^T G delta) / ell, evaluated as the isotropic kernel on ``points @ L``, G = L L^T; None is
    the identity.  'matern' with ``nu`` (keyword only, 1/8 <= nu <= 8): the Matern correlation of any smoothness,
    2^(1-nu) / Gamma(nu) a^nu K_nu(a), a = sqrt(2 nu) r, by ``scipy.special.kve`` -- not the device's arithmetic, so this stays an
    independent reference.  nu = 1/2, 3/2, 5/2 and 1 are 'matern12', 'matern32', 'matern52' and 'matern1' to rounding; the named
    families are the fast ones on the device and nothing dispatches to them.  What tests and users compare the device operator against."""
    if family not in L.KERNEL_FAMILIES:
        raise _unknown_family(family)
    nu = _check_nu(family, nu)
    pts = _points_array(points)
    pts = _metric_points(pts, _check_metric(metric, pts.shape[1]))
    r = np.arange(pts.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    d2 = np.zeros((len(r), pts.shape[0]))
    for c in range(pts.shape[1]):
        d2 += (pts[r, c][:, None] - pts[None, :, c]) ** 2
    C = sigma ** 2 * _kernel_phi(family, np.sqrt(d2), ell, nu)
    if nugget:
        C[np.arange(len(r)), r] += nugget
    return C


class KernelCovarianceOperator(DeviceOperator):
    """Kernel covariance over scattered points WITHOUT the N x N matrix: y = C x with C_ij = sigma^2 phi(|x_i - x_j| / ell)
    + nugget delta_ij, its entries evaluated inside the apply (hfmi_kcov.hip) and fed to the fp64 matrix cores.  ``points`` are
    the (N, d) node coordinates of the parameter's mesh or point cloud, d = 1, 2 or 3; ``family`` as in ``kernel_cov_host``.
    A drop-in ``prior.C`` for ``KLEProjector`` (and any place an explicit covariance went through ``npToDeviceOperator``):
    memory is 8 N d bytes, so N is bounded by time (2 N^2 k flops per apply), not by HBM.

    ``family="matern1"`` is a K_1(a), the kernel of the BiLaplacian prior in two dimensions (``bilaplacian_kernel_2d``); its entries
    cost several times those of the other families, so its apply is bound by their evaluation.  ``metric``: a symmetric positive
    definite d x d matrix G, distances are sqrt(delta^T G delta) (None: the identity).  The library is handed L^T x, G = L L^T, and
    runs the isotropic kernels; ``.points`` stays the caller's coordinates and ``.metric`` goes to every operator derived from this
    one.  One of the four other families without a metric is created exactly as before.

    ``family="matern"`` with ``nu`` (keyword only, 1/8 <= nu <= 8) is the Matern correlation of any smoothness,
    2^(1-nu) / Gamma(nu) a^nu K_nu(a), a = sqrt(2 nu) r / ell: the kernel of (delta - gamma div Theta grad)^alpha in d dimensions has
    nu = alpha - d/2 (``whittle_matern_kernel``).  K_nu is evaluated on the device from tables computed once at creation; an entry
    costs 2.3 times a Matern-1 entry (measured at nu = 1.25).  There is no silent dispatch: ``nu=1.5`` runs this general evaluation
    and agrees with ``"matern32"`` to rounding -- the named families stay the fast ones.  ``.nu`` goes to every operator derived from
    this one."""

    def __init__(self, points, family="matern32", sigma=1.0, ell=0.1, nugget=0.0, ctx=None, *, nu=None, metric=None):
        if family not in L.KERNEL_FAMILIES:
            raise _unknown_family(family)
        nu = _check_nu(family, nu)
        pts = _points_array(points)
        G = _check_metric(metric, pts.shape[1])
        super().__init__(ctx, pts.shape[0])
        self.family, self.sigma, self.ell, self.nugget = family, float(sigma), float(ell), float(nugget)
        self.points, self.metric, self.nu = pts, G, nu
        if family == "matern1" or G is not None or nu is not None:
            spec = _kernel_spec(family, pts.shape[1], self.sigma, self.ell, self.nugget, G, nu)
            L.call("hfmi_op_kernel_cov" + _spec_suffix(nu), self.ctx.handle, L.ptr(pts), pts.shape[0], pts.shape[1], C.byref(spec), C.byref(self._op))
        else:
            L.call("hfmi_op_kernel_cov", self.ctx.handle, L.ptr(pts), pts.shape[0], pts.shape[1], L.KERNEL_FAMILIES[family],
                   self.sigma, self.ell, self.nugget, C.byref(self._op))

    def to_dense(self, rows=None):
        """The same matrix on the host (``kernel_cov_host``): for checks at sizes where it fits."""
        return kernel_cov_host(self.points, self.family, self.sigma, self.ell, self.nugget, rows=rows, nu=self.nu, metric=self.metric)

    def rows(self, row0, row1):
        """Rows ``row0 .. row1 - 1`` of this operator as an operator N -> N (``KernelCovarianceRowsOperator``)."""
        return KernelCovarianceRowsOperator(self.points, self.family, self.sigma, self.ell, self.nugget, row0, row1, ctx=self.ctx,
                                            nu=self.nu, metric=self.metric)

    def sharded(self, collective):
        """An operator N -> N that equals C on every rank of ``collective``: this rank's row slab (``shard_rows``) with the collective's
        SUM attached for the object's lifetime -- a ``NativeCollective`` through ``hfmi_op_set_collective`` (the all-reduce is enqueued by
        the C apply itself), any other collective as a post-apply hook; ``NullCollective`` or one rank attaches nothing.  Each rank
        does 2 N^2 k / size flops; the slabs' rows are the bits of the full apply and the other rows are zeros, so the result is the
        full apply bit for bit.  Use it wherever C goes (doublePass, MassPreconditionedCovarianceOperator, singlePass,
        StreamedSketch); accumulating into it is the library's "ambiguous" error."""
        size, rank = int(collective.size()), int(collective.rank())
        op = self.rows(*shard_rows(self.shape[0], size, rank))
        if size > 1 and not _is_null_collective(collective):
            op._attach_sum(collective)
        return op


def _check_grid(shape, spacing, nodes, origin, family, ell, nugget, max_nodes=None):
    """The argument rules of hfmi_op_kernel_cov_grid that need no device; returns (shape, spacing, nodes or None, origin) as arrays.
    ``max_nodes``: nodes per axis, ``GRID_COV_MAX_NODES`` unless given (the long route's ``GRID_COV_LONG_MAX_NODES``)."""
    max_nodes = L.GRID_COV_MAX_NODES if max_nodes is None else int(max_nodes)
    if family not in L.KERNEL_FAMILIES:
        raise _unknown_family(family)
    n = np.atleast_1d(np.asarray(shape, dtype=np.int64))
    if n.ndim != 1 or not 1 <= n.size <= 3:
        raise ValueError("a grid has 1, 2 or 3 axes, got shape %r" % (shape,))
    if n.min() < 1 or n.max() > max_nodes:
        raise ValueError("every axis of the grid has 1 .. %d nodes, got %r" % (max_nodes, tuple(int(v) for v in n)))
    h = np.asarray(spacing, dtype=np.float64)
    h = np.full(n.size, float(h)) if h.ndim == 0 else h
    if h.shape != n.shape or not np.all(np.isfinite(h)) or not np.all(h > 0.0):
        raise ValueError("spacing: one positive finite number per axis, got %r" % (spacing,))
    o = np.zeros(n.size) if origin is None else np.asarray(origin, dtype=np.float64)
    if o.shape != n.shape or not np.all(np.isfinite(o)):
        raise ValueError("origin: one finite number per axis, got %r" % (origin,))
    total = int(np.prod(n))
    if nodes is not None:
        nodes = np.ascontiguousarray(np.asarray(nodes, dtype=np.int64))
        if nodes.ndim != 1 or nodes.size < 1:
            raise ValueError("nodes: a non-empty 1-D array of grid node indices")
        if nodes.min() < 0 or nodes.max() >= total:
            raise ValueError("nodes must lie in 0 .. %d" % (total - 1))
        if np.unique(nodes).size != nodes.size:
            raise ValueError("nodes must be distinct")
    if not float(ell) > 0.0:
        raise ValueError("the correlation length must be positive")
    if not float(nugget) >= 0.0:
        raise ValueError("the nugget must not be negative")
    return np.ascontiguousarray(n), np.ascontiguousarray(h), nodes, o


def grid_node_points(shape, spacing, nodes=None, origin=None):
    """(N, d) coordinates ``origin + index * spacing`` of grid nodes, axis 0 fastest: node g = i0 + n0 (i1 + n1 i2)."""
    n = np.atleast_1d(np.asarray(shape, dtype=np.int64))
    g = np.arange(int(np.prod(n)), dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
    h = np.broadcast_to(np.asarray(spacing, dtype=np.float64), n.shape)
    o = np.zeros(n.size) if origin is None else np.asarray(origin, dtype=np.float64)
    pts = np.empty((g.size, n.size))
    for c in range(n.size):
        pts[:, c] = o[c] + (g % n[c]) * h[c]
        g = g // n[c]
    return pts


class GridKernelCovarianceOperator(DeviceOperator):
    """The kernel covariance of ``KernelCovarianceOperator`` over nodes of a REGULAR grid, applied by FFT (hfmi_fftcov.hip): the matrix is
    block-Toeplitz with Toeplitz blocks, its circulant embedding is diagonalised by the FFT, and y = C x costs a few streaming passes
    over the padded grid per pair of vectors instead of 2 N^2 flops per vector -- the same C x up to rounding, not an approximation.
    ``shape``: nodes per axis (1, 2 or 3 axes of at most 2048 nodes, axis 0 fastest: node g = i0 + n0 (i1 + n1 i2), the numbering of
    ``workloads.grid_points``); ``spacing``: a number or one per axis; ``nodes``: the grid node of every point (distinct, any order;
    None = all nodes in order); ``origin``: coordinates of node 0 (only ``.points`` sees it).  ``.shape`` is the operator's (N, N) as
    for every ``DeviceOperator``; the grid is ``.grid_shape``.  Two vectors ride one complex transform, so a column's result depends
    on its partner in the last bits; two applies of the same block are bit-identical.  ``matrix_free()`` is the
    ``KernelCovarianceOperator`` over the same points (what ``pivoted_cholesky`` takes).

    ``sampler(max_growth=3, on_indefinite="raise" | "clip", seed=0)`` returns a ``GridFieldSampler``: exact draws m ~ N(0, C) by
    circulant embedding, d passes per pair of draws with the noise generated on the device, on an embedding grown until its spectrum
    is non-negative (or clipped, with a reported bound on the covariance error).  It is the draw to use on a grid, above all for rough
    kernels, short correlation lengths and large grids; ``PivotedCholesky.sample`` (of ``matrix_free()``) draws from L L^T instead and is
    the one to prefer for draws at scattered points, or when a factor of small rank is at hand anyway.

    ``family="matern1"`` and ``metric`` as for ``KernelCovarianceOperator`` (a scalar metric on a grid with one axis).  With a metric the
    kernel is even only in the whole offset vector, so the circulant's first column is built from signed offsets; its spectrum is real
    all the same, and the apply, the sampler with its growth and clipping, the factor and ``GridKernelPrior`` run as for every kernel.
    ``GridKernelCovarianceOperator(shape, spacing, **bilaplacian_kernel_2d(gamma, delta))`` is the BiLaplacian prior's covariance.
    ``family="matern"`` with ``nu`` (keyword only) as for ``KernelCovarianceOperator``: only the first column's entries differ, so the
    sampler, the factor and ``GridKernelPrior`` follow; ``**whittle_matern_kernel(gamma, delta, alpha, d)`` splats the same way.

    ``long_axes=True`` takes the long route (hfmi_op_kernel_cov_grid_long): an embedding axis longer than one workgroup's line
    (4096, or the tuning key "fftcov_max_line" at creation) is split in two passes, so axes may have up to 2^23 nodes, and
    ``sampler(max_growth=...)`` may double the embedding up to 6 times (every padded axis at most max_line^2).  Where no axis is split
    the applies, draws and factors are bit-identical to the default route's.  ``.long_axes`` records the choice."""

    def __init__(self, shape, spacing, family="matern32", sigma=1.0, ell=0.1, nugget=0.0, nodes=None, origin=None, ctx=None, *, long_axes=False,
                 nu=None, metric=None):
        # keyword-only from `long_axes` on: `metric` stays the last parameter (what splats of bilaplacian_kernel_2d rely on), and a
        # positional tenth argument is refused instead of landing in the new keyword's slot
        self.long_axes = bool(long_axes)
        n, h, nodes, o = _check_grid(shape, spacing, nodes, origin, family, ell, nugget,
                                     L.GRID_COV_LONG_MAX_NODES if self.long_axes else L.GRID_COV_MAX_NODES)
        G = _check_metric(metric, int(n.size))
        nu = _check_nu(family, nu)
        N = int(np.prod(n)) if nodes is None else int(nodes.size)
        super().__init__(ctx, N)
        self.grid_shape = tuple(int(v) for v in n)
        self.spacing, self.origin, self.nodes = h, o, nodes
        self.family, self.sigma, self.ell, self.nugget = family, float(sigma), float(ell), float(nugget)
        self.metric, self.nu = G, nu
        self.points = L.as_f64(grid_node_points(n, h, nodes, o))
        if self.long_axes:
            spec = _kernel_spec(family, int(n.size), self.sigma, self.ell, self.nugget, G, nu)
            L.call("hfmi_op_kernel_cov_grid_long" + ("" if nu is None else "_spec2"), self.ctx.handle, int(n.size), L.ptr(n), L.ptr(h), None if nodes is None else L.ptr(nodes),
                   N, C.byref(spec), C.byref(self._op))
        elif family == "matern1" or G is not None or nu is not None:
            spec = _kernel_spec(family, int(n.size), self.sigma, self.ell, self.nugget, G, nu)
            L.call("hfmi_op_kernel_cov_grid" + _spec_suffix(nu), self.ctx.handle, int(n.size), L.ptr(n), L.ptr(h), None if nodes is None else L.ptr(nodes),
                   N, C.byref(spec), C.byref(self._op))
        else:
            L.call("hfmi_op_kernel_cov_grid", self.ctx.handle, int(n.size), L.ptr(n), L.ptr(h), None if nodes is None else L.ptr(nodes), N,
                   L.KERNEL_FAMILIES[family], self.sigma, self.ell, self.nugget, C.byref(self._op))

    def to_dense(self, rows=None):
        """The same matrix on the host (``kernel_cov_host``): for checks at sizes where it fits."""
        return kernel_cov_host(self.points, self.family, self.sigma, self.ell, self.nugget, rows=rows, nu=self.nu, metric=self.metric)

    def matrix_free(self):
        """The ``KernelCovarianceOperator`` over the same points: 2 N^2 k flops per apply, no padded grid in memory."""
        return KernelCovarianceOperator(self.points, self.family, self.sigma, self.ell, self.nugget, ctx=self.ctx, nu=self.nu,
                                        metric=self.metric)

    def sampler(self, max_growth=3, on_indefinite="raise", seed=0):
        """A ``GridFieldSampler``: exact draws m ~ N(0, C) at the cost of an apply (see the class)."""
        return GridFieldSampler(self, max_growth=max_growth, on_indefinite=on_indefinite, seed=seed)


class GridFieldSampler:
    """Exact draws ``m ~ N(0, C)`` of a ``GridKernelCovarianceOperator`` by circulant embedding (hfmi_grid_sampler_*, hfmi_fftcov.hip):
    coloured noise ``sqrt(Lambda / P) (xi_1 + i xi_2)`` generated on the device, transformed back by the operator's inverse passes; the real
    and the imaginary part on the nodes are two independent draws, d passes per pair against the 2 d - 1 of an apply.  The sampler has
    an embedding of its own: the minimal one is often indefinite, so every padded axis is doubled ``growth`` <= ``max_growth`` (0..3;
    0..6 for an operator with ``long_axes``) times until no eigenvalue is below minus a rounding floor.  If none is definite, ``on_indefinite="raise"`` raises ``HfmiError`` with
    ``lambda_min / lambda_max`` of the last growth; ``"clip"`` zeroes the negative eigenvalues and reports ``n_clipped`` and
    ``cov_error_bound``: every entry of ``Cov(draw) - C`` is at most that in magnitude.  ``growth``, ``embedding`` (P_c per grid axis),
    ``lambda_min``, ``lambda_max``, ``n_clipped``, ``cov_error_bound`` are attributes.  The sampler keeps copies of what it needs: it does not
    keep the operator alive.  Prefer ``PivotedCholesky.sample`` when the draws are wanted at scattered points (``sample_at``), when the
    factor is needed anyway and its rank is small (smooth kernels, long correlation lengths), or when even three doublings leave a
    clip whose bound is too large; prefer this one for rough kernels, short correlation lengths and large grids, where it is exact
    and costs O(P log P) per pair."""

    def __init__(self, op, max_growth=3, on_indefinite="raise", seed=0):
        if not isinstance(op, GridKernelCovarianceOperator):
            raise ValueError("GridFieldSampler: a GridKernelCovarianceOperator is required (got %s)" % type(op).__name__)
        if on_indefinite not in ("raise", "clip"):
            raise ValueError("on_indefinite is 'raise' or 'clip', got %r" % (on_indefinite,))
        self.ctx = op.ctx
        self.N = op.shape[0]
        self.seed = int(seed)
        self._next = 0                   # sample_block's counter: the next draw of the stream `seed`, kept even
        self.handle = C.c_void_p()
        create = "hfmi_grid_sampler_create_long" if getattr(op, "long_axes", False) else "hfmi_grid_sampler_create"   # max_growth 0..6 / 0..3
        L.call(create, op._op, int(max_growth), 1 if on_indefinite == "clip" else 0, C.byref(self.handle))
        g, P, lo, hi, nc, bound = C.c_int(), (C.c_int64 * 3)(), C.c_double(), C.c_double(), C.c_int64(), C.c_double()
        L.call("hfmi_grid_sampler_info", self.handle, C.byref(g), P, C.byref(lo), C.byref(hi), C.byref(nc), C.byref(bound))
        self.growth = g.value
        self.embedding = tuple(int(v) for v in P[:len(op.grid_shape)])
        self.lambda_min, self.lambda_max = lo.value, hi.value
        self.n_clipped, self.cov_error_bound = int(nc.value), bound.value

    def sample(self, n, seed, first=0, out=None, accumulate=False):
        """Draws ``first .. first + n - 1`` of the stream ``seed`` as a ``MultiVector`` of ``n`` vectors of length N (``out``, or a new
        one; ``accumulate`` adds to ``out``).  Draws 2 p and 2 p + 1 are one transform: ``first`` must be even, and consecutive calls with
        ``first = 0, n, 2 n, ...`` (n even) give the bits of one large call."""
        if out is None:
            out = MultiVector(self.N, int(n), ctx=self.ctx)
        elif out.nvec() != int(n):
            raise ValueError("sample: out has %d vectors, n = %d" % (out.nvec(), int(n)))
        L.call("hfmi_grid_sampler_draw", self.handle, out.handle, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(first), 1 if accumulate else 0)
        return out

    def sample_block(self, n):
        """(n, N) array of the next ``n`` draws of the stream of the seed given at construction: what ``_prior_sample_block`` asks of a
        prior.  The counter advances by ``n`` rounded up to even (a dropped imaginary part is not handed out later)."""
        X = self.sample(n, self.seed, first=self._next)
        self._next += int(n) + (int(n) & 1)
        return np.ascontiguousarray(X.to_dense().T)

    def factor(self):
        """The factor ``S`` of this sampler's embedding, C = S S^T (``GridCovarianceFactor``)."""
        return GridCovarianceFactor(self)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                L.load().hfmi_grid_sampler_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class GridCovarianceFactor(DeviceOperator):
    """The factor ``S = Rn Chat^(1/2)`` of a ``GridFieldSampler``'s embedding (hfmi_op_grid_factor): ``S S^T = C`` up to rounding, ``C + E``
    with ``|E_ij| <= cov_error_bound`` for a clipped sampler.  ``shape == (N, Ptot)``, ``Ptot = prod(sampler.embedding)``: ``mult`` /
    ``matMvMult`` take padded vectors (natural order, entry e = s0 + P0 (s1 + P1 s2)) to the nodes, ``transpmult`` the other way;
    ``transpose()`` is ``S^T`` as an operator of its own (what a whitened Hessian S^T H S composes).  ``init_vector(x, dim)``: 0 gives N
    entries, 1 gives Ptot.  Ptot is 4 to 64 times N depending on the number of axes and the growth: that is the price of handing the
    noise over instead of letting ``GridFieldSampler.sample`` generate it.  The operator keeps the sampler alive."""

    def __init__(self, sampler, _transpose=False, _other=None):
        if not isinstance(sampler, GridFieldSampler):
            raise ValueError("GridCovarianceFactor: a GridFieldSampler is required (got %s)" % type(sampler).__name__)
        Ptot = int(np.prod(sampler.embedding))
        super().__init__(sampler.ctx, *((Ptot, sampler.N) if _transpose else (sampler.N, Ptot)))
        self.sampler = sampler
        self.is_transpose = bool(_transpose)
        self._other = _other
        L.call("hfmi_op_grid_factor", sampler.handle, 1 if _transpose else 0, C.byref(self._op))

    def transpose(self):
        """``S^T`` of ``S`` and back: an operator of shape ``shape[::-1]`` over the same sampler (made once)."""
        if self._other is None:
            self._other = GridCovarianceFactor(self.sampler, _transpose=not self.is_transpose, _other=self)
        return self._other

    def transpmult(self, x, y):
        self.transpose().mult(x, y)

    def matMvTranspmult(self, X, Y, accumulate=False):
        self.transpose().matMvMult(X, Y, accumulate=accumulate)


class _GridCovarianceSolver:
    """``prior.Rsolver`` of a ``GridKernelPrior``: ``solve(y, x)`` is y = R^-1 x = C x, an apply and no solve."""

    def __init__(self, op):
        self.op = op

    def init_vector(self, x, dim=0):
        self.op.init_vector(x, dim)

    def solve(self, y, x):
        if H.is_host_vector(x):
            X = MultiVector.from_vectors(np.asarray(x.get_local(), dtype=np.float64)[None, :], ctx=self.op.ctx)
            Y = MultiVector(self.op.shape[0], 1, ctx=self.op.ctx)
            self.op.matMvMult(X, Y)
            y.set_local(Y.to_vectors()[0])
            y.apply("")
        else:
            self.op.mult(x, y)

    def _device_operator(self):
        return self.op


class _KernelFactorPrior:
    """What ``GridKernelPrior`` and ``InterpolatedKernelPrior`` share: a covariance operator ``C`` with a factor C = F F^T behind the PRIOR
    protocol, the mean, ``Rsolver`` (an apply of C), the absent ``R``, ``sample`` (mean + factor . noise) and ``sample_block`` (noise
    generated on the device by ``sampler``)."""

    _noise_of = "the embedding"        # what the noise's length is that of, in sample's message

    def _setup(self, op, sampler, factor, mean, M, Msolver):
        self.C = op
        self.ctx = op.ctx
        self.N = op.shape[0]
        self.sampler = sampler
        self._factor = factor
        self.Rsolver = _GridCovarianceSolver(op)
        if M is not None:
            self.M = M
        if Msolver is not None:
            self.Msolver = Msolver
        mean = np.zeros(self.N) if mean is None else np.asarray(mean.get_local() if hasattr(mean, "get_local") else mean, dtype=np.float64)
        if mean.shape != (self.N,):
            raise ValueError("%s: the mean has %s entries, the operator %d points" % (type(self).__name__, mean.shape, self.N))
        self._mean = mean.copy()
        self.mean = H.new_host_vector()
        self.mean.init(self.N)
        self.mean.set_local(self._mean)
        self.mean.apply("")

    growth = property(lambda self: self.sampler.growth)
    embedding = property(lambda self: self.sampler.embedding)
    n_clipped = property(lambda self: self.sampler.n_clipped)
    cov_error_bound = property(lambda self: self.sampler.cov_error_bound)

    def __getattr__(self, name):          # only reached for attributes that are not there
        if name == "R":
            raise AttributeError("%s has no precision R = C^-1 and never solves with C: the prior-preconditioned double pass "
                                 "is randomized.doublePassC(A, prior.C, Omega, k), encoders come out of it, draws are prior.sample"
                                 % type(self).__name__)
        raise AttributeError("%s object has no attribute %r" % (type(self).__name__, name))

    def init_vector(self, x, dim):
        x.init(self._factor.shape[1] if dim == "noise" else self.N)

    def sample(self, noise, m, add_mean=True):
        """m = mean + factor . noise (``add_mean=False``: without the mean); ``noise`` has ``init_vector(x, "noise")`` entries, m has N."""
        host = H.is_host_vector(noise)
        xi = np.asarray(noise.get_local() if host else noise._mv.to_vectors()[0], dtype=np.float64)
        nn = self._factor.shape[1]
        if xi.shape != (nn,):
            raise ValueError("%s.sample: the noise has %s entries, %s %d (init_vector(x, 'noise'))" % (type(self).__name__, xi.shape, self._noise_of, nn))
        Xi = MultiVector.from_vectors(xi[None, :], ctx=self.ctx)
        Y = MultiVector(self.N, 1, ctx=self.ctx)
        self._factor.matMvMult(Xi, Y)
        y = Y.to_vectors()[0]
        if add_mean:
            y = y + self._mean
        if H.is_host_vector(m):
            m.set_local(y)
            m.apply("")
        else:
            L.call("hfmi_block_upload", m._mv.handle, L.ptr(L.as_f64(y[None, :])), L.LAYOUT_VECTORS)

    def sample_block(self, n):
        """(n, N) array of the next n draws mean + N(0, C) with noise generated on the device (the sampler's ``sample_block``)."""
        return self.sampler.sample_block(n) + self._mean[None, :]


class GridKernelPrior(_KernelFactorPrior):
    """A ``GridKernelCovarianceOperator`` behind the PRIOR protocol of the drivers (projectors.py, datagen.py, datasets.py, errors.py):
    ``init_vector(x, "noise")``, ``sample(noise, m)``, ``mean``, ``Rsolver``, ``M`` / ``Msolver`` -- with NO precision ``R``: a kernel
    covariance has no sparse inverse, and a Krylov solve with C needs hundreds of applies where it converges at all.  Nothing here
    solves with C.  ``sample`` is m = mean + S noise with the factor C = S S^T of a sampler's embedding (``GridCovarianceFactor``); the
    prior-preconditioned active subspace takes ``randomized.doublePassC``, which works in encoder coordinates and needs C alone.

    ``init_vector(x, dim)``: ``"noise"`` gives ``Ptot = prod(embedding)`` entries (4 to 64 times N, depending on the number of axes and
    the growth), 0 / 1 give N.  ``sample(noise, m, add_mean=True)`` works on dolfin-like host vectors (or device ``Vector``s);
    ``sample_block(n)`` hands out draws with noise generated on the device and stays the cheap route for many draws.  ``C`` is the
    operator, ``Rsolver.solve(y, x)`` is y = C x; ``mean`` defaults to zero; ``M`` / ``Msolver`` are whatever the caller has (KLE with
    ``orthogonality='mass'`` needs them).  ``growth``, ``embedding``, ``n_clipped`` and ``cov_error_bound`` are the sampler's.  ``R`` is
    deliberately absent: reading it raises ``AttributeError`` pointing at ``doublePassC``."""

    def __init__(self, op, mean=None, M=None, Msolver=None, max_growth=3, on_indefinite="raise", seed=0):
        if not isinstance(op, GridKernelCovarianceOperator):
            raise ValueError("GridKernelPrior: a GridKernelCovarianceOperator is required (got %s)" % type(op).__name__)
        sampler = op.sampler(max_growth=max_growth, on_indefinite=on_indefinite, seed=seed)
        self.S = sampler.factor()
        self._setup(op, sampler, self.S, mean, M, Msolver)


def _interp_grid_args(shape, spacing, origin, points):
    """(n, h, o, pts) as the arrays hfmi_grid_interp_weights takes; only shapes are checked here, the rules are the library's"""
    n = np.ascontiguousarray(np.atleast_1d(np.asarray(shape, dtype=np.int64)))
    if n.ndim != 1 or not 1 <= n.size <= 3:
        raise ValueError("a grid has 1, 2 or 3 axes, got shape %r" % (shape,))
    h = np.asarray(spacing, dtype=np.float64)
    h = np.ascontiguousarray(np.full(n.size, float(h)) if h.ndim == 0 else h)
    o = np.ascontiguousarray(np.zeros(n.size) if origin is None else np.atleast_1d(np.asarray(origin, dtype=np.float64)))
    pts = _points_array(points)
    if h.shape != n.shape or o.shape != n.shape or pts.shape[1] != n.size:
        raise ValueError("spacing, origin and the points' coordinates: one entry per axis of the grid %r" % (tuple(int(v) for v in n),))
    return n, h, o, pts


class GridInterpolationOperator(DeviceOperator):
    """The sparse cubic interpolation W from the nodes of a regular grid to N scattered points (hfmi_op_grid_interp, hfmi_interp.hip):
    ``shape == (N, prod(grid))``, ``mult`` / ``matMvMult`` take grid blocks to the points (a gather), ``transpose()`` is W^T as an
    operator of its own (a spread without atomics: bit-identical from apply to apply).  Per axis a point needs
    1 <= (x - origin) / spacing <= n - 2; its four weights are Keys' cubic convolution (a = -1/2), computed once on the host and
    uploaded, 4 d doubles and two indices per point.  ``weights()`` returns ``(base, w)`` -- the node of each point's stencil corner
    and the (N, d, 4) weights, the operator's own to the last bit -- and ``to_dense()`` the N x prod(grid) matrix from them.  Grid
    numbering as ``grid_node_points``: axis 0 fastest."""

    def __init__(self, shape, spacing, origin, points, ctx=None, _transpose=False, _other=None):
        n, h, o, pts = _interp_grid_args(shape, spacing, origin, points)
        Ng, N = int(np.prod(n)), pts.shape[0]
        super().__init__(ctx, *((Ng, N) if _transpose else (N, Ng)))
        self.grid_shape = tuple(int(v) for v in n)
        self.spacing, self.origin, self.points = h, o, pts
        self.is_transpose = bool(_transpose)
        self._other = _other
        L.call("hfmi_op_grid_interp", self.ctx.handle, int(n.size), L.ptr(n), L.ptr(h), L.ptr(o), L.ptr(pts), N, 1 if _transpose else 0,
               C.byref(self._op))

    def transpose(self):
        """``W^T`` of ``W`` and back: an operator of shape ``shape[::-1]`` over the same points (made once)."""
        if self._other is None:
            self._other = GridInterpolationOperator(self.grid_shape, self.spacing, self.origin, self.points, ctx=self.ctx,
                                                    _transpose=not self.is_transpose, _other=self)
        return self._other

    def transpmult(self, x, y):
        self.transpose().mult(x, y)

    def matMvTranspmult(self, X, Y, accumulate=False):
        self.transpose().matMvMult(X, Y, accumulate=accumulate)

    def weights(self, bins=False):
        """``(base, w)``: int64 (N,) nodes of the stencil corners and float64 (N, d, 4) weights, from the host rules the operator was
        built with (hfmi_grid_interp_weights; no device).  ``bins=True`` adds ``(cell_start, perm)``, the cell binning the spread walks."""
        n = np.ascontiguousarray(np.asarray(self.grid_shape, dtype=np.int64))
        N, d = self.points.shape
        base, w = np.empty(N, dtype=np.int64), np.empty((N, d, 4))
        cs = np.empty(int(np.prod(n - 3)) + 1, dtype=np.int64) if bins else None
        perm = np.empty(N, dtype=np.int64) if bins else None
        L.call("hfmi_grid_interp_weights", d, L.ptr(n), L.ptr(self.spacing), L.ptr(self.origin), L.ptr(self.points), N, L.ptr(base), L.ptr(w),
               L.ptr(cs) if bins else None, L.ptr(perm) if bins else None)
        return (base, w, cs, perm) if bins else (base, w)

    def to_dense(self):
        """The dense matrix on the host from ``weights()`` (W, or W^T for a transposed operator): for checks at sizes where it fits."""
        base, w = self.weights()
        n = self.grid_shape
        N, d = self.points.shape
        W = np.zeros((N, int(np.prod(n))))
        rows = np.arange(N)
        for s2 in range(4 if d > 2 else 1):
            for s1 in range(4 if d > 1 else 1):
                for s0 in range(4):
                    wt = w[:, 0, s0] if d == 1 else w[:, 1, s1] * w[:, 0, s0] if d == 2 else (w[:, 2, s2] * w[:, 1, s1]) * w[:, 0, s0]
                    W[rows, base + s0 + (n[0] * s1 if d > 1 else 0) + (n[0] * n[1] * s2 if d > 2 else 0)] = wt
        return np.ascontiguousarray(W.T) if self.is_transpose else W


class InterpolatedKernelCovarianceOperator(DeviceOperator):
    """A kernel covariance over SCATTERED points on the FFT route, by structured kernel interpolation (hfmi_op_kernel_cov_interp):

        K = W Cg W^T + diag(delta)

    with ``Cg`` the ``GridKernelCovarianceOperator`` of the same kernel over all nodes of a regular grid that covers the points
    (nugget 0) and ``W`` the sparse cubic ``GridInterpolationOperator`` from its nodes to the points.  An apply is one spread, the grid's
    FFT apply and one gather: O(4^d N + P log P) against the 2 N^2 flops per vector of ``KernelCovarianceOperator``.  K is symmetric
    positive semidefinite by construction, whatever the interpolation error.

    **K is not C.**  Unlike every other operator of this family it is an approximation of the covariance
    ``C = kernel_cov_host(points, ...)``; the device is held to K as defined at rounding level, and K - C is a property of the kernel and
    of ``ell / h``.  ``delta_i = nugget + max(sigma^2 - q_i, 0)`` with ``q_i = (W Cg W^T)_ii`` (``diag_correction=True``, the default)
    makes the marginal variances exact, ``K_ii = sigma^2 + nugget``, wherever nothing was clipped; ``diag_min`` / ``diag_max`` are the
    extremes of ``sigma^2 - q_i`` and ``n_diag_clipped`` counts the negative ones.  Measured on the CPU in numpy (400 random points in
    the unit square, ``ell = 0.2``, ``ell / h = 8``; tests/test_grid_interp_cpu.py recomputes the first three rows on its own point set):

        family     max_ij |K - C| / sigma^2     sigma^2 - q_i
        matern32   2.0e-3                       6.4e-6 .. 2.2e-3
        matern52   4.1e-4                       1.3e-6 .. 4.3e-4
        sqexp      1.4e-4                       2.2e-7 .. 6.8e-5
        matern12   2.8e-2                       1.5e-4 .. 5.0e-2

    With the correction the ten leading eigenvalues were within 8.1e-5 (matern52) and 7.7e-5 (matern32) relative of those of C.  At
    ``ell / h = 4`` the first column reads 4.9e-3 (matern52) and 1.3e-2 (matern32); matern12 stays at 2.8e-2 at ``ell / h = 8`` and
    7.1e-2 at 4.  Prefer ``matrix_free()`` (exact, 2 N^2 flops per vector) or ``pivoted_cholesky(op.matrix_free())`` for rough kernels
    such as matern12, and whenever an ``ell / h`` that makes the error acceptable cannot be afforded (the grid has
    ``prod(ceil(extent / h) + 4)`` nodes); prefer this operator for smooth kernels over many points.

    The grid is placed here: ``h = ell / cells_per_ell`` unless ``spacing`` is given (a number or one per axis), ``origin = min(points) -
    h`` and ``n = ceil((max - min) / h) + 4`` nodes per axis, so that every point has its full stencil.  ``long_axes`` as for
    ``GridKernelCovarianceOperator``; ``family``, ``nu`` and ``metric`` as everywhere in this family.  Attributes: ``grid`` (the grid
    operator), ``W`` (made on first use), ``delta``, ``q``, ``diag_min``, ``diag_max``, ``n_diag_clipped``.  ``to_dense()`` is the dense
    K on the host from ``W.to_dense()`` and ``grid.to_dense()``, ``exact_dense()`` is C, ``matrix_free()`` the exact operator over the
    same points, ``cross(targets)`` the Nystrom extension ``K(T, S) = W_T Cg W_S^T`` and ``sampler()`` an
    ``InterpolatedFieldSampler``.  Two vectors ride one complex transform of the grid apply, as there; two applies are bit-identical."""

    def __init__(self, points, family="matern32", sigma=1.0, ell=0.1, nugget=0.0, *, cells_per_ell=8, spacing=None, diag_correction=True,
                 long_axes=False, nu=None, metric=None, ctx=None):
        pts = _points_array(points)
        d = pts.shape[1]
        if not np.all(np.isfinite(pts)):
            raise ValueError("points: every coordinate must be finite")
        if not float(ell) > 0.0:
            raise ValueError("the correlation length must be positive")
        if spacing is None:
            if not float(cells_per_ell) > 0.0:
                raise ValueError("cells_per_ell must be positive")
            h = np.full(d, float(ell) / float(cells_per_ell))
        else:
            h = np.asarray(spacing, dtype=np.float64)
            h = np.full(d, float(h)) if h.ndim == 0 else h.copy()
            if h.shape != (d,) or not np.all(np.isfinite(h)) or not np.all(h > 0.0):
                raise ValueError("spacing: one positive finite number per axis, got %r" % (spacing,))
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        o = lo - h
        for c in range(d):      # the cell rule's own arithmetic must put min(points) at u >= 1
            while (lo[c] - o[c]) / h[c] < 1.0:
                o[c] = np.nextafter(o[c], -np.inf)
        n = np.ceil((hi - lo) / h).astype(np.int64) + 4
        cap = L.GRID_COV_LONG_MAX_NODES if long_axes else L.GRID_COV_MAX_NODES
        if n.max() > cap:
            raise ValueError("the grid over the points needs %r nodes per axis, more than the %d of this route: enlarge `spacing`, lower "
                             "`cells_per_ell` (now h = %r)%s" % (tuple(int(v) for v in n), cap, tuple(float(v) for v in h),
                                                              " (`long_axes=True` is taken already)" if long_axes else ", or take `long_axes=True`"))
        grid = GridKernelCovarianceOperator(tuple(int(v) for v in n), h, family=family, sigma=sigma, ell=ell, nugget=0.0, origin=o, ctx=ctx,
                                            long_axes=long_axes, nu=nu, metric=metric)
        self._attach(grid, pts, nugget, diag_correction)

    @classmethod
    def on_grid(cls, grid, points, nugget=0.0, diag_correction=True):
        """K over ``points`` on a grid operator the caller placed: a ``GridKernelCovarianceOperator`` over all nodes with nugget 0 whose
        grid gives every point its full stencil, 1 <= (x - origin) / spacing <= n - 2 per axis.  Several point sets may share one."""
        if not isinstance(grid, GridKernelCovarianceOperator):
            raise ValueError("on_grid: a GridKernelCovarianceOperator is required (got %s)" % type(grid).__name__)
        self = cls.__new__(cls)
        self._attach(grid, _points_array(points), nugget, diag_correction)
        return self

    def _attach(self, grid, pts, nugget, diag_correction):
        self.grid = grid
        DeviceOperator.__init__(self, grid.ctx, pts.shape[0])
        self.points, self.family, self.sigma, self.ell, self.nugget = pts, grid.family, grid.sigma, grid.ell, float(nugget)
        self.nu, self.metric, self.long_axes = grid.nu, grid.metric, grid.long_axes
        self.diag_correction = bool(diag_correction)
        self.grid_shape, self.spacing, self.origin = grid.grid_shape, np.ascontiguousarray(grid.spacing), np.ascontiguousarray(grid.origin)
        self._keep = [grid]      # the C operator refers to the grid operator
        self._W = None
        N = pts.shape[0]
        if pts.shape[1] != len(self.grid_shape):
            raise ValueError("the points have %d coordinates, the grid %d axes" % (pts.shape[1], len(self.grid_shape)))
        L.call("hfmi_op_kernel_cov_interp", grid._op, L.ptr(self.origin), L.ptr(pts), N, self.nugget, 1 if self.diag_correction else 0,
               C.byref(self._op))
        lo_, hi_, nc = C.c_double(), C.c_double(), C.c_int64()
        L.call("hfmi_op_kernel_cov_interp_info", self._op, C.byref(lo_), C.byref(hi_), C.byref(nc))
        self.diag_min, self.diag_max, self.n_diag_clipped = lo_.value, hi_.value, int(nc.value)
        self.q, self.delta = np.empty(N), np.empty(N)
        L.call("hfmi_op_kernel_cov_interp_diag", self._op, L.ptr(self.q), L.ptr(self.delta))

    @property
    def W(self):
        """The ``GridInterpolationOperator`` of these points on ``grid``'s nodes (a device object of its own, made on first use)."""
        if self._W is None:
            self._W = GridInterpolationOperator(self.grid_shape, self.spacing, self.origin, self.points, ctx=self.ctx)
        return self._W

    def to_dense(self):
        """The dense K on the host, ``W Cg W^T + diag(delta)`` from ``W.to_dense()``, ``grid.to_dense()`` and ``delta``."""
        W = self.W.to_dense()
        K = W @ self.grid.to_dense() @ W.T
        K[np.diag_indices_from(K)] += self.delta
        return K

    def exact_dense(self, rows=None):
        """The covariance C that K approximates (``kernel_cov_host`` over the points, with the nugget)."""
        return kernel_cov_host(self.points, self.family, self.sigma, self.ell, self.nugget, rows=rows, nu=self.nu, metric=self.metric)

    def matrix_free(self):
        """The exact ``KernelCovarianceOperator`` over the same points: 2 N^2 k flops per apply."""
        return KernelCovarianceOperator(self.points, self.family, self.sigma, self.ell, self.nugget, ctx=self.ctx, nu=self.nu, metric=self.metric)

    def cross(self, targets):
        """``K(T, S) = W_T Cg W_S^T`` from these points S to ``targets`` T on the same grid, a ``ComposedOperator`` of shape (M, N): the
        Nystrom extension without a second N x M kernel sweep.  Every target needs its full stencil inside the grid."""
        WT = GridInterpolationOperator(self.grid_shape, self.spacing, self.origin, targets, ctx=self.ctx)
        return ComposedOperator(self.W.transpose(), self.grid, WT)

    def sampler(self, max_growth=3, on_indefinite="raise", seed=0):
        """An ``InterpolatedFieldSampler``: draws ``W z + sqrt(delta) eta`` ~ N(0, K) at the cost of a grid draw and a gather."""
        return InterpolatedFieldSampler(self, max_growth=max_growth, on_indefinite=on_indefinite, seed=seed)


class InterpolatedFieldSampler:
    """Draws ``m = W z + sqrt(delta) eta ~ N(0, K)`` of an ``InterpolatedKernelCovarianceOperator`` (hfmi_interp_sampler_draw): ``z`` is
    the exact grid draw of the grid operator's ``GridFieldSampler`` (same seed, same draw number) and ``eta`` i.i.d. N(0, 1) from the
    probe draw's generator under a key of its own, so the two are independent.  The draws are exact for K, which is not C (see the
    operator).  ``growth``, ``embedding``, ``n_clipped`` and ``cov_error_bound`` are the grid sampler's; a clipped grid sampler adds
    its bound to K - C on the grid.  ``sample`` and ``sample_block`` mirror ``GridFieldSampler``.  Keeps the operator alive."""

    def __init__(self, op, max_growth=3, on_indefinite="raise", seed=0):
        if not isinstance(op, InterpolatedKernelCovarianceOperator):
            raise ValueError("InterpolatedFieldSampler: an InterpolatedKernelCovarianceOperator is required (got %s)" % type(op).__name__)
        self.op = op
        self.ctx = op.ctx
        self.N = op.shape[0]
        self.seed = int(seed)
        self._next = 0
        self.grid_sampler = GridFieldSampler(op.grid, max_growth=max_growth, on_indefinite=on_indefinite, seed=seed)

    growth = property(lambda self: self.grid_sampler.growth)
    embedding = property(lambda self: self.grid_sampler.embedding)
    n_clipped = property(lambda self: self.grid_sampler.n_clipped)
    cov_error_bound = property(lambda self: self.grid_sampler.cov_error_bound)

    def sample(self, n, seed, first=0, out=None, accumulate=False):
        """Draws ``first .. first + n - 1`` of the stream ``seed`` as a ``MultiVector`` of ``n`` vectors of length N (``out``, or a new
        one; ``accumulate`` adds to ``out``).  ``first`` must be even; consecutive calls with ``first = 0, n, 2 n, ...`` (n even) give
        the bits of one large call."""
        if out is None:
            out = MultiVector(self.N, int(n), ctx=self.ctx)
        elif out.nvec() != int(n):
            raise ValueError("sample: out has %d vectors, n = %d" % (out.nvec(), int(n)))
        L.call("hfmi_interp_sampler_draw", self.op._op, self.grid_sampler.handle, out.handle, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
               int(first), 1 if accumulate else 0)
        return out

    def sample_block(self, n):
        """(n, N) array of the next ``n`` draws of the stream of the seed given at construction; the counter advances by ``n`` rounded
        up to even, as ``GridFieldSampler.sample_block``'s."""
        X = self.sample(n, self.seed, first=self._next)
        self._next += int(n) + (int(n) & 1)
        return np.ascontiguousarray(X.to_dense().T)

    def factor(self):
        """The factor ``F = [W S | diag(sqrt(delta))]`` of the operator over this sampler's embedding, K = F F^T
        (``InterpolatedCovarianceFactor``)."""
        return InterpolatedCovarianceFactor(self)


class InterpolatedCovarianceFactor(DeviceOperator):
    """The factor ``F = [ W S | diag(sqrt(delta)) ]`` of an ``InterpolatedKernelCovarianceOperator`` K over the embedding of an
    ``InterpolatedFieldSampler`` (hfmi_op_interp_factor): ``S`` is the ``GridCovarianceFactor`` of the grid sampler, ``F F^T = W S S^T W^T +
    diag(delta)`` is K up to rounding for a definite sampler.  ``shape == (N, Ptot + N)`` with ``Ptot = prod(sampler.embedding)`` and
    ``noise_split == (Ptot, N)``: the first Ptot entries of a noise vector are the padded-grid noise in ``GridCovarianceFactor``'s natural
    order, the last N one entry per point in the order of ``op.points``.  ``mult`` / ``matMvMult`` take noise to the points (the grid
    factor, then one gather with the tail fused), ``transpmult`` / ``matMvTranspmult`` the other way; ``transpose()`` is ``F^T`` as an
    operator of its own (what a whitened Hessian F^T H F composes).  ``init_vector(x, dim)``: 0 gives N entries, 1 gives Ptot + N.

    ``factor_error_bound`` bounds ``max_ij |F F^T - K|``: 0 for a definite sampler, ``1.25**(2 d) * sampler.cov_error_bound`` for a
    clipped one.  There ``S S^T = Cg + E`` with ``|E_ij| <= cov_error_bound``, so ``F F^T - K = W E W^T``; the four Keys weights of one axis
    have 1-norm ``1 + t (1 - t) <= 1.25``, a row of W has 1-norm at most ``1.25**d``, and ``|W E W^T|_ij <= |E|_max * 1.25**d * 1.25**d``.

    The price: a noise vector has ``Ptot + N`` entries, and Ptot is 4 to 64 times the grid, which itself covers the points' box at
    ``cells_per_ell`` nodes per correlation length: ``InterpolatedFieldSampler.sample_block`` (noise generated on the device) stays the
    route for many draws.  The operator keeps the sampler alive, and the sampler keeps K alive."""

    def __init__(self, sampler, _transpose=False, _other=None):
        if not isinstance(sampler, InterpolatedFieldSampler):
            raise ValueError("InterpolatedCovarianceFactor: an InterpolatedFieldSampler is required (got %s)" % type(sampler).__name__)
        Ptot, N = int(np.prod(sampler.embedding)), sampler.N
        super().__init__(sampler.ctx, *((Ptot + N, N) if _transpose else (N, Ptot + N)))
        self.sampler = sampler
        self.noise_split = (Ptot, N)
        self.is_transpose = bool(_transpose)
        self._other = _other
        self.factor_error_bound = 1.25 ** (2 * len(sampler.embedding)) * sampler.cov_error_bound
        L.call("hfmi_op_interp_factor", sampler.op._op, sampler.grid_sampler.handle, 1 if _transpose else 0, C.byref(self._op))

    def transpose(self):
        """``F^T`` of ``F`` and back: an operator of shape ``shape[::-1]`` over the same sampler (made once)."""
        if self._other is None:
            self._other = InterpolatedCovarianceFactor(self.sampler, _transpose=not self.is_transpose, _other=self)
        return self._other

    def transpmult(self, x, y):
        self.transpose().mult(x, y)

    def matMvTranspmult(self, X, Y, accumulate=False):
        self.transpose().matMvMult(X, Y, accumulate=accumulate)


class InterpolatedKernelPrior(_KernelFactorPrior):
    """An ``InterpolatedKernelCovarianceOperator`` behind the PRIOR protocol of the drivers, as ``GridKernelPrior`` puts a grid operator
    there: a kernel prior over SCATTERED points (mesh nodes, ``Vh.tabulate_dof_coordinates()``) with no assembly, no precision ``R`` and no
    solve.  ``sample`` is m = mean + F noise with the factor K = F F^T (``InterpolatedCovarianceFactor``); the prior-preconditioned active
    subspace takes ``randomized.doublePassC(A, prior.C, Omega, k)``, and ``F`` / ``F.transpose()`` compose the whitened Hessian.

    ``init_vector(x, dim)``: ``"noise"`` gives ``Ptot + N`` entries -- the padded-grid noise first, then one entry per point -- and 0 / 1
    give N.  Ptot = prod(embedding) is 4 to 64 times the grid, so a noise vector is far longer than a parameter:
    ``sample_block(n)`` hands out ``InterpolatedFieldSampler.sample_block``'s draws (noise generated on the device) plus the mean and
    stays the route for many draws.  ``C`` is the operator, ``Rsolver.solve(y, x)`` is y = K x; ``mean``, ``M`` / ``Msolver`` as for
    ``GridKernelPrior``.  ``growth``, ``embedding``, ``n_clipped`` and ``cov_error_bound`` are the sampler's, ``factor_error_bound`` the
    factor's.  ``R`` is deliberately absent: reading it raises ``AttributeError`` pointing at ``doublePassC``.  The Gaussian is N(mean, K),
    and K is not the exact kernel covariance (see the operator)."""

    _noise_of = "the factor"

    def __init__(self, op, mean=None, M=None, Msolver=None, max_growth=3, on_indefinite="raise", seed=0):
        if not isinstance(op, InterpolatedKernelCovarianceOperator):
            raise ValueError("InterpolatedKernelPrior: an InterpolatedKernelCovarianceOperator is required (got %s)" % type(op).__name__)
        sampler = op.sampler(max_growth=max_growth, on_indefinite=on_indefinite, seed=seed)
        self.F = sampler.factor()
        self._setup(op, sampler, self.F, mean, M, Msolver)

    factor_error_bound = property(lambda self: self.F.factor_error_bound)


class _BoxPowerOperator(DeviceOperator):
    """``W^a T_s W^b`` of a ``BoxSpectralCovariance`` (hfmi_op_box); ``transpose()`` is ``W^(1+b) T_s W^(a-1)``, its transpose (T_s^T =
    W T_s W^-1: T_s = Phi Lambda^s Phi^* W is self-adjoint in the W inner product).  The operator keeps the box alive."""

    def __init__(self, box, s, a, b, _other=None):
        super().__init__(box.ctx, box.N)
        self.box = box
        self.power = (float(s), float(a), float(b))
        self._other = _other
        L.call("hfmi_op_box", box.handle, self.power[0], self.power[1], self.power[2], C.byref(self._op))

    def transpose(self):
        if self._other is None:
            s, a, b = self.power
            self._other = _BoxPowerOperator(self.box, s, 1.0 + b, a - 1.0, _other=self)
        return self._other

    def transpmult(self, x, y):
        self.transpose().mult(x, y)

    def matMvTranspmult(self, X, Y, accumulate=False):
        self.transpose().matMvMult(X, Y, accumulate=accumulate)

    def solve(self, y, x):
        """y = (this operator)^-1 x when the inverse is at hand as another power of the same box: ``W^-b T_-s W^-a``."""
        s, a, b = self.power
        self.box.power(-s, -b, -a).mult(x, y)


def _box_axis_ok(n, boundary):
    """The rule of an axis of a box (boxcov_axis_ok of csrc/hfmi_boxcov_plan.h): the transformed line of P = 2 (n - 1) entries (Neumann,
    1 for one node) or P = n (periodic) is a power of two, or a multiple of 4 with no prime factor but 2, 3 and 5."""
    if n < 1 or n > (L.BOX_MAX_NEUMANN if boundary == "neumann" else L.BOX_MAX_PERIODIC):
        return False
    P = (2 * (n - 1) if n > 1 else 1) if boundary == "neumann" else n
    if P & (P - 1) == 0:
        return True
    if P % 4:
        return False
    for r in (2, 3, 5):
        while P % r == 0:
            P //= r
    return P == 1


class BoxSpectralCovariance:
    """The Whittle-Matern operator ``(delta - gamma div Theta grad)^(-alpha)`` on a box, on a regular grid with Neumann or periodic sides
    and axis-aligned ``Theta = diag(theta)``, diagonalised by cosine and Fourier transforms (hfmi_box_*, hfmi_boxcov.hip; include/hfmi.h
    states the contract).  Covariance, precision and both square roots are each one transform - multiply - inverse transform, exact up
    to rounding and O(N log N): nothing is grown, clipped, iterated or approximated, and a noise vector has N entries.

    ``shape``: nodes per axis (1 to 3 axes, axis 0 fastest, the numbering of ``grid_node_points``).  ``boundary``: "neumann" or
    "periodic", one string or one per axis.  The transformed line of an axis, 2 (n - 1) entries on a Neumann axis of n > 1 nodes and n on a
    periodic one, is a power of two or a multiple of 4 of the form 2^m 3^a 5^b, at most 4096: 2^m + 1 nodes as well as 7, 11, 13, 25, 49,
    97, 101, 193, 201, 385 ... Neumann (at most 2049), 2^m as well as 12, 20, 24, 48, 96, 100, 192 ... periodic (at most 4096).  ``symbol``:
    "fd" (the two-point stiffness with lumped mass: R = A W^-1 A exactly, A = delta W + gamma K; with Neumann sides and alpha = 2 the
    BiLaplacian prior on a tensor grid with lumped mass) or "continuous" ((t_k / h)^2).  Not itself an operator; the ``DeviceOperator``s
    are made on first use: ``.C`` (covariance of the nodal values), ``.R`` (= C^-1), ``.S`` (S S^T = C; ``.S.transpose()``,
    ``transpmult``, ``matMvTranspmult`` as ``GridCovarianceFactor`` has them), ``.Sinv`` (whitening) and ``.power(s, a, b)`` =
    ``W^a T_s W^b``.  ``.points``, ``.weights`` (N,), ``.spectrum()`` (mode-array shape, axis 0 first), ``.modes()`` (the dense
    W-orthonormal ``Phi`` on the host, from cosines and exponentials only, no FFT) and ``.to_dense(which)`` from those three are for
    checks at sizes where N x N fits."""

    def __init__(self, shape, spacing, gamma, delta, alpha=2.0, theta=None, boundary="neumann", symbol="fd", origin=None, ctx=None):
        raw = np.atleast_1d(np.asarray(shape))
        if raw.ndim != 1 or not 1 <= raw.size <= 3:
            raise ValueError("a grid has 1, 2 or 3 axes, got shape %r" % (shape,))
        if raw.dtype.kind not in "iuf" or not np.all(np.isfinite(raw)) or not np.all(raw == np.round(raw)):
            raise ValueError("shape: whole numbers of nodes per axis, got %r" % (shape,))
        n = raw.astype(np.int64)
        d = int(n.size)
        bd = [boundary] * d if isinstance(boundary, str) else list(boundary)
        if len(bd) != d or any(b not in L.BOX_BOUNDARIES for b in bd):
            raise ValueError("boundary: 'neumann' or 'periodic', one string or one per axis, got %r" % (boundary,))
        for c in range(d):
            v = int(n[c])
            if not _box_axis_ok(v, bd[c]):
                raise ValueError("axis %d: %d nodes; the line of an axis, 2 (n - 1) entries on a Neumann axis of n > 1 nodes and n on a "
                                 "periodic one, is a power of two or a multiple of 4 with no prime factor but 2, 3 and 5; a Neumann axis "
                                 "has at most %d nodes, a periodic one %d" % (c, v, L.BOX_MAX_NEUMANN, L.BOX_MAX_PERIODIC))
        if symbol not in L.BOX_SYMBOLS:
            raise ValueError("symbol is 'fd' or 'continuous', got %r" % (symbol,))
        h = np.asarray(spacing, dtype=np.float64)
        h = np.full(d, float(h)) if h.ndim == 0 else h
        if h.shape != n.shape or not np.all(np.isfinite(h)) or not np.all(h > 0.0):
            raise ValueError("spacing: one positive finite number per axis, got %r" % (spacing,))
        th = np.ones(d) if theta is None else np.asarray(theta, dtype=np.float64)
        th = np.full(d, float(th)) if th.ndim == 0 else th
        if th.shape != n.shape or not np.all(np.isfinite(th)) or not np.all(th > 0.0):
            raise ValueError("theta: one positive finite number per axis, got %r" % (theta,))
        for name, v in (("gamma", gamma), ("delta", delta), ("alpha", alpha)):
            if not (np.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError("%s must be positive and finite, got %r" % (name, v))
        o = np.zeros(d) if origin is None else np.asarray(origin, dtype=np.float64)
        if o.shape != n.shape or not np.all(np.isfinite(o)):
            raise ValueError("origin: one finite number per axis, got %r" % (origin,))
        self._ctx = ctx
        self.grid_shape = tuple(int(v) for v in n)
        self.N = int(np.prod(n))
        self.spacing, self.origin, self.theta = np.ascontiguousarray(h), o, np.ascontiguousarray(th)
        self.boundary, self.symbol = tuple(bd), symbol
        self.gamma, self.delta, self.alpha = float(gamma), float(delta), float(alpha)
        self.points = L.as_f64(grid_node_points(n, h, None, o))
        self._ops = {}
        self._handle = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = L.Context.default()
        return self._ctx

    @property
    def handle(self):
        """The hfmi_box, made at the first device use: the host formulas (``weights``, ``spectrum``, ``modes``, ``to_dense``) need none."""
        if self._handle is None:
            h = C.c_void_p()
            n = np.ascontiguousarray(self.grid_shape, dtype=np.int64)
            bnd = np.ascontiguousarray([L.BOX_BOUNDARIES[b] for b in self.boundary], dtype=np.int32)
            L.call("hfmi_box_create", self.ctx.handle, int(n.size), L.ptr(n), L.ptr(self.spacing), L.ptr(bnd), self.gamma, self.delta,
                   self.alpha, L.ptr(self.theta), L.BOX_SYMBOLS[self.symbol], C.byref(h))
            self._handle = h
        return self._handle

    def power(self, s, a=0.0, b=0.0):
        """``W^a T_s W^b`` as a ``DeviceOperator`` (made once per (s, a, b))."""
        key = (float(s), float(a), float(b))
        if key not in self._ops:
            self._ops[key] = _BoxPowerOperator(self, *key)
        return self._ops[key]

    C = property(lambda self: self.power(1.0, 0.0, -1.0))
    R = property(lambda self: self.power(-1.0, 1.0, 0.0))
    S = property(lambda self: self.power(0.5, 0.0, -0.5))
    Sinv = property(lambda self: self.power(-0.5, 0.5, 0.0))

    def _axis_weights(self, c):
        n, h = self.grid_shape[c], float(self.spacing[c])
        if self.boundary[c] == "periodic":
            return np.full(n, h)
        if n == 1:
            return np.ones(1)
        w = np.full(n, h)
        w[0] = w[-1] = 0.5 * h
        return w

    @property
    def weights(self):
        """(N,) quadrature weights ``prod_c w_c`` of the nodes: the diagonal of the lumped mass matrix W."""
        w = np.ones(1)
        for c in range(len(self.grid_shape)):      # axis 0 fastest: node g = i0 + n0 (i1 + n1 i2)
            w = np.kron(self._axis_weights(c), w)
        return np.ascontiguousarray(w)

    def _axis_symbol(self, c):
        n, h = self.grid_shape[c], float(self.spacing[c])
        k = np.arange(n)
        if self.boundary[c] == "periodic":
            t = 2.0 * np.pi * np.where(2 * k <= n, k, k - n) / n
        else:
            t = np.pi * k / (n - 1) if n > 1 else np.zeros(1)
        # fd: (2 - 2 cos t) / h^2, written without the cancellation at small t
        return (t / h) ** 2 if self.symbol == "continuous" else (2.0 * np.sin(0.5 * t) / h) ** 2

    def spectrum(self):
        """``lambda_k = (delta + gamma sum_c theta_c mu_c(k_c))^(-alpha)`` in mode-array shape ``grid_shape`` (entry [k0, k1, k2]), natural
        mode order, on the host (hfmi_box_spectrum is the library's statement of the same numbers)."""
        total = np.zeros(self.grid_shape)
        for c in range(len(self.grid_shape)):
            shape = [1] * len(self.grid_shape)
            shape[c] = self.grid_shape[c]
            total = total + self.theta[c] * self._axis_symbol(c).reshape(shape)
        return (self.delta + self.gamma * total) ** (-self.alpha)

    def _axis_modes(self, c):
        n, h = self.grid_shape[c], float(self.spacing[c])
        j = np.arange(n)[:, None]
        k = np.arange(n)[None, :]
        if self.boundary[c] == "periodic":
            ks = np.where(2 * k <= n, k, k - n)
            return np.exp(2j * np.pi * j * ks / n) / np.sqrt(n * h)
        if n == 1:
            return np.ones((1, 1))
        e = np.where((k == 0) | (k == n - 1), 1.0, 2.0)
        return np.sqrt(e / ((n - 1) * h)) * np.cos(np.pi * j * k / (n - 1))

    def modes(self):
        """The dense (N, N) ``Phi``: L2-normalised cosines (Neumann) and exponentials (periodic) sampled at the nodes, column k0 + n0 (k1 +
        n1 k2); ``Phi^* W Phi = I`` and ``C = Phi Lambda Phi^*``.  Complex when an axis is periodic."""
        Phi = np.ones((1, 1))
        for c in range(len(self.grid_shape)):
            Phi = np.kron(self._axis_modes(c), Phi)
        return Phi

    def dense_power(self, s, a=0.0, b=0.0):
        """``W^a T_s W^b = W^a Phi Lambda^s Phi^* W^(1+b)`` as a dense host matrix."""
        Phi, w = self.modes(), self.weights
        lam = self.spectrum().transpose().ravel()       # column order of Phi: k0 fastest
        A = (Phi * lam ** float(s)) @ Phi.conj().T
        return np.ascontiguousarray((w ** float(a))[:, None] * A.real * (w ** (1.0 + float(b)))[None, :])

    def to_dense(self, which="C"):
        """"C", "R", "S" (also "St", "Sinv") on the host, from ``modes()``, ``spectrum()`` and ``weights``."""
        powers = {"C": (1.0, 0.0, -1.0), "R": (-1.0, 1.0, 0.0), "S": (0.5, 0.0, -0.5), "St": (0.5, 0.5, -1.0), "Sinv": (-0.5, 0.5, 0.0)}
        if which not in powers:
            raise ValueError("to_dense: which is one of %s, got %r" % (sorted(powers), which))
        return self.dense_power(*powers[which])

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                L.load().hfmi_box_destroy(self._handle)
                self._handle = None
        except Exception:
            pass


class BoxSpectralPrior:
    """A ``BoxSpectralCovariance`` behind the FULL prior protocol of the drivers (projectors.py, datagen.py, datasets.py, errors.py): unlike
    the kernel priors it has a precision.  ``R`` and ``C`` are the box's device operators, ``Rsolver.solve(y, x)`` is y = C x (host or
    device vectors; ``as_device_operator(prior.Rsolver)`` is ``box.C``, no host callback), so ``ActiveSubspaceProjector``, ``doublePassG``
    and ``singlePassG`` take their existing routes with B and B^-1 both on the device.  ``init_vector(x, "noise")`` gives N entries;
    ``sample(noise, m, add_mean=True)`` is m = mean + S noise; ``sample_block(n)`` fills an (N, n) block with the device's Philox normals
    (hfmi_randn_fill, key ``seed``, stream = the number of earlier calls), applies S, adds the mean and returns (n, N);
    ``cost(m)`` = 0.5 (m - mean)^T R (m - mean).  ``M`` / ``Msolver`` are whatever the caller has (``scipy.sparse.diags(box.weights)`` is
    the lumped mass matrix; KLE with ``orthogonality='mass'`` over it is the analytical KLE)."""

    def __init__(self, box, mean=None, M=None, Msolver=None, seed=0):
        if not isinstance(box, BoxSpectralCovariance):
            raise ValueError("BoxSpectralPrior: a BoxSpectralCovariance is required (got %s)" % type(box).__name__)
        self.box = box
        self.ctx = box.ctx
        self.N = box.N
        self.R, self.C, self.S = box.R, box.C, box.S
        self.Rsolver = _GridCovarianceSolver(self.C)
        if M is not None:
            self.M = M
        if Msolver is not None:
            self.Msolver = Msolver
        self.seed = int(seed)
        self._calls = 0                  # sample_block's stream: the number of earlier calls
        mean = np.zeros(self.N) if mean is None else np.asarray(mean.get_local() if hasattr(mean, "get_local") else mean, dtype=np.float64)
        if mean.shape != (self.N,):
            raise ValueError("BoxSpectralPrior: the mean has %s entries, the box %d nodes" % (mean.shape, self.N))
        self._mean = mean.copy()
        self._mean_dev = None            # the mean as a device Vector, made when a device vector first needs it
        self.mean = H.new_host_vector()
        self.mean.init(self.N)
        self.mean.set_local(self._mean)
        self.mean.apply("")

    def init_vector(self, x, dim):
        x.init(self.N)

    @staticmethod
    def _host_array(v):
        if isinstance(v, np.ndarray):
            return np.asarray(v, dtype=np.float64)
        return np.asarray(v.get_local() if H.is_host_vector(v) else v._mv.to_vectors()[0], dtype=np.float64)

    def _device_mean(self):
        if self._mean_dev is None:
            self._mean_dev = Vector(ctx=self.ctx)
            self._mean_dev.init(self.N)
            self._mean_dev.set_local(self._mean)
        return self._mean_dev

    def sample(self, noise, m, add_mean=True):
        """m = mean + S noise (``add_mean=False``: without the mean); noise and m have N entries.  Two device ``Vector``s stay on the
        device (one apply of S and an axpy with the mean, no transfer); host vectors, or a mixed pair, go through the host."""
        if isinstance(noise, Vector) and isinstance(m, Vector):
            if noise.size() != self.N or m.size() != self.N:
                raise ValueError("BoxSpectralPrior.sample: noise and m have %d and %d entries, the box %d nodes" % (noise.size(), m.size(), self.N))
            self.S.mult(noise, m)
            if add_mean:
                m.axpy(1.0, self._device_mean())
            return
        xi = self._host_array(noise)
        if xi.shape != (self.N,):
            raise ValueError("BoxSpectralPrior.sample: the noise has %s entries, the box %d nodes" % (xi.shape, self.N))
        Xi = MultiVector.from_vectors(xi[None, :], ctx=self.ctx)
        Y = MultiVector(self.N, 1, ctx=self.ctx)
        self.S.matMvMult(Xi, Y)
        y = Y.to_vectors()[0]
        if add_mean:
            y = y + self._mean
        if H.is_host_vector(m):
            m.set_local(y)
            m.apply("")
        else:
            L.call("hfmi_block_upload", m._mv.handle, L.ptr(L.as_f64(y[None, :])), L.LAYOUT_VECTORS)

    def sample_block(self, n):
        """(n, N) array of n draws mean + S Xi, Xi the (N, n) block hfmi_randn_fill makes with key ``seed`` and stream = the number of
        earlier calls of this method."""
        Xi = MultiVector(self.N, int(n), ctx=self.ctx)
        L.call("hfmi_randn_fill", Xi.handle, C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), C.c_uint32(self._calls & 0xFFFFFFFF), 1.0)
        self._calls += 1
        Y = MultiVector(self.N, int(n), ctx=self.ctx)
        self.S.matMvMult(Xi, Y)
        return np.ascontiguousarray(Y.to_dense().T) + self._mean[None, :]

    def cost(self, m):
        """0.5 (m - mean)^T R (m - mean).  A device ``Vector`` stays on the device (an axpy, one apply of R, one inner product: only the
        number comes back); a host vector or an array is uploaded once and R (m - mean) comes back for the inner product on the host."""
        if isinstance(m, Vector):
            if m.size() != self.N:
                raise ValueError("BoxSpectralPrior.cost: m has %d entries, the box %d nodes" % (m.size(), self.N))
            dm = m.copy()
            dm.axpy(-1.0, self._device_mean())
            y = Vector(ctx=self.ctx)
            y.init(self.N)
            self.R.mult(dm, y)
            return 0.5 * dm.inner(y)
        dm = self._host_array(m) - self._mean
        X = MultiVector.from_vectors(dm[None, :], ctx=self.ctx)
        Y = MultiVector(self.N, 1, ctx=self.ctx)
        self.R.matMvMult(X, Y)
        return 0.5 * float(dm @ Y.to_vectors()[0])


def _is_null_collective(collective):
    from .collectives import NullCollective
    return isinstance(collective, NullCollective)


def shard_rows(N, size, rank):
    """Contiguous rows ``(row0, row1)`` of rank ``rank`` when ``N`` rows are dealt to ``size`` ranks: the first ``N % size`` ranks get one
    row more; ranges are empty when there are more ranks than rows."""
    N, size, rank = int(N), int(size), int(rank)
    if N < 0 or size < 1 or not 0 <= rank < size:
        raise ValueError("shard_rows: N = %d, size = %d, rank = %d" % (N, size, rank))
    q, rem = divmod(N, size)
    row0 = rank * q + min(rank, rem)
    return row0, row0 + q + (1 if rank < rem else 0)


def kernel_cross_cov_host(targets, sources, family, sigma, ell, nugget=0.0, diag_offset=None, *, nu=None, metric=None):
    """Dense host evaluation of what ``KernelCrossCovarianceOperator`` applies: the (M, N) matrix K_ij = sigma^2 phi(|t_i - s_j| / ell)
    + nugget [j == i + diag_offset], ``family``, ``nu`` and ``metric`` as in ``kernel_cov_host``.  ``diag_offset`` None: no target is a source
    (and the nugget must be 0).  With ``targets = points[r0:r1]``, ``sources = points`` and ``diag_offset = r0`` it is
    ``kernel_cov_host(points, ..., rows=range(r0, r1))``."""
    if family not in L.KERNEL_FAMILIES:
        raise _unknown_family(family)
    tg, src = _points_array(targets), _points_array(sources)
    _check_cross(tg, src, nugget, diag_offset)
    nu = _check_nu(family, nu)
    G = _check_metric(metric, src.shape[1])
    tg, src = _metric_points(tg, G), _metric_points(src, G)
    d2 = np.zeros((tg.shape[0], src.shape[0]))
    for c in range(src.shape[1]):
        d2 += (tg[:, c][:, None] - src[None, :, c]) ** 2
    K = sigma ** 2 * _kernel_phi(family, np.sqrt(d2), ell, nu)
    if nugget:
        i = np.arange(tg.shape[0])
        K[i, i + int(diag_offset)] += nugget
    return K


def _check_cross(tg, src, nugget, diag_offset):
    """The argument rules of hfmi_op_kernel_cross_cov that need no device."""
    M, N = tg.shape[0], src.shape[0]
    if tg.shape[1] != src.shape[1]:
        raise ValueError("targets have %d coordinates, sources %d" % (tg.shape[1], src.shape[1]))
    if M < 1 or N < 1:
        raise ValueError("a cross-covariance needs at least one target and one source (M = %d, N = %d)" % (M, N))
    if diag_offset is None:
        if nugget:
            raise ValueError("a nugget needs targets that are sources: pass diag_offset")
    elif int(diag_offset) < 0 or int(diag_offset) + M > N:
        raise ValueError("diag_offset = %d with %d targets does not lie inside the %d sources" % (diag_offset, M, N))


class KernelCrossCovarianceOperator(DeviceOperator):
    """Rectangular cross-covariance K(T, S) between M ``targets`` and N ``sources`` without the M x N matrix: y = K x maps length N to
    length M, K_ij = sigma^2 phi(|t_i - s_j| / ell) + nugget [j == i + diag_offset], by the kernel of ``KernelCovarianceOperator`` with a
    second coordinate set (hfmi_kcov.hip).  ``diag_offset``: target i IS source i + diag_offset (the nugget sits on the index); None: no
    target is a source, and the nugget must be 0.  What the Nystrom extension of a KLE or of a pivoted Cholesky factor applies
    (``nystrom_extend``, ``KLEProjector.extend``, ``PivotedCholesky.extend``)."""

    def __init__(self, targets, sources, family="matern32", sigma=1.0, ell=0.1, nugget=0.0, diag_offset=None, ctx=None, *, nu=None, metric=None):
        if family not in L.KERNEL_FAMILIES:
            raise _unknown_family(family)
        nu = _check_nu(family, nu)
        tg, src = _points_array(targets), _points_array(sources)
        _check_cross(tg, src, nugget, diag_offset)
        G = _check_metric(metric, src.shape[1])
        super().__init__(ctx, tg.shape[0], src.shape[0])
        self.family, self.sigma, self.ell, self.nugget = family, float(sigma), float(ell), float(nugget)
        self.targets, self.sources, self.metric, self.nu = tg, src, G, nu
        self.diag_offset = None if diag_offset is None else int(diag_offset)
        diag = L.KERNEL_NO_DIAGONAL if diag_offset is None else self.diag_offset
        if family == "matern1" or G is not None or nu is not None:      # family, nu and metric (targets and sources alike) of ``KernelCovarianceOperator``
            spec = _kernel_spec(family, src.shape[1], self.sigma, self.ell, self.nugget, G, nu)
            L.call("hfmi_op_kernel_cross_cov" + _spec_suffix(nu), self.ctx.handle, L.ptr(tg), tg.shape[0], L.ptr(src), src.shape[0], src.shape[1],
                   C.byref(spec), diag, C.byref(self._op))
        else:
            L.call("hfmi_op_kernel_cross_cov", self.ctx.handle, L.ptr(tg), tg.shape[0], L.ptr(src), src.shape[0], src.shape[1],
                   L.KERNEL_FAMILIES[family], self.sigma, self.ell, self.nugget, diag, C.byref(self._op))

    def to_dense(self):
        """The same matrix on the host (``kernel_cross_cov_host``)."""
        return kernel_cross_cov_host(self.targets, self.sources, self.family, self.sigma, self.ell, self.nugget, self.diag_offset,
                                     nu=self.nu, metric=self.metric)

    def transpose(self):
        """K(S, T), the operator with the two point sets swapped; only without a diagonal."""
        if self.diag_offset is not None:
            raise ValueError("transpose: only for a cross-covariance without a diagonal (diag_offset is %d)" % self.diag_offset)
        return KernelCrossCovarianceOperator(self.sources, self.targets, self.family, self.sigma, self.ell, ctx=self.ctx, nu=self.nu,
                                             metric=self.metric)

    def transpmult(self, x, y):
        raise NotImplementedError("KernelCrossCovarianceOperator: apply transpose() for K^T")


class KernelCovarianceRowsOperator(DeviceOperator):
    """Rows ``row0 .. row1 - 1`` of a ``KernelCovarianceOperator`` as an operator N -> N (hfmi_op_kernel_cov_rows): those rows of y are
    the rows of C x, bit for bit; an overwriting apply leaves the other rows +0.0, an accumulating one leaves them alone.  An empty
    range is valid.  Made by ``KernelCovarianceOperator.rows`` / ``.sharded``."""

    def __init__(self, points, family, sigma, ell, nugget, row0, row1, ctx=None, *, nu=None, metric=None):
        if family not in L.KERNEL_FAMILIES:
            raise _unknown_family(family)
        nu = _check_nu(family, nu)
        pts = _points_array(points)
        row0, row1 = int(row0), int(row1)
        if not 0 <= row0 <= row1 <= pts.shape[0]:
            raise ValueError("rows %d .. %d do not lie inside 0 .. %d" % (row0, row1, pts.shape[0]))
        G = _check_metric(metric, pts.shape[1])
        super().__init__(ctx, pts.shape[0])
        self.family, self.sigma, self.ell, self.nugget = family, float(sigma), float(ell), float(nugget)
        self.points, self.row0, self.row1, self.metric, self.nu = pts, row0, row1, G, nu
        self.collective = None
        self._hook = self._hook_error = None
        if family == "matern1" or G is not None or nu is not None:
            spec = _kernel_spec(family, pts.shape[1], self.sigma, self.ell, self.nugget, G, nu)
            L.call("hfmi_op_kernel_cov_rows" + _spec_suffix(nu), self.ctx.handle, L.ptr(pts), pts.shape[0], pts.shape[1], C.byref(spec), row0, row1 - row0,
                   C.byref(self._op))
        else:
            L.call("hfmi_op_kernel_cov_rows", self.ctx.handle, L.ptr(pts), pts.shape[0], pts.shape[1], L.KERNEL_FAMILIES[family],
                   self.sigma, self.ell, self.nugget, row0, row1 - row0, C.byref(self._op))

    def to_dense(self):
        """The N x N matrix this operator applies: the slab's rows of C, zeros elsewhere (before any rank sum)."""
        out = np.zeros((self.points.shape[0],) * 2)
        if self.row1 > self.row0:
            out[self.row0:self.row1] = kernel_cov_host(self.points, self.family, self.sigma, self.ell, self.nugget,
                                                       rows=np.arange(self.row0, self.row1), nu=self.nu, metric=self.metric)
        return out

    def _attach_sum(self, collective):
        """The rank SUM of every result block, for this object's lifetime."""
        from .collectives import NativeCollective
        self.collective = collective                    # the communicator outlives the operator that points at it
        if isinstance(collective, NativeCollective):
            L.call("hfmi_op_set_collective", self._op, collective._comm, L.REDUCE_SUM)
            return

        def _cb(user, block_handle):
            try:
                collective.allReduce(MultiVector(ctx=self.ctx, _handle=C.c_void_p(block_handle), _borrowed=True), "sum")
                return 0
            except Exception as exc:  # never let an exception cross the C boundary
                self._hook_error = exc
                return 1

        self._hook = L.POST_APPLY_FN(_cb)
        L.call("hfmi_op_set_post_apply", self._op, self._hook, None)

    def _raise_pending(self):
        if self._hook_error is not None:
            exc, self._hook_error = self._hook_error, None
            raise exc

    def matMvMult(self, X, Y, accumulate=False):
        try:
            super().matMvMult(X, Y, accumulate)
        except L.HfmiError:
            self._raise_pending()
            raise

    def mult(self, x, y):
        try:
            super().mult(x, y)
        except L.HfmiError:
            self._raise_pending()
            raise


def nystrom_extend(cross_op, encoder, d):
    """Nystrom extension of eigenpairs to the targets of ``cross_op``: K(T, S) . encoder . diag(1 / d), a ``MultiVector`` of M rows.
    ``encoder``: the block the eigenvectors are applied through on the sources (M V for an M-orthonormal KLE, V for an orthonormal one);
    ``d``: its eigenvalues, one per vector, none zero."""
    d = np.asarray(d, dtype=np.float64).ravel()
    if d.size != encoder.nvec():
        raise ValueError("nystrom_extend: %d eigenvalues for %d vectors" % (d.size, encoder.nvec()))
    if np.any(d == 0.0):
        raise ZeroDivisionError("nystrom_extend: zero eigenvalue")
    out = MultiVector(cross_op.shape[0], encoder.nvec(), ctx=cross_op.ctx)
    cross_op.matMvMult(encoder, out)
    for j in range(out.nvec()):
        out.view(j, 1).scale(1.0 / d[j])
    return out


def anisotropy_2d(theta0, theta1, alpha):
    """The 2 x 2 anisotropy tensor Theta of a BiLaplacian prior with ``theta0``, ``theta1`` and the angle ``alpha``:

        Theta_00 = theta0 sin^2 alpha + theta1 cos^2 alpha,   Theta_01 = Theta_10 = (theta0 - theta1) sin alpha cos alpha,
        Theta_11 = theta0 cos^2 alpha + theta1 sin^2 alpha.

    This formula IS the definition for this package (it is the one the reference's prior is documented with; that code is not
    available here to compare against).  theta0 and theta1 are its eigenvalues, so both must be positive."""
    theta0, theta1, alpha = float(theta0), float(theta1), float(alpha)
    if not (theta0 > 0.0 and theta1 > 0.0 and np.isfinite(theta0) and np.isfinite(theta1) and np.isfinite(alpha)):
        raise ValueError("anisotropy_2d: theta0 and theta1 must be positive and finite, alpha finite")
    s, c = np.sin(alpha), np.cos(alpha)
    off = (theta0 - theta1) * s * c
    return np.array([[theta0 * s * s + theta1 * c * c, off], [off, theta0 * c * c + theta1 * s * s]])


def bilaplacian_kernel_2d(gamma, delta, theta0=2.0, theta1=0.5, alpha=np.pi / 4):
    """The kernel of the BiLaplacian prior in two dimensions as keyword arguments of the kernel covariance operators: the covariance of
    the precision (delta - gamma div Theta grad)^2 in FREE SPACE is the Matern field of smoothness 1,

        c(x) = sigma^2 (kappa r) K_1(kappa r),   r^2 = x^T Theta^-1 x,   kappa^2 = delta / gamma,
        sigma^2 = 1 / (4 pi delta gamma sqrt(det Theta)),

    that is ``family="matern1"`` (a K_1(a), a = sqrt(2) r / ell) with ``ell = sqrt(2 gamma / delta)`` and ``metric = inv(Theta)``,
    ``Theta = anisotropy_2d(theta0, theta1, alpha)``.  The defaults are those of the reference's ``BiLaplacian2D``.  Splat the result:
    ``GridKernelCovarianceOperator(shape, spacing, **bilaplacian_kernel_2d(gamma, delta))``.  What is NOT in it: the boundary.  A
    finite-element prior on a bounded mesh has Robin or Neumann conditions that raise the variance near the boundary and bend the
    correlations there; this is the kernel of the interior, away from it by a few correlation lengths."""
    gamma, delta = float(gamma), float(delta)
    if not (gamma > 0.0 and delta > 0.0 and np.isfinite(gamma) and np.isfinite(delta)):
        raise ValueError("bilaplacian_kernel_2d: gamma and delta must be positive and finite")
    Theta = anisotropy_2d(theta0, theta1, alpha)
    det = Theta[0, 0] * Theta[1, 1] - Theta[0, 1] * Theta[1, 0]
    inv = np.array([[Theta[1, 1], -Theta[0, 1]], [-Theta[1, 0], Theta[0, 0]]]) / det
    return dict(family="matern1", sigma=1.0 / np.sqrt(4.0 * np.pi * delta * gamma * np.sqrt(det)), ell=np.sqrt(2.0 * gamma / delta), metric=inv)


def whittle_matern_kernel(gamma, delta, alpha, d, Theta=None):
    """The kernel of the precision (delta - gamma div Theta grad)^alpha in d dimensions, in FREE SPACE, as keyword arguments of the
    kernel covariance operators: the Matern field of smoothness nu = alpha - d/2,

        c(x) = sigma^2 2^(1-nu) / Gamma(nu) (kappa r)^nu K_nu(kappa r),   r^2 = x^T Theta^-1 x,   kappa^2 = delta / gamma,
        sigma^2 = Gamma(nu) / (Gamma(alpha) (4 pi)^(d/2) kappa^(2 nu) gamma^alpha sqrt(det Theta)),

    that is ``family="matern"`` with that ``nu``, ``ell = sqrt(2 nu gamma / delta)`` (so that a = sqrt(2 nu) r / ell = kappa r) and
    ``metric = inv(Theta)``.  ``alpha`` need not be an integer; nu must lie in [1/8, 8] (ValueError otherwise).  ``Theta``: a symmetric
    positive definite d x d matrix, None for the identity.  Splat the result:
    ``GridKernelCovarianceOperator(shape, spacing, **whittle_matern_kernel(gamma, delta, 3, 2))``.  For alpha = 2, d = 2 these are the
    numbers of ``bilaplacian_kernel_2d``, which stays the fast way to that kernel (``"matern1"``).  What is NOT in it: the boundary.
    A finite-element prior on a bounded mesh has Robin or Neumann conditions that raise the variance near the boundary and bend the
    correlations there; this is the kernel of the interior, away from it by a few correlation lengths."""
    from scipy.special import gamma as gamma_fn
    gamma, delta, alpha, d = float(gamma), float(delta), float(alpha), int(d)
    if not (gamma > 0.0 and delta > 0.0 and np.isfinite(gamma) and np.isfinite(delta)):
        raise ValueError("whittle_matern_kernel: gamma and delta must be positive and finite")
    if d not in (1, 2, 3):
        raise ValueError("whittle_matern_kernel: d is 1, 2 or 3, got %r" % (d,))
    nu = alpha - 0.5 * d
    if not (np.isfinite(nu) and L.MATERN_NU_MIN <= nu <= L.MATERN_NU_MAX):
        raise ValueError("whittle_matern_kernel: nu = alpha - d/2 = %r does not lie in [%g, %g]" % (nu, L.MATERN_NU_MIN, L.MATERN_NU_MAX))
    Th = _check_metric(np.eye(d) if Theta is None else Theta, d)
    kappa2 = delta / gamma
    var = gamma_fn(nu) / (gamma_fn(alpha) * (4.0 * np.pi) ** (0.5 * d) * kappa2 ** nu * gamma ** alpha * np.sqrt(np.linalg.det(Th)))
    return dict(family="matern", sigma=np.sqrt(var), ell=np.sqrt(2.0 * nu * gamma / delta), nu=nu, metric=np.linalg.inv(Th))


class _Csr:
    def __init__(self, M, ctx):
        import scipy.sparse as sp
        M = sp.csr_matrix(M)
        M.sort_indices()
        self.shape = M.shape
        self.indptr = np.ascontiguousarray(M.indptr, dtype=np.int64)
        self.indices = np.ascontiguousarray(M.indices, dtype=np.int32)
        self.data = np.ascontiguousarray(M.data, dtype=np.float64)
        self.ctx = ctx
        self.handle = C.c_void_p()
        L.call("hfmi_csr_create", ctx.handle, M.shape[0], M.shape[1], int(M.nnz), L.ptr(self.indptr),
               L.ptr(self.indices), L.ptr(self.data), C.byref(self.handle))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                L.load().hfmi_csr_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class CsrOperator(DeviceOperator):
    """Sparse matrix operator y = M x (prior.M, prior.R; the encoder step hp.MatMvMult(B, decoder, encoder))."""

    def __init__(self, M, ctx=None):
        ctx = ctx or L.Context.default()
        self.csr = M if isinstance(M, _Csr) else _Csr(M, ctx)
        super().__init__(ctx, self.csr.shape[0], self.csr.shape[1])
        L.call("hfmi_op_csr", self.ctx.handle, self.csr.handle, C.byref(self._op))


class CsrPCGSolver(DeviceOperator):
    """Solver object for an SPD sparse matrix (prior.Msolver): ``solve(y, x)`` gives y = M^{-1} x to a relative
    residual ``rel_tol`` per vector, on the device; as an operator it IS hp.Solver2Operator(Msolver).  The work is done by a
    Jacobi-preconditioned Chebyshev iteration (hfmi_cheb.hip) when the Jacobi-scaled spectrum is narrow -- mass matrices --
    and by Jacobi-preconditioned block CG otherwise; ``info()`` tells which."""

    def __init__(self, M, rel_tol=1e-13, max_iter=500, ctx=None):
        ctx = ctx or L.Context.default()
        self.csr = M if isinstance(M, _Csr) else _Csr(M, ctx)
        super().__init__(ctx, self.csr.shape[0])
        L.call("hfmi_op_csr_pcg", self.ctx.handle, self.csr.handle, float(rel_tol), int(max_iter), C.byref(self._op))

    def solve(self, y, x):
        self.mult(x, y)

    def info(self):
        """Of the last solve: {'iterations', 'method' ('chebyshev' | 'cg'), 'spectrum' (bracket of D^-1 M in use, or None)}."""
        it, method, lo, hi = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
        L.call("hfmi_op_solver_info", self._op, C.byref(it), C.byref(method), C.byref(lo), C.byref(hi))
        return {"iterations": it.value, "method": "chebyshev" if method.value == 1 else "cg",
                "spectrum": (lo.value, hi.value) if hi.value > 0 else None}


class CsrAMGSolver(DeviceOperator):
    """Solver object for an SPD sparse elliptic matrix (hippylib ``BiLaplacianPrior.Asolver``: PETSc CG preconditioned by
    algebraic multigrid, rel_tol 1e-12): ``solve(y, x)`` gives y = A^{-1} x with every vector's residual at most
    ``rel_tol`` times its right-hand side.  The smoothed-aggregation hierarchy is built once on the host
    (``hippyflow_amd.amg.AMGHierarchy``; ``setup_options`` go there); block CG with one V-cycle as preconditioner runs on the
    device (hfmi_amg.hip).  ValueError for a matrix that cannot be SPD (not square or symmetric, a diagonal entry <= 0,
    non-finite entries); HfmiError NUMERIC / NOT_CONVERGED from a solve that breaks down or runs out of iterations."""

    def __init__(self, A, rel_tol=1e-12, max_iter=100, ctx=None, **setup_options):
        from .amg import AMGHierarchy
        ctx = ctx or L.Context.default()
        csr = csr_from_matrix(A)
        h = AMGHierarchy(csr if csr is not None else A, **setup_options)
        super().__init__(ctx, h.levels[0].A.shape[0])
        self._hierarchy = h
        self._amg = C.c_void_p()
        levels = h.levels
        mats = [_Csr(lv.A, ctx) for lv in levels]
        links = [(_Csr(lv.P, ctx), _Csr(lv.R, ctx)) for lv in levels[:-1]]
        self._keep = mats + [m for pr in links for m in pr]
        L.call("hfmi_amg_create", ctx.handle, mats[0].handle, levels[0].lmin, levels[0].lmax, int(h.degree), C.byref(self._amg))
        for l in range(1, len(levels)):
            P, R = links[l - 1]
            L.call("hfmi_amg_add_level", self._amg, P.handle, R.handle, mats[l].handle, levels[l].lmin, levels[l].lmax)
        inv = np.ascontiguousarray(h.coarse_inv, dtype=np.float64)
        L.call("hfmi_amg_set_coarse", self._amg, int(inv.shape[0]), L.ptr(inv))
        L.call("hfmi_op_amg_pcg", self.ctx.handle, self._amg, float(rel_tol), int(max_iter), C.byref(self._op))
        self.rel_tol, self.max_iter = float(rel_tol), int(max_iter)

    def solve(self, y, x):
        self.mult(x, y)

    def vcycle(self, B, X):
        """X = V B: one V-cycle of the preconditioner on a block (MultiVectors of length N)."""
        L.call("hfmi_amg_vcycle", self._amg, B.handle, X.handle)

    def info(self):
        """Of the last solve: {'iterations', 'method': 'amg-cg'}."""
        it, method = C.c_int(0), C.c_int(0)
        L.call("hfmi_op_solver_info", self._op, C.byref(it), C.byref(method), None, None)
        return {"iterations": it.value, "method": "amg-cg" if method.value == 2 else str(method.value)}

    def hierarchy(self):
        """The host hierarchy (``sizes()``, ``nnz()``, ``operator_complexity()``, ``info()``)."""
        return self._hierarchy

    def __del__(self):
        super().__del__()
        try:
            if getattr(self, "_amg", None):
                L.load().hfmi_amg_destroy(self._amg)
                self._amg = None
        except Exception:
            pass


class HostCallbackOperator(DeviceOperator):
    """A host black box plugged into the device solve (FEniCS/hIPPYlib PDE solves stay on the host).

    ``fn`` is, in this order of preference:

    * numpy fast paths -- a plain callable mapping an (N, k) array to an (N, k) array; an object with
      ``matMvMult_np(X) -> Y`` or (solvers) ``solve_block(X) -> Y`` on (N, k) arrays;
    * the REFERENCE'S OWN PROTOCOL -- an object whose vectors can be shaped (``init_vector(x, dim)`` on the object, on
      its ``operator()`` / ``get_operator()`` as hp.Solver2Operator looks it up, or passed as ``init_vector=``): the
      slab is moved column by column into host vectors made by ``hostvec.new_host_vector`` + that ``init_vector``
      through ``set_local`` and the result read back with ``get_local`` (how collectives/collective.py:98-107 moves
      data), calling ``fn.matMvMult(X, Y)`` with host column lists when the object has the block form (Y arrives
      zeroed: the reference's block operators accumulate, activeSubspaceProjector.py:214-221), else ``fn.mult(x, y)`` /
      ``fn.solve(y, x)`` per column -- so ``prior.R``, ``prior.Rsolver``, ``JTJ(ObservableJacobian(obs))``, PETSc
      matrices and Krylov solvers plug in as they are;
    * objects with ``solve(y, x)`` / ``mult(x, y)`` on 1-D numpy arrays and no ``init_vector`` (numpy test doubles).

    ``chunk_vectors``: for black boxes that treat the vectors independently (solvers), the callback is invoked on
    slabs of that many vectors and the PCIe copies of the neighbouring slabs overlap the host work
    (``hfmi_op_host_set_chunk``).  Default: solver-like objects (``solve`` / ``solve_block``) 32, everything else the
    whole block in one call (a serialized-sampling Jacobian operator re-solves its PDEs on every call)."""

    def __init__(self, fn, N=None, ctx=None, chunk_vectors=None, init_vector=None):
        self.fn = fn
        self.error = None
        solver_like = hasattr(fn, "solve") or hasattr(fn, "solve_block")
        shaper = init_vector
        if shaper is None and not (hasattr(fn, "matMvMult_np") or hasattr(fn, "solve_block")):
            shaper = H.find_init_vector(fn)
        plain_callable = callable(fn) and not hasattr(fn, "mult") and not hasattr(fn, "matMvMult") and not solver_like
        if plain_callable:
            self.mode = "array"
        elif hasattr(fn, "matMvMult_np"):
            self.mode = "block_np"
        elif hasattr(fn, "solve_block"):
            self.mode = "solve_np"
        elif shaper is not None:
            self.mode = "block" if hasattr(fn, "matMvMult") else ("solve" if hasattr(fn, "solve") else "mult")
        else:
            self.mode = "solve_1d" if hasattr(fn, "solve") else "mult_1d"
        self._shaper = shaper
        self._x = self._y = None           # host vectors, shaped on first use (domain, range)
        if N is None:
            if shaper is None:
                raise ValueError("HostCallbackOperator: the vector length is needed to wrap an operator without init_vector")
            N = H.shape_with(shaper, 0, self._comm()).size()
        super().__init__(ctx, N)

        def _cb(user, w_ptr, y_ptr, n, k):
            try:
                W = np.ctypeslib.as_array(w_ptr, shape=(k, n))    # one vector per row
                Y = np.ctypeslib.as_array(y_ptr, shape=(k, n))
                self._apply_rows(W, Y)
                return 0
            except Exception as exc:  # never let an exception cross the C boundary
                self.error = exc
                return 1

        self._cb = L.HOST_APPLY_FN(_cb)
        L.call("hfmi_op_host_callback", self.ctx.handle, self._cb, None, int(N), C.byref(self._op))
        if chunk_vectors is None:
            chunk_vectors = 32 if solver_like else 0
        self.chunk_vectors = int(chunk_vectors)
        if self.chunk_vectors:
            L.call("hfmi_op_host_set_chunk", self._op, self.chunk_vectors)

    def _comm(self):
        try:
            return self.fn.mpi_comm() if hasattr(self.fn, "mpi_comm") and callable(self.fn.mpi_comm) else None
        except Exception:          # noqa: BLE001
            return None

    def _host_pair(self):
        if self._x is None:
            comm = self._comm()
            # a solver maps the range of its operator back to the domain: both shapes coincide on this (square) path
            self._x = H.shape_with(self._shaper, 1, comm)
            self._y = H.shape_with(self._shaper, 0, comm)
        return self._x, self._y

    def _apply_rows(self, W, Y):
        fn, mode = self.fn, self.mode
        if mode == "array":
            Y[...] = np.asarray(fn(W.T)).T
        elif mode == "block_np":
            Y[...] = np.asarray(fn.matMvMult_np(W.T)).T
        elif mode == "solve_np":
            Y[...] = np.asarray(fn.solve_block(W.T)).T
        elif mode == "block":
            x, y = self._host_pair()
            X, Yh = H.HostMultiVector(x, W.shape[0]), H.HostMultiVector(y, W.shape[0])
            for j in range(W.shape[0]):
                X[j].set_local(W[j])
                X[j].apply("")
            fn.matMvMult(X, Yh)
            for j in range(W.shape[0]):
                Y[j] = Yh[j].get_local()
        elif mode in ("mult", "solve"):
            x, y = self._host_pair()
            for j in range(W.shape[0]):
                x.set_local(W[j])
                x.apply("")
                if mode == "mult":
                    fn.mult(x, y)
                else:
                    fn.solve(y, x)
                Y[j] = y.get_local()
        elif mode == "solve_1d":
            for j in range(W.shape[0]):
                fn.solve(Y[j], W[j])
        else:
            for j in range(W.shape[0]):
                fn.mult(W[j], Y[j])

    def _raise_pending(self):
        if self.error is not None:
            exc, self.error = self.error, None
            raise exc

    def matMvMult(self, X, Y, accumulate=False):
        try:
            super().matMvMult(X, Y, accumulate)
        except L.HfmiError:
            self._raise_pending()
            raise

    def mult(self, x, y):
        try:
            super().mult(x, y)
        except L.HfmiError:
            self._raise_pending()
            raise

    def solve(self, y, x):
        self.mult(x, y)


class DenseJacobianOperator:
    """A stored Jacobian J (q x N) behind the reference's rectangular-operator protocol
    (ObservableJacobian: ``mult`` N -> q, ``transpmult`` q -> N, ``init_vector(x, dim)``; jacobian.py:62-139).
    The rows of J are the vectors of a block, so J W is a ``dot_mv`` (reduction over N) and J^T Y an ``MvDSmatMult``."""

    def __init__(self, J, ctx=None):
        self.rows = J if isinstance(J, MultiVector) else MultiVector.from_vectors(np.asarray(J, dtype=np.float64), ctx=ctx)
        self.ctx = self.rows.ctx
        self.shape = (self.rows.nvec(), self.rows.size())

    def mpi_comm(self):
        from .multivector import _NullComm
        return _NullComm()

    def init_vector(self, x, dim):
        if dim not in (0, 1):
            raise ValueError("dim must be 0 or 1")
        x.init(self.shape[dim])

    def matMvMult(self, X, Y):          # Y (q x k) = J X
        Y_dense = self.rows.dot_mv(X)                    # (q, k)
        L.call("hfmi_block_upload", Y.handle, L.ptr(np.ascontiguousarray(Y_dense)), L.LAYOUT_DENSE)

    def matMvTranspmult(self, X, Y):    # Y (N x k) = J^T X
        from .multivector import MvDSmatMult
        MvDSmatMult(self.rows, np.ascontiguousarray(X.to_dense()), Y)

    def mult(self, x, y):
        self.matMvMult(x._mv, y._mv)

    def transpmult(self, x, y):
        self.matMvTranspmult(x._mv, y._mv)


class ComposedOperator(DeviceOperator):
    """y = c(b(a x))."""

    def __init__(self, a, b, c):
        super().__init__(a.ctx, c.shape[0], a.shape[1])
        self._keep = [a, b, c]
        L.call("hfmi_op_compose3", self.ctx.handle, a._op, b._op, c._op, C.byref(self._op))


class BiLaplacianRsolver(ComposedOperator):
    """Device ``prior.Rsolver`` of a bi-Laplacian prior: R^-1 = A^-1 M A^-1, with A = delta M + gamma K solved by ONE
    ``CsrAMGSolver`` (its hierarchy shared by both solves) and M either the consistent mass matrix (hippylib's form) or a
    diagonal given as a 1-D array (the lumped form of ``workloads.BiLaplacianPrior``).  ``solve(y, x)`` is hippylib's
    solver protocol, so it plugs in as ``prior.Rsolver`` and behind ``Solver2Operator``.

    ``rel_tol`` defaults to 1e-14, tighter than hippylib's 1e-12 for ``Asolver``: doublePassG(A, R, R^-1, ...) orthonormalises
    R^-1 Y in the R inner product, and what a solve leaves in the high-frequency modes is amplified there by ||R|| ~ 1e10
    (1e-12 gave an R-orthonormality defect 40x the sparse-LU route's at N = 5e4; 1e-14 costs about three more iterations)."""

    def __init__(self, A, M, rel_tol=1e-14, max_iter=100, ctx=None, **setup_options):
        import scipy.sparse as sp
        ctx = ctx or L.Context.default()
        self.Asolver = A if isinstance(A, CsrAMGSolver) else CsrAMGSolver(A, rel_tol=rel_tol, max_iter=max_iter, ctx=ctx, **setup_options)
        if isinstance(M, DeviceOperator):
            self.Mop = M
        else:
            Mcsr = csr_from_matrix(M)
            if Mcsr is None:
                Mcsr = sp.diags(np.asarray(M, dtype=np.float64).ravel()).tocsr()
            self.Mop = CsrOperator(Mcsr, ctx=ctx)
        if self.Mop.shape != self.Asolver.shape:
            raise ValueError("BiLaplacianRsolver: M is %s, A is %s" % (self.Mop.shape, self.Asolver.shape))
        super().__init__(self.Asolver, self.Mop, self.Asolver)
        self.N = self.Asolver.shape[0]

    def solve(self, y, x):
        self.mult(x, y)

    def info(self):
        """Of the second A-solve of the last apply."""
        return self.Asolver.info()


def device_bilaplacian_rsolver(prior, rel_tol=1e-14, max_iter=100, ctx=None, **setup_options):
    """``BiLaplacianRsolver`` from a prior's ``A`` and ``M`` (hippylib ``BiLaplacianPrior``'s attribute names; scipy, PETSc
    or dolfin matrices, through ``csr_from_matrix``).  A prior that carries ``M_lumped`` (``workloads.BiLaplacianPrior``,
    R = A M_l^-1 A) gets that diagonal.  A driver swaps it in with ``prior.Rsolver = device_bilaplacian_rsolver(prior)``."""
    A = csr_from_matrix(prior.A)
    if A is None:
        raise TypeError("device_bilaplacian_rsolver: prior.A is not an assembled matrix (%r)" % (type(prior.A),))
    M = getattr(prior, "M_lumped", None)
    if M is None:
        M = csr_from_matrix(prior.M)
        if M is None:
            raise TypeError("device_bilaplacian_rsolver: prior.M is not an assembled matrix (%r)" % (type(prior.M),))
    return BiLaplacianRsolver(A, M, rel_tol=rel_tol, max_iter=max_iter, ctx=ctx, **setup_options)


def csr_from_matrix(M):
    """scipy CSR from the kinds of assembled matrices a prior carries: a scipy sparse matrix, a PETSc matrix
    (``getValuesCSR()``, the call the reference itself uses to export matrices, PODProjector.py:322-324), a dolfin
    matrix (``.mat()`` of its PETSc backend).  None when ``M`` is none of these."""
    import scipy.sparse as sp
    if sp.issparse(M):
        return sp.csr_matrix(M)
    for unwrap in (lambda m: m, lambda m: m.mat(), _dolfin_backend_mat):
        try:
            petsc = unwrap(M)
            indptr, indices, data = petsc.getValuesCSR()
        except Exception:          # noqa: BLE001 -- not that kind of matrix
            continue
        n_rows = len(indptr) - 1
        n_cols = petsc.getSize()[1] if hasattr(petsc, "getSize") else n_rows
        return sp.csr_matrix((np.asarray(data, dtype=np.float64), np.asarray(indices), np.asarray(indptr)), shape=(n_rows, n_cols))
    return None


def _dolfin_backend_mat(M):
    import dolfin
    return dolfin.as_backend_type(M).mat()


def as_device_operator(obj, N=None, ctx=None, init_vector=None):
    """Coerce the kinds of objects the reference passes as A / B / B^{-1} into device operators: device operators
    and adapters as they are, assembled matrices (scipy / PETSc / dolfin) as CSR in HBM, dense symmetric arrays, and
    every other operator or solver as a host callback -- through the reference's vector protocol when its vectors
    can be shaped (``init_vector`` on the object or passed in), on numpy slices otherwise."""
    if isinstance(obj, DeviceOperator):
        return obj
    if hasattr(obj, "_device_operator"):
        return obj._device_operator()
    if isinstance(obj, np.ndarray) and obj.ndim == 2:
        return npToDeviceOperator(obj, ctx=ctx)
    if hasattr(obj, "getValuesCSR") or hasattr(obj, "mat") or hasattr(obj, "tocsr"):
        csr = csr_from_matrix(obj)
        if csr is not None:
            return CsrOperator(csr, ctx=ctx)
    if callable(obj) or any(hasattr(obj, m) for m in ("mult", "solve", "matMvMult", "matMvMult_np", "solve_block")):
        return HostCallbackOperator(obj, N, ctx=ctx, init_vector=init_vector)
    raise TypeError("cannot use %r as an operator" % (type(obj),))


class Solver2Operator:
    """hp.Solver2Operator(S): ``mult(x, y)`` = ``S.solve(y, x)`` (KLEProjector.py:103)."""

    def __init__(self, solver, mpi_comm=None, init_vector=None):
        self.solver = solver
        self._mpi_comm = mpi_comm
        self._init_vector = init_vector or H.find_init_vector(solver)

    def mpi_comm(self):
        return self._mpi_comm

    def init_vector(self, x, dim):
        if self._init_vector is None:
            raise NotImplementedError("Solver2Operator: no init_vector available")
        self._init_vector(x, dim)

    def mult(self, x, y):
        self.solver.solve(y, x)

    def _device_operator(self):
        s = self.solver
        return s if isinstance(s, DeviceOperator) else as_device_operator(s, getattr(s, "N", None), init_vector=self._init_vector)


# ======================================================================================================================
# The reference's small adapter classes (same names, constructor arguments and duck types).  They are written around
# three helpers: a chain of maps through scratch vectors, a weighted sum of operator applications, and a retrying
# sample loop.  Every one of them works on device vectors / blocks and on host (dolfin-like) vectors alike: only
# ``zero``, ``axpy`` and the block members ``dot_v`` / ``reduce`` are used.
# ======================================================================================================================
def _scratch(like_init, dim, ctx=None):
    """A work vector shaped by an operator's ``init_vector``: in HBM when the owner lives on the device (it has a
    context), else a host vector of the kind the host operator expects."""
    if ctx is None:
        return H.shape_with(like_init, dim)
    v = Vector(ctx=ctx)
    like_init(v, dim)
    return v


def _run_chain(steps, x, y, scratch):
    """y = steps[-1](... steps[0](x)): each step is ``f(src, dst)``, intermediates live in ``scratch``."""
    src = x
    for f, dst in zip(steps[:-1], scratch):
        f(src, dst)
        src = dst
    steps[-1](src, y)


def _weighted_sum(applications, y, weight, make_like):
    """y = weight * sum of f(tmp) over ``applications`` (each fills ``tmp``); the accumulator starts from zero."""
    tmp, acc = make_like(y), make_like(y)
    acc.zero()
    for f in applications:
        f(tmp)
        acc.axpy(1.0, tmp)
    y.zero()
    y.axpy(weight, acc)


def _low_rank_apply(left, weights, right, x, y):
    """y = left diag(weights) right^T x."""
    coeff = right.dot_v(x)
    y.zero()
    left.reduce(y, coeff if weights is None else weights * coeff)


class MassPreconditionedCovarianceOperator:
    """M C M (KLEProjector.py:47-69).  On the device the three factors are composed into one operator; called with host
    vectors it runs the chain there."""

    def __init__(self, C, M):
        self.C, self.M = C, M
        self._dev = None
        self._host_scratch = None

    def mpi_comm(self):
        return self.M.mpi_comm()

    def init_vector(self, x, dim):
        self.M.init_vector(x, dim)

    def _device_operator(self):
        if self._dev is None:
            Md = as_device_operator(self.M)
            self._dev = ComposedOperator(Md, as_device_operator(self.C, Md.shape[0], Md.ctx), Md)
        return self._dev

    def mult(self, x, y):
        if H.is_host_vector(x):
            if self._host_scratch is None:
                self._host_scratch = [H.shape_with(self.M.init_vector, 0), H.shape_with(self.M.init_vector, 0)]
            _run_chain([self.M.mult, self.C.mult, self.M.mult], x, y, self._host_scratch)
        else:
            self._device_operator().mult(x, y)

    def matMvMult(self, X, Y):
        self._device_operator().matMvMult(X, Y)


class SummedListOperator:
    """Mean (``average``) or sum of operators of one shape (activeSubspaceProjector.py:69-95).  The accumulator starts
    from zero; the reference seeds it with the incoming y (:83-86), which is a mean only when y arrives zero-filled
    (SURVEY.md section 3.6)."""

    def __init__(self, operators, communicator=None, average=True):
        assert type(operators) is list
        self.operators = operators
        self.average = average

    def _weight(self):
        return 1.0 / float(len(self.operators)) if self.average else 1.0

    def init_vector(self, x, dim=0):
        self.operators[0].init_vector(x, dim)

    def mult(self, x, y):
        _weighted_sum([lambda t, op=op: op.mult(x, t) for op in self.operators], y, self._weight(), H._copy_vector if H.is_host_vector(y) else Vector)

    def matMvMult(self, X, Y):
        from .multivector import MatMvMult
        make = H.HostMultiVector if isinstance(Y, H.HostMultiVector) else MultiVector
        _weighted_sum([lambda T, op=op: MatMvMult(op, X, T) for op in self.operators], Y, self._weight(), make)


class StateSpaceIdentityOperator:
    """The observation operator of a full-state observable (fullStateObservable.py:18-52): the identity, whose adjoint
    in the M inner product is M itself unless ``use_mass_matrix`` is off."""

    def __init__(self, M, use_mass_matrix=True):
        self.M = M
        self.use_mass_matrix = use_mass_matrix

    def mpi_comm(self):
        return self.M.mpi_comm()

    def init_vector(self, v, dim):
        return self.M.init_vector(v, dim)

    @staticmethod
    def _copy(src, dst):
        dst.zero()
        dst.axpy(1.0, src)

    def mult(self, u, y):
        self._copy(u, y)

    def transpmult(self, x, p):
        if not self.use_mass_matrix:
            self._copy(x, p)
        else:
            getattr(self.M, "transpmult", self.M.mult)(x, p)          # M is symmetric


class Jacobian:
    """The interface a Jacobian offers (jacobian.py:19-60): ``init_vector(x, dim)`` with dim 0 = range and 1 = domain,
    ``mpi_comm()``, ``mult(x, y)``, ``transpmult(x, y)``.  A user-written Jacobian deriving from this plugs into ``JTJ`` / ``JJT``
    and the projectors' ``jacobian_factory`` like ``ObservableJacobian`` does."""

    def _missing(self, what):
        raise NotImplementedError("%s.%s: a Jacobian implements init_vector, mpi_comm, mult and transpmult"
                                  % (type(self).__name__, what))

    def init_vector(self, x, dim):
        self._missing("init_vector")

    def mpi_comm(self):
        self._missing("mpi_comm")

    def mult(self, x, y):
        self._missing("mult")

    def transpmult(self, x, y):
        self._missing("transpmult")


class ObservableJacobian(Jacobian):
    """Matrix-free Jacobian of the parameter-to-observable map at the observable's current linearisation point
    (jacobian.py:62-139), through the reference's own calls: ``mult`` is ``applyC -> solveFwdIncremental -> applyB`` and a
    sign, ``transpmult`` is ``applyBt -> solveAdjIncremental -> applyCt`` and a sign.  Everything stays on the host, in
    vectors the observable generated."""

    domain = H.PARAMETER                 # the variable the derivative is taken in
    domain_dim = 1                       # what observable.init_vector calls that space
    c_block = ("applyC", "applyCt")      # the observable's calls for d(residual)/d(domain variable) and its transpose

    def __init__(self, observable):
        self.observable = observable
        for name in self.c_block:
            assert hasattr(observable, name), "the observable must have attribute %s" % name
        self.ncalls = 0
        gen = observable.generate_vector
        self._rhs = {False: gen(H.STATE), True: gen(H.ADJOINT)}         # right-hand side of the incremental solve
        self._inc = {False: gen(H.STATE), True: gen(H.ADJOINT)}         # its solution
        q_like = H.new_host_vector(self.mpi_comm())
        observable.B.init_vector(q_like, 0)
        self.shape = (len(q_like.get_local()), len(gen(self.domain).get_local()))

    def mpi_comm(self):
        return self.observable.B.mpi_comm()

    def init_vector(self, x, dim):
        if dim not in (0, 1):
            raise ValueError("dim must be 0 (observable space) or 1 (the space of the derivative's variable)")
        self.observable.init_vector(x, 0 if dim == 0 else self.domain_dim)

    def _through(self, adjoint, into_rhs, solve, out_of_solution, x, y):
        into_rhs(x, self._rhs[adjoint])
        solve(self._inc[adjoint], self._rhs[adjoint])
        out_of_solution(self._inc[adjoint], y)
        y *= -1.0
        self.ncalls += 1

    def mult(self, x, y):
        obs = self.observable
        assert hasattr(obs, 'applyB'), 'LinearObservable must have attribute applyB'
        self._through(False, getattr(obs, self.c_block[0]), obs.solveFwdIncremental, obs.applyB, x, y)

    def transpmult(self, x, y):
        obs = self.observable
        assert hasattr(obs, 'applyBt'), 'LinearObservable must have attribute applyBt'
        self._through(True, obs.applyBt, obs.solveAdjIncremental, getattr(obs, self.c_block[1]), x, y)

    def rows(self, out=None):
        """The Jacobian as a dense (q, N) array, one adjoint solve per row (J^T e_i): how a sample's linearisation is
        materialised for the device when q is below the number of operator applications it would otherwise cost."""
        q, n = self.shape
        out = np.empty((q, n)) if out is None else out
        e, row = H.shape_with(self.init_vector, 0, self.mpi_comm()), H.shape_with(self.init_vector, 1, self.mpi_comm())
        unit = np.zeros(q)
        for i in range(q):
            unit[i] = 1.0
            e.set_local(unit)
            e.apply("")
            unit[i] = 0.0
            self.transpmult(e, row)
            out[i] = row.get_local()
        return out

    def dense(self):
        """The same array by whichever side is shorter: rows (adjoint solves) or, for a small domain such as a control
        variable, columns (one forward incremental solve each, J e_j)."""
        q, n = self.shape
        if q <= n:
            return self.rows()
        out = np.empty((q, n))
        e, col = H.shape_with(self.init_vector, 1, self.mpi_comm()), H.shape_with(self.init_vector, 0, self.mpi_comm())
        unit = np.zeros(n)
        for j in range(n):
            unit[j] = 1.0
            e.set_local(unit)
            e.apply("")
            unit[j] = 0.0
            self.mult(e, col)
            out[:, j] = col.get_local()
        return out


class ObservableControlJacobian(ObservableJacobian):
    """The same with respect to the CONTROL variable of a control problem (controlJacobian.py:21-95): ``applyCz`` /
    ``applyCzt`` in place of ``applyC`` / ``applyCt``, vectors of the control space (``observable.init_vector(x, 3)``)."""

    domain = H.CONTROL
    domain_dim = 3
    c_block = ("applyCz", "applyCzt")


class _NormalOperator:
    """J^T J or J J^T of a Jacobian-protocol object (``mult`` parameter -> observable, ``transpmult`` back,
    ``init_vector(x, dim)``); jacobian.py:142-193.  With a block-capable Jacobian (``DenseJacobianOperator``) the block
    form is two tall-skinny contractions."""

    inner_dim = None       # the space the intermediate vector lives in: 0 observable (JTJ), 1 parameter (JJT)

    def __init__(self, J):
        self.J = J
        self.vector_help = _scratch(J.init_vector, self.inner_dim, getattr(J, "ctx", None))

    def _steps(self, block=False):
        first, second = ("matMvMult", "matMvTranspmult") if block else ("mult", "transpmult")
        fs = (getattr(self.J, first), getattr(self.J, second))
        return fs if self.inner_dim == 0 else fs[::-1]

    def mult(self, x, y):
        _run_chain(list(self._steps()), x, y, [self.vector_help])

    def init_vector(self, x, dim=None):
        self.J.init_vector(x, 1 - self.inner_dim)

    def matMvMult(self, X, Y):
        """Y = op X (overwrites Y, the semantics of hp.MatMvMult on an operator without a block form)."""
        if hasattr(self.J, "matMvMult") and hasattr(self.J, "matMvTranspmult"):
            _run_chain(list(self._steps(block=True)), X, Y, [MultiVector(self.vector_help, X.nvec())])
        else:
            for j in range(X.nvec()):
                self.mult(X[j], Y[j])


class JTJ(_NormalOperator):
    """J^T J (jacobian.py:142-166)."""
    inner_dim = 0


class JJT(_NormalOperator):
    """J J^T (jacobian.py:169-193)."""
    inner_dim = 1


def default_jacobian_factory(observable):
    """What ``SeriallySampledJacobianOperator`` linearises with: the reference hard-wires ``ObservableJacobian``
    (activeSubspaceProjector.py:178-181); observables that hold their Jacobian in HBM offer ``jacobian()``."""
    if hasattr(observable, "jacobian"):
        return observable.jacobian()
    return ObservableJacobian(observable)


class SeriallySampledJacobianOperator:
    """Sample-by-sample accumulation of J^T J (or J J^T) over prior draws (activeSubspaceProjector.py:98-257).

    The PDE work stays behind the duck-typed ``observable`` exactly as in the reference: per sample ``noise`` is drawn,
    ``prior.sample(noise, m)``, the control (if any), ``solveFwd``, ``setLinearizationPoint``; then the linearised map
    ``jacobian_factory(observable)`` is applied to the whole probe block.  ``matMvMult`` ACCUMULATES into y (:214-221,
    :242-248): callers hand it a zeroed block, as ``MatrixMultCollectiveOperator`` + ``doublePass`` do.  A failing
    forward solve is answered with a fresh draw, as upstream (:180-211, whose ``while not solved`` has no exit) -- at most
    ``max_solver_retries`` times per sample here.

    Called with DEVICE blocks and a host observable, each sample's Jacobian is materialised row by row
    (``ObservableJacobian.rows``: q adjoint solves instead of the 2 k incremental solves of the column loop) into a pinned
    buffer, shipped to HBM on the ingest stream and contracted there while the host solves the next sample
    (``materialize`` = None: whenever q <= 2 k; True / False force it)."""

    def __init__(self, observable, noise, prior, control_distribution=None, operation='JTJ', nsamples=None, ms=None, zs=None,
                 communicator=None, average=True, jacobian_factory=None, materialize=None):
        assert operation in ['JTJ', 'JJT']
        assert (nsamples is not None) or (ms is not None)
        self.observable, self.noise, self.prior = observable, noise, prior
        self.control_distribution = control_distribution
        self.operation = operation
        self.nsamples = nsamples
        self.average = average
        self.ms = ms
        self.zs = zs if zs is not None else (len(ms) * [None] if type(ms) is list else None)
        self.jacobian_factory = jacobian_factory or default_jacobian_factory
        self.materialize = materialize
        self.max_solver_retries = 100         # fresh draws per sample before a failing forward solve is reported
        self.solver_failures = 0              # failed forward solves so far (each was followed by a fresh draw)
        self.samples_linearized = 0
        gen = getattr(observable, "generate_vector", None)
        projected = hasattr(getattr(observable, "problem", None), 'parameter_projection')
        self.u = gen(H.STATE) if gen else None
        if gen and projected:                 # the sample lives on the prior's space and is projected for the PDE (:131-137)
            self.m = H.shape_with(prior.init_vector, 0, communicator)
        else:
            self.m = gen(H.PARAMETER) if gen else None
        self.z = None if control_distribution is None else gen(H.CONTROL)

    def init_vector(self, x, dim=None):
        if self.operation == 'JJT':
            self.observable.init_vector(x, 0)
        elif hasattr(getattr(self.observable, "problem", None), 'parameter_projection'):
            self.prior.init_vector(x, 0)
        else:
            self.observable.init_vector(x, 1)

    # ---- one linearisation point
    def _linearize(self, m, z):
        point = [self.u, m, None] if z is None else [self.u, m, None, z]
        problem = getattr(self.observable, "problem", None)
        if hasattr(problem, 'parameter_projection') and m is self.m:
            point[1] = problem.parameter_projection(m)
        self.observable.solveFwd(self.u, point)
        self.observable.setLinearizationPoint(point)
        self.samples_linearized += 1

    def _draw_and_linearize(self):
        from .randomized import parRandom
        last = None
        for _ in range(self.max_solver_retries + 1):
            self.m.zero()
            self.noise.zero()
            parRandom.normal(1, self.noise)
            self.prior.sample(self.noise, self.m)
            if self.control_distribution is not None:
                self.z.zero()
                self.control_distribution.sample(self.z)
            try:
                return self._linearize(self.m, self.z)
            except Exception as exc:          # noqa: BLE001 -- any solver failure means "draw again", as upstream
                self.solver_failures += 1
                last = exc
        raise RuntimeError("forward solve failed for %d consecutive draws of one sample (last error: %r)"
                           % (self.max_solver_retries + 1, last)) from last

    def _points(self):
        """One linearisation per item: fresh draws, or the given ``ms`` (the reference's unit-test path, :223-248)."""
        if self.ms is None:
            for _ in range(self.nsamples):
                self._draw_and_linearize()
                yield
        else:
            for m, z in zip(self.ms, self.zs):
                self._linearize(m, z)
                yield

    # ---- the accumulation
    def matMvMult(self, x, y):
        assert x.nvec() == y.nvec(), "x and y have non-matching number of vectors"
        count = self.nsamples if self.ms is None else len(self.ms)
        weight = 1.0 / count if self.average else 1.0
        normal = JTJ if self.operation == 'JTJ' else JJT
        on_device = isinstance(x, MultiVector)
        J = None
        stager = None
        for _ in self._points():
            J = self.jacobian_factory(self.observable) if (J is None or not isinstance(J, ObservableJacobian)) else J
            if on_device and isinstance(J, ObservableJacobian):
                if stager is None:
                    stager = _JacobianStager(J, x.ctx, self.materialize, x.nvec())
                stager.accumulate(normal, x, y, weight)
                continue
            op = normal(J)
            if on_device:
                tmp = MultiVector(y)
                op.matMvMult(x, tmp)
                y.axpy(weight, tmp)
            else:                             # host column lists: the reference's loop (:214-221)
                tmp = H._copy_vector(y[0])
                for j in range(x.nvec()):
                    tmp.zero()
                    op.mult(x[j], tmp)
                    y[j].axpy(weight, tmp)
        if stager is not None:
            stager.finish()


class _JacobianStager:
    """Device accumulation of w J^T J X (or w J J^T X) for a HOST Jacobian.  Materialising route: the q rows of J go
    through one of two pinned buffers to a (q x N) block in HBM on the ingest stream, and the two contractions are enqueued
    on the solve's stream as a one-sample ``hfmi_op_jtj`` / ``hfmi_op_jjt`` accumulating into Y -- nothing waits for them:
    the host is already solving for the next sample's rows.  Column route (q > 2 k): the probe block is downloaded once
    and each column goes through ``mult`` / ``transpmult`` on host vectors."""

    def __init__(self, J, ctx, materialize, k):
        self.J, self.ctx = J, ctx
        q, n = J.shape
        self.q, self.n = q, n
        self.materialize = (q <= 2 * k) if materialize is None else bool(materialize)
        self._i = 0
        if self.materialize:
            self._pinned = [L.pinned_empty((q, n)) for _ in range(2)]
            self._blocks = [MultiVector(n, q, ctx=ctx) for _ in range(2)]
            self._tickets = [None, None]
            self._ops = [None, None]          # the operator reading block b: alive until its kernels have run
        else:
            self._x_host = None

    def accumulate(self, normal, X, Y, weight):
        if not self.materialize:
            return self._columns(normal, X, Y, weight)
        b = self._i % 2
        self._i += 1
        if self._tickets[b] is not None:
            self.ctx.ingest_wait(self._tickets[b])   # the pinned buffer has been read
            self.ctx.synchronize()                   # and the contraction that used this block two samples ago has run
        self.J.rows(self._pinned[b])                 # q adjoint solves on the host
        self._tickets[b] = self._blocks[b].upload_async(self._pinned[b])
        self.ctx.ingest_fence()
        if normal is JTJ:
            op = MeanJTJfromDataOperator.from_block(self._blocks[b], 1, self.q, scale=weight)
        else:
            op = MeanJJTfromDataOperator((self._blocks[b], 1, self.q), scale=weight)
        op.matMvMult(X, Y, accumulate=True)
        self._ops[b] = op

    def _columns(self, normal, X, Y, weight):
        op = normal(self.J)
        if self._x_host is None:
            self._x_host = X.to_vectors()
        dim_in = 1 if normal is JTJ else 0
        xin = H.shape_with(self.J.init_vector, dim_in, self.J.mpi_comm())
        yout = H.shape_with(self.J.init_vector, dim_in, self.J.mpi_comm())
        out = np.empty_like(self._x_host)
        for j in range(self._x_host.shape[0]):
            xin.set_local(self._x_host[j])
            xin.apply("")
            op.mult(xin, yout)
            out[j] = yout.get_local()
        Y.axpy(weight, MultiVector.from_vectors(out, ctx=self.ctx))

    def finish(self):
        if self.materialize:
            for t in self._tickets:
                if t is not None:
                    self.ctx.ingest_wait(t)
            self.ctx.synchronize()
            self._ops = [None, None]


class PriorPreconditionedProjector:
    """x -> U U^T C^{-1} x (priorPreconditionedProjector.py:19-55)."""

    def __init__(self, U, Cinv, my_init_vector):
        self.U, self.Cinv = U, Cinv
        self.my_init_vector = my_init_vector
        self.Cinvx = _scratch(my_init_vector, 0, getattr(U, "ctx", None))

    def init_vector(self, x, dim):
        self.my_init_vector(x, dim)

    def mult(self, x, y):
        self.Cinv.mult(x, self.Cinvx)
        _low_rank_apply(self.U, None, self.U, self.Cinvx, y)


class LowRankRectangularOperator:
    """U diag(s) V^T and its transpose (lowRankRectangularOperator.py:17-66)."""

    def __init__(self, U, s, V, U_init_vector=None, V_init_vector=None):
        self.U, self.s, self.V = U, np.asarray(s, dtype=np.float64), V
        self._shapers = (U_init_vector, V_init_vector)
        self.U_init_vector, self.V_init_vector = U_init_vector, V_init_vector

    def init_vector(self, x, dim):
        if dim not in (0, 1):
            raise ValueError("dim must be 0 or 1")
        assert self._shapers[dim] is not None
        self._shapers[dim](x)

    def mult(self, x, y):
        _low_rank_apply(self.U, self.s, self.V, x, y)

    def transpmult(self, x, y):
        _low_rank_apply(self.V, self.s, self.U, x, y)


# the reference's name for the dense-array operator wrapper (operatorWrappers.py:19-52)
npToDolfinOperator = npToDeviceOperator
