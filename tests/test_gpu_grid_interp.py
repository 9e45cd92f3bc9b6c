"""Scattered points on the FFT route on the device: ``GridInterpolationOperator`` (W, W^T), ``InterpolatedKernelCovarianceOperator``
(K = W Cg W^T + diag(delta)) and ``InterpolatedFieldSampler`` (hfmi_interp.hip) against the numpy twin (tests/helpers/interp_twin.py)
with the operator's own weights.  The device is held to K at rounding level; K - C is checked on the CPU (test_grid_interp_cpu.py).

Accumulating applies: the kernels form the result and then add it to what the block holds, so an accumulating apply is checked to
equal ``before + (the overwriting result)`` bit for bit; the rounding bounds are asserted on the overwriting results."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import interp_twin as tw                          # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = tw.EPS
SIGMA = 1.3
COLUMNS = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def _points(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "d1":        # n = 9, N = 7: both edge points (u = 1 and u = n - 2 exactly: dyadic spacing), two points in one cell, a node
        shape, h, o = (9,), (0.25,), (1.0,)
        u = np.array([[1.0], [7.0], [3.25], [3.75], [5.0], [2.6], [6.1]])
    elif name == "d2":      # 9 x 6, N = 23, 12 of the points in the cell (4, 2)
        shape, h, o = (9, 6), (0.1, 0.13), (0.3, -0.2)
        u = np.concatenate([np.array([4.0, 2.0]) + rng.random((12, 2)), 1.0 + rng.random((11, 2)) * (np.array(shape) - 3)])
        u = u[rng.permutation(23)]
    elif name == "d3":      # 6 x 5 x 7, N = 40
        shape, h, o = (6, 5, 7), (0.07, 0.1, 0.09), (-1.0, 0.25, 2.0)
        u = 1.0 + rng.random((40, 3)) * (np.array(shape) - 3)
    else:                   # 70 x 67, N = 5000 in no order: several workgroups of points and of nodes, several chunks with "fftcov_pairs"
        shape, h, o = (70, 67), (1.0 / 64, 1.0 / 60), (-0.02, 0.1)
        u = 1.0 + rng.random((5000, 2)) * (np.array(shape) - 3)
    return shape, h, o, np.ascontiguousarray(np.asarray(o) + u * np.asarray(h))


KERNELS = {"d1": ("matern32", 1.0, 0.0), "d2": ("matern52", 0.45, 0.01), "d3": ("sqexp", 0.3, 0.02), "big": ("matern52", 0.2, 0.0)}
CASES = ("d1", "d2", "d3", "big")


@functools.lru_cache(maxsize=None)
def twin_dense(name):
    """(W, Cg, ||W||_2, ||Cg||_2) of a case, computed once"""
    shape, h, o, pts = _points(name)
    family, ell, _ = KERNELS[name]
    base, w, _ = tw.cell_and_weights(shape, h, o, pts)
    W = tw.dense_W(shape, base, w)
    Cg = hf.kernel_cov_host(ft.points(shape, h, origin=o), family, SIGMA, ell)
    nW = float(scipy.sparse.linalg.svds(W, k=1, return_singular_vectors=False)[0]) if min(W.shape) > 2 else float(np.linalg.norm(W, 2))
    nC = float(scipy.sparse.linalg.eigsh(Cg, k=1, return_eigenvectors=False)[0]) if Cg.shape[0] > 2 else float(np.linalg.norm(Cg, 2))
    return W, Cg, nW, nC


def make(ctx, name, diag_correction=True):
    shape, h, o, pts = _points(name)
    family, ell, nugget = KERNELS[name]
    grid = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, origin=o, ctx=ctx)
    K = hf.InterpolatedKernelCovarianceOperator.on_grid(grid, pts, nugget=nugget, diag_correction=diag_correction)
    return K, grid, K.W, (shape, h, o, pts, family, ell, nugget)


def dev(A, ctx):
    return hf.MultiVector.from_dense(np.asfortranarray(A), ctx=ctx)


def apply(op, X, ctx, accumulate_onto=None):
    Y = hf.MultiVector(op.shape[0], X.shape[1], ctx=ctx) if accumulate_onto is None else dev(accumulate_onto, ctx)
    op.matMvMult(dev(X, ctx), Y, accumulate=accumulate_onto is not None)
    return Y.to_dense()


# ------------------------------------------------------------------------------------------------- 1. gather, spread, adjointness
@pytest.mark.parametrize("name", CASES)
def test_gather_spread_and_adjointness_against_the_twin(ctx, name):
    """|Y - T| <= 2 (4^d + d) eps sum_s |w_s| |G_s| for W;  2 (m_g + d) eps sum |w| |X| over the m_g contributions to a node for W^T (a node
    nobody reaches is +0.0);  <W G, X> = <G, W^T X> per column to 2 (4^d + d) eps sum |w| |G| |X|; 1, 2, 3 and 5 columns, overwriting and
    accumulating (see the module's docstring)."""
    K, grid, W, (shape, h, o, pts, *_rest) = make(ctx, name)
    d, N, Ng = len(shape), pts.shape[0], int(np.prod(shape))
    assert W.shape == (N, Ng) and W.transpose().shape == (Ng, N) and W.transpose().transpose() is W
    base, w = W.weights()
    tb, tww, _ = tw.cell_and_weights(shape, h, o, pts)
    assert np.array_equal(base, tb) and np.max(np.abs(w - tww)) <= 4 * EPS
    assert np.array_equal(W.to_dense(), tw.dense_W(shape, base, w))
    rng = np.random.default_rng(N)
    worst = [0.0, 0.0, 0.0]
    for k in COLUMNS:
        G, X = rng.standard_normal((Ng, k)), rng.standard_normal((N, k))
        T, A = tw.gather(shape, base, w, G)
        Y = apply(W, G, ctx)
        worst[0] = max(worst[0], np.max(np.abs(Y - T) / (2 * (4 ** d + d) * EPS * A)))
        Y0 = rng.standard_normal((N, k))
        assert np.array_equal(apply(W, G, ctx, accumulate_onto=Y0), Y0 + Y)
        Ts, As, m = tw.spread(shape, base, w, X)
        S = apply(W.transpose(), X, ctx)
        assert np.all(S[m == 0] == 0.0) and not np.any(np.signbit(S[m == 0]))
        hit = m > 0
        sb = 2 * (m[hit, None] + d) * EPS * As[hit]      # 0 where every contribution is a zero weight (a point on a node): exact there
        assert np.array_equal((S - Ts)[hit][sb == 0.0], np.zeros(int(np.sum(sb == 0.0))))
        worst[1] = max(worst[1], np.max(np.abs(S - Ts)[hit][sb > 0.0] / sb[sb > 0.0]))
        S0 = rng.standard_normal((Ng, k))
        assert np.array_equal(apply(W.transpose(), X, ctx, accumulate_onto=S0), S0 + S)
        # adjointness, from the device's results; the sums on the host are exact (fsum) up to the rounding of each product
        for j in range(k):
            lhs, rhs = math.fsum(Y[:, j] * X[:, j]), math.fsum(G[:, j] * S[:, j])
            scale = math.fsum(A[:, j] * np.abs(X[:, j]))
            worst[2] = max(worst[2], abs(lhs - rhs) / (2 * (4 ** d + d) * EPS * scale))
    print("interp %s: worst gather %.3g, spread %.3g, adjoint %.3g of the bounds" % (name, *worst))
    assert max(worst) <= 1.0


# ------------------------------------------------------------------------------------------------- 2. the diagonal
@pytest.mark.parametrize("name", CASES)
def test_diagonal_and_delta_against_the_twin(ctx, name):
    """|q_i - twin| <= 2 (16^d + 2 d) eps sum |w_s w_s' c|; delta_i = nugget + max(sigma^2 - q_i, 0) exactly from the device's q; the info
    record agrees with ``.delta``; without the correction delta is the nugget."""
    K, grid, W, (shape, h, o, pts, family, ell, nugget) = make(ctx, name)
    d = len(shape)
    base, w = W.weights()
    q, absq = tw.diagonal(shape, h, family, SIGMA, ell, w)
    worst = np.max(np.abs(K.q - q) / (2 * (16 ** d + 2 * d) * EPS * absq))
    print("interp %s: worst |q - twin| / bound = %.3g; sigma^2 - q in [%.3g, %.3g]" % (name, worst, K.diag_min, K.diag_max))
    assert worst <= 1.0
    defect = SIGMA * SIGMA - K.q
    assert np.array_equal(K.delta, nugget + np.maximum(defect, 0.0))
    assert K.diag_min == defect.min() and K.diag_max == defect.max() and K.n_diag_clipped == int(np.sum(defect < 0.0))
    K0 = make(ctx, name, diag_correction=False)[0]
    assert np.array_equal(K0.q, K.q) and np.all(K0.delta == nugget) and (K0.diag_min, K0.diag_max) == (K.diag_min, K.diag_max)


# ------------------------------------------------------------------------------------------------- 3. K as one operator
@pytest.mark.parametrize("name", CASES)
def test_K_against_its_three_public_steps(ctx, name):
    """W^T, the grid operator and W run separately on the device, delta X added on the host: |diff_ij| <= 2 eps (|(W G)_ij| + |delta_i X_ij|)"""
    K, grid, W, (shape, h, o, pts, *_rest) = make(ctx, name)
    N = pts.shape[0]
    rng = np.random.default_rng(N + 1)
    worst = 0.0
    for k in COLUMNS:
        X = rng.standard_normal((N, k))
        WG = apply(W, apply(grid, apply(W.transpose(), X, ctx), ctx), ctx)
        DX = K.delta[:, None] * X
        Y = apply(K, X, ctx)
        worst = max(worst, np.max(np.abs(Y - (WG + DX)) / (2 * EPS * (np.abs(WG) + np.abs(DX)) + np.finfo(np.float64).tiny)))
        Y0 = rng.standard_normal((N, k))
        assert np.array_equal(apply(K, X, ctx, accumulate_onto=Y0), Y0 + Y)
    print("interp %s: worst |K X - steps| / bound = %.3g" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_K_against_the_dense_twin(ctx, name):
    """Per column, all norms from the dense twins:  ||K X_j - T_j||_2 <= ||W||_2 b_j + 2 (4^d + d) eps ( || |W| |Cg W^T X_j| ||_2 +
    ||W||_2 ||Cg||_2 || |W^T| |X_j| ||_2 ), b_j = fftcov_twin.column_bounds of the twin's spread column.  T = W (Cg (W^T X)) + delta X with
    the dense W and Cg and the operator's delta (held to the twin's in test 2)."""
    K, grid, _, (shape, h, o, pts, family, ell, nugget) = make(ctx, name)
    Wd, Cg, nW, nC = twin_dense(name)
    d, N = len(shape), pts.shape[0]
    rng = np.random.default_rng(N + 2)
    worst = 0.0
    for k in COLUMNS:
        X = rng.standard_normal((N, k))
        Gs = Wd.T @ X
        CG = Cg @ Gs
        T = Wd @ CG + K.delta[:, None] * X
        b = ft.column_bounds(shape, h, family, SIGMA, ell, 0.0, Gs, np.abs(Cg) @ np.abs(Gs))
        bound = nW * b + 2 * (4 ** d + d) * EPS * (np.linalg.norm(np.abs(Wd) @ np.abs(CG), axis=0)
                                                   + nW * nC * np.linalg.norm(np.abs(Wd.T) @ np.abs(X), axis=0))
        worst = max(worst, np.max(np.linalg.norm(apply(K, X, ctx) - T, axis=0) / bound))
    print("interp %s: worst ||K X - twin|| / bound = %.3g" % (name, worst))
    assert worst <= 1.0
    if name == "d2":        # the public dense forms say the same
        assert np.allclose(K.to_dense(), Wd @ Cg @ Wd.T + np.diag(K.delta), rtol=0, atol=64 * EPS * SIGMA ** 2)
        assert np.array_equal(K.exact_dense(), hf.kernel_cov_host(pts, family, SIGMA, ell, nugget))


# ------------------------------------------------------------------------------------------------- 4. repeatability
@pytest.mark.parametrize("name", ["d3", "big"])
def test_repeatability_chunking_and_point_order(ctx, name):
    """Two applies are bit-identical; "fftcov_pairs" = 1, 2 and the default give the same bits of K X and of the draws; the spread of the
    same points given in another order (X permuted with them) is the same G within the spread bound."""
    K, grid, W, (shape, h, o, pts, family, ell, nugget) = make(ctx, name)
    d, N = len(shape), pts.shape[0]
    rng = np.random.default_rng(N + 3)
    X = rng.standard_normal((N, 5))
    ref = apply(K, X, ctx)
    assert np.array_equal(apply(K, X, ctx), ref)
    S = apply(W.transpose(), X, ctx)
    assert np.array_equal(apply(W.transpose(), X, ctx), S)
    s = K.sampler(on_indefinite="clip")
    draws = s.sample(5, 3).to_dense()
    for pairs in (1, 2):
        L.call("hfmi_tuning_set", b"fftcov_pairs", pairs)
        try:
            assert np.array_equal(apply(K, X, ctx), ref) and np.array_equal(s.sample(5, 3).to_dense(), draws)
        finally:
            L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    p = rng.permutation(N)
    Wp = hf.GridInterpolationOperator(shape, h, o, pts[p], ctx=ctx)
    Sp = apply(Wp.transpose(), X[p], ctx)
    base, w = W.weights()
    _, As, m = tw.spread(shape, base, w, X)
    hit = m > 0
    assert np.array_equal(Sp[~hit], S[~hit])
    sb = 2 * (m[hit, None] + d) * EPS * As[hit]
    assert np.all(np.abs(Sp - S)[hit] <= sb)


# ------------------------------------------------------------------------------------------------- 5. block storage contract
@pytest.mark.parametrize("layout", ["wrapped", "parent"])
@pytest.mark.parametrize("name", ["d2", "big"])
def test_block_contract_of_the_three_operators(ctx, name, layout):
    """Y a view inside a wider parent with guard columns, for W (length N), W^T (length prod n) and K: padding rows stay +0.0, nothing
    outside Y's window changes, an overwriting apply equals the apply into a plain block bit for bit and an accumulating one adds it;
    blocks of another length are refused."""
    K, grid, W, (shape, h, o, pts, *_rest) = make(ctx, name)
    N, Ng = W.shape
    k, guard = 3, 2
    rng = np.random.default_rng(N + 4)
    for op, nin, nout in ((W, Ng, N), (W.transpose(), N, Ng), (K, N, N)):
        Xin = dev(rng.standard_normal((nin, k)), ctx)
        plain = hf.MultiVector(nout, k, ctx=ctx)
        op.matMvMult(Xin, plain)
        D = plain.to_dense()
        if layout == "wrapped":
            a = ba.Arena.wrapped(ctx, nout, k + 2 * guard, ld=ba.round_up(nout, 32) + 32)
            y = a.window(guard, k)
        else:
            a = ba.Arena.in_parent(ctx, nout, 2 * k + 2 * guard)
            a.window(guard, k)
            y = a.window(guard + k, k)
        Y0 = rng.standard_normal((nout, k))
        L.call("hfmi_block_upload", y.mv.handle, L.ptr(L.as_f64(Y0)), L.LAYOUT_DENSE)
        for accumulate in (True, False, True):
            a.snapshot()
            before = y.mv.to_dense()
            op.matMvMult(Xin, y.mv, accumulate=accumulate)
            a.check(written=[y], what="hfmi_op_apply of %s accumulate=%d [%s]" % (type(op).__name__, accumulate, layout))
            assert np.array_equal(y.mv.to_dense(), before + D if accumulate else D), accumulate
        for bad_in, bad_out in ((nin + 1, nout), (nin, nout + 1), (nout, nin) if nin != nout else (nin + 2, nout)):
            with pytest.raises(hf.HfmiError):
                op.matMvMult(hf.MultiVector(bad_in, k, ctx=ctx), hf.MultiVector(bad_out, k, ctx=ctx))
    # the draw writes through a const handle: the same contract
    s = K.sampler(on_indefinite="clip")
    D = s.sample(k, 9).to_dense()
    a = ba.Arena.wrapped(ctx, N, k + 2 * guard, ld=ba.round_up(N, 32) + 32) if layout == "wrapped" else ba.Arena.in_parent(ctx, N, k + 2 * guard)
    y = a.window(guard, k)
    L.call("hfmi_block_upload", y.mv.handle, L.ptr(L.as_f64(np.zeros((N, k)))), L.LAYOUT_DENSE)
    for accumulate in (False, True):
        a.snapshot()
        before = y.mv.to_dense()
        s.sample(k, 9, out=y.mv, accumulate=accumulate)
        a.check(written=[y], what="hfmi_interp_sampler_draw accumulate=%d [%s]" % (accumulate, layout))
        assert np.array_equal(y.mv.to_dense(), before + D if accumulate else D)


# ------------------------------------------------------------------------------------------------- 6. the sampler
@pytest.mark.parametrize("name", CASES)
def test_sampler_against_its_definition(ctx, name):
    """sample(n, seed, first) = W z + sqrt(delta) eta within 2 eps (|W z| + |sqrt(delta) eta|) plus the gather bound: z the grid sampler's
    draws first .. first + n - 1 of the same seed, eta the vectors first .. first + n - 1 of hfmi_randn_fill under the key
    seed ^ 0x9E3779B97F4A7C15, stream 0 -- generated on the device by that entry point, and held to the twin's statement of key, stream
    and index (oracle/philox.py through libm) at the 1e-13 of test_gpu_kernels.py.  Chunks reproduce one call; an odd first is refused."""
    K, grid, W, (shape, h, o, pts, *_rest) = make(ctx, name)
    d, N = len(shape), pts.shape[0]
    s = K.sampler(on_indefinite="clip", seed=5)
    assert (s.growth, s.embedding, s.n_clipped, s.cov_error_bound) == (s.grid_sampler.growth, s.grid_sampler.embedding,
                                                                       s.grid_sampler.n_clipped, s.grid_sampler.cov_error_bound)
    base, w = W.weights()
    seed, n = 0x1234567890ABCDEF, 5
    for first in (0, 6):
        Y = s.sample(n, seed, first=first).to_dense()
        Z = s.grid_sampler.sample(n, seed, first=first).to_dense()
        E = hf.MultiVector(N, first + n, ctx=ctx)
        L.call("hfmi_randn_fill", E.handle, C.c_uint64((seed ^ tw.NOISE_KEY_XOR) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(0), 1.0)
        eta = E.to_dense()[:, first:]
        np.testing.assert_allclose(eta, tw.noise(N, n, seed, first), rtol=0, atol=1e-13)
        WZ, A = tw.gather(shape, base, w, Z)
        SE = np.sqrt(K.delta)[:, None] * eta
        bound = 2 * EPS * (np.abs(WZ) + np.abs(SE)) + 2 * (4 ** d + d) * EPS * A
        assert np.max(np.abs(Y - (WZ + SE)) / bound) <= 1.0
    whole = s.sample(12, seed).to_dense()
    parts = np.concatenate([s.sample(4, seed, first=f).to_dense() for f in (0, 4, 8)], axis=1)
    assert np.array_equal(parts, whole)
    with pytest.raises(hf.HfmiError):
        s.sample(2, seed, first=3)
    # sample_block walks the stream of the construction seed, rounding its counter up to even
    blk = np.concatenate([s.sample_block(3), s.sample_block(2)])
    ref = s.sample(6, 5).to_dense().T
    assert np.array_equal(blk, ref[[0, 1, 2, 4, 5]])


# ------------------------------------------------------------------------------------------------- 7. KLE
KLE_ELL = 1.0      # Matern-5/2 with ell = 1, the kernel of the test whose tolerance form this one takes


def test_kle_of_K_against_the_dense_twin(ctx):
    """doublePass on K over the grid and the points of the 70 x 67 case, rank 10, against scipy.linalg.eigh of the twin's dense K (not of
    C), in the tolerance form of test_gpu_grid_kernel_cov.py::test_kle_equivalence_with_the_matrix_free_operator: orthonormality to
    1e-10, eigen-residual 1e-4.  The kernel is that test's (Matern-5/2, ell = 1): the residual measures the randomized method first and
    the operator second, and the method needs a spectrum that has decayed at rank + oversampling.  In exact numpy arithmetic on the
    dense twin (10 + 10 probes, s = 2) the double pass leaves a residual of 8.3e-7 with ell = 1 (lambda_20 / lambda_1 = 3.6e-5) and of
    8.0e-3 with the ell = 0.2 of the other tests here (lambda_20 / lambda_1 = 4.8e-2), whatever applies K."""
    shape, h, o, pts = _points("big")
    grid = hf.GridKernelCovarianceOperator(shape, h, family="matern52", sigma=SIGMA, ell=KLE_ELL, origin=o, ctx=ctx)
    K = hf.InterpolatedKernelCovarianceOperator.on_grid(grid, pts)
    Wd = twin_dense("big")[0]
    Kd = Wd @ hf.kernel_cov_host(ft.points(shape, h, origin=o), "matern52", SIGMA, KLE_ELL) @ Wd.T
    Kd = 0.5 * (Kd + Kd.T) + np.diag(K.delta)
    N, r, p = pts.shape[0], 10, 10
    lam = scipy.linalg.eigh(Kd, eigvals_only=True, subset_by_index=[N - r, N - 1])[::-1]
    Omega = hf.MultiVector(N, r + p, ctx=ctx)
    hf.parRandom.reseed(7)
    hf.parRandom.normal(1.0, Omega)
    dvals, U = hf.doublePass(K, Omega, r, s=2)
    V = U.to_dense()
    assert np.abs(V.T @ V - np.eye(r)).max() < 1e-10
    res = np.linalg.norm(Kd @ V - V * dvals) / np.linalg.norm(Kd @ V)
    print("interp kle: residual %.3g, worst eigenvalue defect %.3g" % (res, np.max(np.abs(dvals - lam) / lam[0])))
    assert res < 1e-4 and np.max(np.abs(dvals - lam) / lam[0]) < 1e-4


# ------------------------------------------------------------------------------------------------- 8. the placed grid, cross, refusals
def test_the_operator_places_its_grid_and_cross_extends(ctx):
    rng = np.random.default_rng(8)
    pts, tg = rng.random((300, 2)) * np.array([1.0, 0.6]), 0.1 + rng.random((70, 2)) * np.array([0.8, 0.4])
    K = hf.InterpolatedKernelCovarianceOperator(pts, "matern52", SIGMA, 0.25, nugget=0.01, cells_per_ell=4, ctx=ctx)
    hgrid = 0.25 / 4
    assert np.allclose(K.spacing, hgrid) and np.all(K.origin <= pts.min(axis=0) - hgrid) and np.allclose(K.origin, pts.min(axis=0) - hgrid)
    assert K.grid_shape == tuple(int(v) for v in np.ceil((pts.max(axis=0) - pts.min(axis=0)) / hgrid).astype(int) + 4)
    assert K.grid.nugget == 0.0 and K.shape == (300, 300) and K.n_diag_clipped == 0 and K.diag_min > 0.0
    Kd = K.to_dense()
    assert np.max(np.abs(np.diag(Kd) - (SIGMA ** 2 + 0.01))) <= 16 ** 2 * EPS * SIGMA ** 2
    X = rng.standard_normal((300, 3))
    Y = apply(K, X, ctx)
    assert np.linalg.norm(Y - Kd @ X) <= 1e-12 * np.linalg.norm(Kd, 2) * np.linalg.norm(X)
    assert np.max(np.abs(Kd - K.exact_dense())) / SIGMA ** 2 < 2 * 4.9e-3          # ell / h = 4, matern52 (the CPU suite holds the table)
    mf = K.matrix_free()
    assert isinstance(mf, hf.KernelCovarianceOperator) and mf.shape == K.shape and mf.nugget == 0.01
    # K(T, S) = W_T Cg W_S^T through the public pieces
    cross = K.cross(tg)
    assert cross.shape == (70, 300)
    WT = hf.GridInterpolationOperator(K.grid_shape, K.spacing, K.origin, tg, ctx=ctx).to_dense()
    ref = WT @ K.grid.to_dense() @ K.W.to_dense().T
    Z = apply(cross, X, ctx)
    assert np.linalg.norm(Z - ref @ X) <= 1e-12 * np.linalg.norm(ref, 2) * np.linalg.norm(X)
    Z0 = rng.standard_normal((70, 3))
    assert np.array_equal(apply(cross, X, ctx, accumulate_onto=Z0), Z0 + Z)


def test_argument_errors(ctx):
    shape, h, o, pts = _points("d2")
    family, ell, nugget = KERNELS["d2"]
    grid = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, origin=o, ctx=ctx)
    subset = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, origin=o, nodes=np.arange(40), ctx=ctx)
    withnug = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, nugget=0.1, origin=o, ctx=ctx)
    on_grid = hf.InterpolatedKernelCovarianceOperator.on_grid
    for bad in (subset, withnug):
        with pytest.raises(hf.HfmiError) as e:
            on_grid(bad, pts)
        assert e.value.code == -1
    outside = pts.copy()
    outside[7, 1] = o[1] + 0.5 * h[1]
    for make_bad in (lambda: on_grid(grid, outside), lambda: hf.GridInterpolationOperator(shape, h, o, outside, ctx=ctx),
                     lambda: on_grid(grid, pts, nugget=-1.0), lambda: hf.GridInterpolationOperator((9, 3), h, o, pts, ctx=ctx)):
        with pytest.raises(hf.HfmiError) as e:
            make_bad()
        assert e.value.code == -1
    with pytest.raises(hf.HfmiError) as e:
        on_grid(grid, outside)
    assert "point 7" in str(e.value) and "axis 1" in str(e.value)
    with pytest.raises(ValueError):
        on_grid(hf.KernelCovarianceOperator(pts, ctx=ctx), pts)
    K = on_grid(grid, pts, nugget=nugget)
    N = pts.shape[0]
    for bad_in, bad_out in ((N + 1, N), (N, N + 1), (int(np.prod(shape)), N)):
        with pytest.raises(hf.HfmiError):
            K.matMvMult(hf.MultiVector(bad_in, 2, ctx=ctx), hf.MultiVector(bad_out, 2, ctx=ctx))
    # a sampler of another covariance is refused by the draw
    other = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=2 * ell, origin=o, ctx=ctx)
    s = K.sampler(on_indefinite="clip")
    s.grid_sampler = other.sampler(on_indefinite="clip")
    with pytest.raises(hf.HfmiError):
        s.sample(2, 1)
