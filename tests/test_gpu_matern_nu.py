"""GPU suite of the Matern family of any smoothness (family "matern" with nu; the hfmi_op_kernel_*_spec2 creators, hfmi_kcov_nu.h):
single entries against the numpy twin run with the library's tables, applies against the dense matrix of the TWIN, the rectangular and
row-slab forms, a rotated metric, grids (with the long route and the sampler's factor), the pivoted Cholesky factor, the KLE of a
Whittle-Matern kernel end to end, and the argument checks.  The shapes are those of tests/test_gpu_kernel_spec.py."""
import contextlib
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_factor_twin as gf                     # noqa: E402
import grid_metric_twin as gt                     # noqa: E402
import matern_nu_twin as tw                       # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
HFMI_ERR_INVALID = -1
E_ASSERT = 64.0                      # eps: the twin against 40 digits (tests/test_matern_nu_cpu.py; measured 23.75)
ENTRY = 2.0 * (E_ASSERT + 16.0)      # eps: device against twin -- the structure of the Matern-1 suite's 64 with E_ASSERT in place of its 16


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def tables(nu):
    T = np.empty(tw.WORDS)
    assert L.load().hfmi_kernel_matern_tables(float(nu), L.ptr(T)) == 0
    return T


def scattered(N, d, seed):
    """seeded points in the unit cube, two of them coincident"""
    pts = np.random.default_rng(seed).random((N, d))
    if N > 3:
        pts[N - 1] = pts[1]
    return pts


def twin_matrix(targets, sources, nu, sigma, ell, nugget=0.0, diag_offset=None, G=None):
    """the dense matrix with the TWIN's phi at the device's own a = ca * sqrt(r2) * (1 / ell), r2 summed coordinate by coordinate on the
    points the library is handed (points @ L with a metric)"""
    T = tables(nu)
    if G is not None:
        Lf = np.linalg.cholesky(G)
        targets, sources = targets @ Lf, sources @ Lf
    r2 = np.zeros((targets.shape[0], sources.shape[0]))
    for c in range(sources.shape[1]):
        dx = targets[:, c][:, None] - sources[None, :, c]
        r2 = r2 + dx * dx
    K = sigma ** 2 * tw.phi(T, T[tw.W_CA] * np.sqrt(r2) * (1.0 / ell))
    if nugget and diag_offset is not None:
        i = np.arange(targets.shape[0])
        K[i, i + diag_offset] += nugget
    return K


@contextlib.contextmanager
def grid_twin_family(nu):
    """tests/helpers/grid_metric_twin.py with phi of family "matern" = the twin's phi_nu (the helper's other families untouched)"""
    T, old = tables(nu), gt.phi
    gt.phi = lambda family, r: tw.phi(T, T[tw.W_CA] * r) if family == "matern" else old(family, r)
    try:
        yield
    finally:
        gt.phi = old


def within_bound(what, Y, Y_ref, N, absCW):
    """entrywise |Y - Y_ref| <= (8 N + 2 (E_ASSERT + 16)) eps (|C| |W|): the worst case of a length-N fp64 sum in any order with the 8 of
    tests/test_gpu_kernel_cov.py, and the entries' own bound (test_entries)"""
    err, bound = np.abs(Y - Y_ref), (8 * N + ENTRY) * EPS * absCW
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("matern nu %s: N=%d k=%d max err/bound = %.3g" % (what, N, Y.shape[1], worst))
    assert np.all(np.isfinite(Y)) and np.all(err <= bound), worst


def apply(op, W, ctx, into=None, accumulate=False):
    Yd = hf.MultiVector(op.shape[0], W.shape[1], ctx=ctx) if into is None else into
    op.matMvMult(hf.MultiVector.from_dense(W, ctx=ctx), Yd, accumulate=accumulate)
    return Yd


# ---------------------------------------------------------------------------------------------------------------- 1. entries
@pytest.fixture(scope="module")
def abscissae():
    """95 abscissae of the fixture, picked as tests/test_gpu_kernel_spec.py::test_entries picks them: 2, its three fp64 neighbours on
    either side and 88 others between 1e-9 and 600"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "matern_nu_phi.npz"))
    a_all = np.unique(z["a"][(z["a"] >= 1e-9) & (z["a"] <= 600.0)])
    near = a_all[np.argsort(np.abs(a_all - 2.0))[:7]]
    assert near.min() < 2.0 < near.max() and 2.0 in near
    rest = np.setdiff1d(a_all, near)
    pick = np.concatenate([near, rest[np.linspace(0, rest.size - 1, 95 - near.size).astype(int)]])
    assert pick.size == 95 and np.unique(pick).size == 95
    return pick


@pytest.mark.parametrize("nu", [0.3, 0.5, 1.0, 1.0 + 2.0 ** -30, 2.5, 3.2, 8.0])
def test_entries(ctx, abscissae, nu):
    """Row 0 of the operator applied to the identity is sigma^2 phi_nu(a_j), one term per sum: within 2 (E_ASSERT + 16) = 160 eps relative
    of the twin at the device's own a -- E_ASSERT for the twin's own error, 16 for fma contraction and the device's log / exp / sqrt,
    and a factor 2 over their sum."""
    T = tables(nu)
    ca = T[tw.W_CA]
    x = np.concatenate([[0.0], abscissae / ca])
    N = x.size
    assert N == 96
    op = hf.KernelCovarianceOperator(x, family="matern", sigma=1.0, ell=1.0, nu=nu, ctx=ctx)
    assert op.nu == nu and op.family == "matern"
    Y = apply(op, np.eye(N), ctx).to_dense()
    dx = x[0] - x[1:]
    a = ca * np.sqrt(dx * dx) * (1.0 / 1.0)                                  # the device's a: ca * sqrt(r2) * inv_ell
    ref = tw.phi(T, a)
    rel = np.abs(Y[0, 1:] - ref) / ref
    j = int(np.argmax(rel))
    print("matern nu = %.10g entries: worst |device - twin| / twin = %.3f eps at a = %.6g (%g allowed); near 2: %.3f eps"
          % (nu, rel.max() / EPS, a[j], ENTRY, rel[np.abs(a - 2.0) < 0.01].max() / EPS))
    assert np.all(np.isfinite(Y)) and Y[0, 0] == 1.0 and np.all(np.diag(Y) == 1.0)
    assert rel.max() <= ENTRY * EPS
    assert np.array_equal(Y, Y.T)
    # coincident points with different indices: phi(0) = 1 exactly, no nugget there, the nugget on the index
    sigma = 1.3
    pts = np.array([0.25, 0.25, 0.7, 0.25])
    op = hf.KernelCovarianceOperator(pts, family="matern", sigma=sigma, ell=0.4, nugget=0.5, nu=nu, ctx=ctx)
    Y = apply(op, np.eye(4), ctx).to_dense()
    assert np.all(np.isfinite(Y))
    assert Y[0, 1] == Y[1, 0] == Y[0, 3] == sigma * sigma and np.all(np.diag(Y) == sigma * sigma + 0.5)


# ---------------------------------------------------------------------------------------------------------------- 2. applies against the twin
@pytest.mark.parametrize("N,nvec,d", [(65, 1, 1), (95, 17, 2), (200, 150, 3)])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nu", [0.75, 3.2])
def test_apply_against_the_twin(ctx, N, nvec, d, accumulate, nu):
    sigma, ell, nugget = 1.3, 0.3, 0.2
    rng = np.random.default_rng(1000 * N + nvec)
    pts = scattered(N, d, seed=N + d)
    Cm = twin_matrix(pts, pts, nu, sigma, ell, nugget, diag_offset=0)
    op = hf.KernelCovarianceOperator(pts, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, ctx=ctx)
    W = rng.standard_normal((N, nvec))
    Yd = apply(op, W, ctx)
    ref, absCW = Cm @ W, np.abs(Cm) @ np.abs(W)
    if accumulate:
        W2 = rng.standard_normal((N, nvec))
        apply(op, W2, ctx, into=Yd, accumulate=True)
        ref, absCW = ref + Cm @ W2, absCW + np.abs(Cm) @ np.abs(W2)
    within_bound("nu=%g acc=%d" % (nu, accumulate), Yd.to_dense(), ref, N, absCW)
    # the host's matrix (scipy) is an independent statement of the same one: 1024 eps and the abscissa's 2 a eps (test_matern_nu_cpu.py)
    host = op.to_dense()
    assert np.array_equal(host, hf.kernel_cov_host(pts, "matern", sigma, ell, nugget, nu=nu))
    a_max = np.sqrt(2.0 * nu * d) / ell
    assert np.all(np.abs(host - Cm) <= (1024.0 + E_ASSERT + 2.0 * a_max) * EPS * np.abs(Cm))


@pytest.mark.parametrize("nu", [0.75, 3.2])
def test_cross_rows_and_determinism(ctx, nu):
    sigma, ell, nugget, N, M, r0, k = 1.1, 0.25, 0.3, 95, 37, 20, 17
    pts = scattered(N, 2, seed=4)
    W = np.random.default_rng(5).standard_normal((N, k))
    cross = hf.KernelCrossCovarianceOperator(pts[r0:r0 + M], pts, family="matern", sigma=sigma, ell=ell, nugget=nugget, diag_offset=r0,
                                             nu=nu, ctx=ctx)
    K = twin_matrix(pts[r0:r0 + M], pts, nu, sigma, ell, nugget, diag_offset=r0)
    assert cross.shape == (M, N) and cross.nu == nu and cross.to_dense().shape == (M, N)
    Yc = apply(cross, W, ctx).to_dense()
    within_bound("nu=%g cross" % nu, Yc, K @ W, N, np.abs(K) @ np.abs(W))
    op = hf.KernelCovarianceOperator(pts, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, ctx=ctx)
    Y1, Y2 = apply(op, W, ctx).to_dense(), apply(op, W, ctx).to_dense()
    assert np.array_equal(Y1, Y2)                                           # two applies are bit-identical
    assert np.array_equal(Yc, Y1[r0:r0 + M])                                # the cross form with a diagonal IS those rows
    slab = op.rows(r0, r0 + M)
    assert slab.family == "matern" and slab.nu == nu
    Ys = apply(slab, W, ctx).to_dense()
    assert np.array_equal(Ys[r0:r0 + M], Y1[r0:r0 + M]) and not Ys[:r0].any() and not Ys[r0 + M:].any()
    # no target is a source: the transposed operator carries nu
    Tg = scattered(11, 2, seed=77)
    free = hf.KernelCrossCovarianceOperator(Tg, pts, family="matern", sigma=sigma, ell=ell, nu=nu, ctx=ctx)
    Kf = twin_matrix(Tg, pts, nu, sigma, ell)
    within_bound("nu=%g cross, no diagonal" % nu, apply(free, W, ctx).to_dense(), Kf @ W, N, np.abs(Kf) @ np.abs(W))
    assert free.transpose().nu == nu and free.transpose().shape == (N, 11)


@pytest.mark.parametrize("nu", [0.75, 3.2])
def test_rotated_metric(ctx, nu):
    sigma, ell, nugget, N, k = 0.9, 0.5, 0.15, 150, 20
    G = gt.rotated_metric()
    pts = scattered(N, 2, seed=32)
    W = np.random.default_rng(31).standard_normal((N, k))
    op = hf.KernelCovarianceOperator(pts, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, metric=G, ctx=ctx)
    Cm = twin_matrix(pts, pts, nu, sigma, ell, nugget, diag_offset=0, G=G)
    Y = apply(op, W, ctx).to_dense()
    within_bound("nu=%g rotated" % nu, Y, Cm @ W, N, np.abs(Cm) @ np.abs(W))
    assert np.abs(Cm - twin_matrix(pts, pts, nu, sigma, ell, nugget, diag_offset=0)).max() > 1e-3      # the metric is not a no-op here
    slab = op.rows(40, 90)
    assert np.array_equal(slab.metric, G) and slab.nu == nu and np.array_equal(apply(slab, W, ctx).to_dense()[40:90], Y[40:90])


def test_nu_three_halves_is_matern32_to_rounding(ctx):
    """no dispatch: the general evaluation at nu = 1.5 and the named family differ by rounding, not by nothing"""
    N, k, sigma, ell = 130, 9, 1.2, 0.4
    pts = scattered(N, 2, seed=8)
    W = np.random.default_rng(9).standard_normal((N, k))
    a = apply(hf.KernelCovarianceOperator(pts, family="matern", sigma=sigma, ell=ell, nu=1.5, ctx=ctx), W, ctx).to_dense()
    b_op = hf.KernelCovarianceOperator(pts, family="matern32", sigma=sigma, ell=ell, ctx=ctx)
    Cm = b_op.to_dense()
    within_bound("nu=1.5 against matern32", a, apply(b_op, W, ctx).to_dense(), N, 2.0 * np.abs(Cm) @ np.abs(W))


# ---------------------------------------------------------------------------------------------------------------- 3. grids
GRID_SHAPES = [("9", (9,), (0.3,), np.array([[2.5]])), ("6x5", (6, 5), (0.2, 0.25), gt.rotated_metric()),
               ("4x3x3", (4, 3, 3), (0.2, 0.25, 0.3), gt.FULL_3D)]


@pytest.mark.parametrize("cid,shape,spacing,G", GRID_SHAPES, ids=[c[0] for c in GRID_SHAPES])
@pytest.mark.parametrize("metric", [False, True])
@pytest.mark.parametrize("subset", [False, True])
def test_grid_apply_against_the_twin(ctx, cid, shape, spacing, G, metric, subset):
    """per column ||Y_j - Yref_j||_2 <= 32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W_j||_2 + 8 N eps || |C| |W_j| ||_2, the grid suite's
    column bound with the twin's signed column c; Yref is the twin's dense matrix times W"""
    sigma, ell, nugget, k, nu = 1.3, 0.45, 0.2, 5, 0.75
    G = G if metric else None
    nodes = gt.case_nodes(shape, subset)
    if nodes is not None:
        nodes = np.random.default_rng(len(shape)).permutation(nodes)                  # a shuffled subset
    op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern", sigma=sigma, ell=ell, nugget=nugget, nodes=nodes, nu=nu,
                                         metric=G, ctx=ctx)
    pts = gt.points(shape, spacing, nodes)
    N = pts.shape[0]
    assert op.shape == (N, N) and np.array_equal(op.points, pts) and op.nu == nu
    W = np.random.default_rng(N).standard_normal((N, k))
    Cm = twin_matrix(pts, pts, nu, sigma, ell, nugget, diag_offset=0, G=G)
    with grid_twin_family(nu):
        bound = gt.column_bounds(shape, spacing, "matern", sigma, ell, nugget, W, np.abs(Cm) @ np.abs(W), G)
    Y = apply(op, W, ctx).to_dense()
    ratio = np.linalg.norm(Y - Cm @ W, axis=0) / bound
    print("grid matern nu %s metric=%s subset=%s: worst err/bound = %.3g" % (cid, metric, subset, ratio.max()))
    assert np.all(np.isfinite(Y)) and ratio.max() <= 1.0
    mf = op.matrix_free()
    assert mf.family == "matern" and mf.nu == nu and (mf.metric is None) == (G is None)
    within_bound("grid matrix_free %s" % cid, apply(mf, W, ctx).to_dense(), Cm @ W, N, np.abs(Cm) @ np.abs(W))


def test_grid_long_route_with_a_split_axis(ctx):
    """(5, 3, 6) at fftcov_max_line = 4, the smallest line of tests/test_gpu_grid_long.py: the embedding axes 8, 4 and 16 are split"""
    shape, spacing, sigma, ell, nugget, k, nu = (5, 3, 6), (0.2, 0.25, 0.3), 1.3, 0.45, 0.2, 3, 0.75
    L.call("hfmi_tuning_set", b"fftcov_max_line", 4)
    try:
        op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, ctx=ctx, long_axes=True)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_max_line", 4096)
    assert op.long_axes and op.nu == nu
    pts = gt.points(shape, spacing, None)
    N = pts.shape[0]
    W = np.random.default_rng(N).standard_normal((N, k))
    Cm = twin_matrix(pts, pts, nu, sigma, ell, nugget, diag_offset=0)
    with grid_twin_family(nu):
        bound = gt.column_bounds(shape, spacing, "matern", sigma, ell, nugget, W, np.abs(Cm) @ np.abs(W), None)
    Y = apply(op, W, ctx).to_dense()
    ratio = np.linalg.norm(Y - Cm @ W, axis=0) / bound
    print("grid matern nu long route (5, 3, 6) max_line 4: worst err/bound = %.3g" % ratio.max())
    assert np.all(np.isfinite(Y)) and ratio.max() <= 1.0
    short = hf.GridKernelCovarianceOperator(shape, spacing, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, ctx=ctx)
    assert (np.linalg.norm(apply(short, W, ctx).to_dense() - Y, axis=0) <= 2.0 * bound).all()


def test_grid_sampler_and_factor(ctx):
    """(6, 5), nu = 0.75, rotated metric: S S^T = C within cov_error_bound plus the rounding of tests/test_gpu_grid_factor.py (the
    composition's bound_S(S^T X) + ||S||_2 bound_St(X) for X = I and the fp64 twin's own 64 eps log2(P) (sigma^2 + nugget)); the sampler
    keeps copies of nu and the tables, so it draws after the operator is gone"""
    shape, spacing, G = (6, 5), (0.2, 0.25), gt.rotated_metric()
    sigma, ell, nugget, nu = 1.3, 0.45, 0.0, 0.75
    op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, metric=G, ctx=ctx)
    s = op.sampler(max_growth=3, on_indefinite="clip")
    S = s.factor()
    N, Ptot = S.shape
    assert Ptot == int(np.prod(s.embedding))
    with grid_twin_family(nu):
        lam = gt.spectrum(shape, spacing, "matern", sigma, ell, nugget, G, growth=s.growth).real
    print("grid matern nu sampler: growth %d, embedding %r, lambda in [%.3g, %.3g] (twin [%.3g, %.3g]), clipped %d, cov_error_bound %.3g"
          % (s.growth, tuple(s.embedding), s.lambda_min, s.lambda_max, lam.min(), lam.max(), s.n_clipped, s.cov_error_bound))
    assert abs(s.lambda_max - lam.max()) <= 1e-10 * lam.max() and abs(s.lambda_min - lam.min()) <= 1e-10 * lam.max()
    X = np.eye(N)
    V, Y = hf.MultiVector(Ptot, N, ctx=ctx), hf.MultiVector(N, N, ctx=ctx)
    S.transpose().matMvMult(hf.MultiVector.from_dense(X, ctx=ctx), V)
    S.matMvMult(V, Y)
    root = np.sqrt(np.maximum(lam, 0.0))
    rounding = gf.column_bounds(root, V.to_dense()) + root.max() * gf.column_bounds(root, X) + gf.twin_tolerance(Ptot, sigma, nugget)
    Cm = twin_matrix(op.points, op.points, nu, sigma, ell, G=G)
    diff = np.abs(Y.to_dense() - Cm).max(axis=0)
    print("grid matern nu factor: max |S S^T - C| %.3g, allowed %.3g" % (diff.max(), (s.cov_error_bound + rounding).min()))
    assert np.all(diff <= s.cov_error_bound + rounding)
    first = s.sample(4, seed=3).to_dense()
    del S, op
    gc.collect()
    again = s.sample(4, seed=3).to_dense()
    assert first.shape == (N, 4) and np.all(np.isfinite(first)) and np.abs(first).max() > 0.0
    assert np.array_equal(first, again)                                      # the same seed, the same draws, without the operator


# ---------------------------------------------------------------------------------------------------------------- 4. pivoted Cholesky
def test_pivoted_cholesky_with_a_rotated_metric(ctx):
    """Scattered N = 150, d = 2, nu = 2.5 THROUGH THE GENERAL FAMILY, rank 30: the order-free properties of tests/helpers/pchol_checks.py
    with its tolerances -- L L^T reproduces C (the twin's matrix) on the pivot columns within 8 (rank + 2) eps (|L| |L_P|^T + |C_P|); the
    reported trace is N d0 - ||L[:, :j]||_F^2 within 8 (j + 2) N eps d0 and decreases."""
    N, rank, sigma, ell, nugget, nu = 150, 30, 1.3, 0.4, 0.0, 2.5
    G = gt.rotated_metric()
    pts = scattered(N, 2, seed=N + 2)
    op = hf.KernelCovarianceOperator(pts, family="matern", sigma=sigma, ell=ell, nugget=nugget, nu=nu, metric=G, ctx=ctx)
    f = hf.pivoted_cholesky(op, rank)
    Lh, piv, trace = f.L.to_dense(), f.pivots, f.trace
    d0 = sigma * sigma + nugget
    assert f.rank == rank and Lh.shape == (N, rank) and piv[0] == 0
    assert len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < N
    assert not ({1, N - 1} <= set(piv.tolist())), "both points of the coincident pair were chosen"
    assert np.all(np.isfinite(Lh)) and np.all(np.diff(trace) <= 0.0)
    Cp = twin_matrix(pts[piv], pts, nu, sigma, ell, G=G).T
    Lp = Lh[piv, :]
    err = np.abs(Cp - Lh @ Lp.T)
    bound = 8 * (rank + 2) * EPS * (np.abs(Lh) @ np.abs(Lp).T + np.abs(Cp))
    print("pchol matern nu + metric: pivot columns max err/bound = %.3g" % float(np.max(err / bound)))
    assert np.all(err <= bound)
    sq = np.concatenate([[0.0], np.cumsum(np.sum(np.ascontiguousarray(Lh.T) ** 2, axis=1))])
    terr, tbound = np.abs(trace - (N * d0 - sq)), 8 * (np.arange(rank + 1) + 2) * N * EPS * d0
    print("pchol matern nu + metric: trace identity max err/bound = %.3g, residual trace %.3g" % (float(np.max(terr / tbound)), trace[-1]))
    assert np.all(terr <= tbound)
    # the factor at other points goes through the cross-covariance with the same nu and metric: at the operator's own points it is L
    back = f.extend(pts[:50]).to_dense()
    assert np.abs(back - Lh[:50]).max() <= 1e-9 * np.abs(Lh).max()


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
class _MassOnly:
    pass


def test_whittle_matern_kle_end_to_end(ctx):
    """The KLE of whittle_matern_kernel(gamma, delta, alpha = 3, d = 2), nu = 2, on a 17 x 17 grid by doublePass through the grid operator
    and through the explicit matrix: the eigenvalues agree to 1e-10 d_0 (what the BiLaplacian test asks), V^T M V = I and E = M V to 1e-10."""
    shape, spacing = (17, 17), (1.0 / 16.0, 1.0 / 16.0)
    kw = hf.whittle_matern_kernel(0.1, 1.0, 3, 2)
    assert kw["nu"] == 2.0
    op = hf.GridKernelCovarianceOperator(shape, spacing, ctx=ctx, **kw)
    N, r, p = op.shape[0], 12, 20
    mdiag = (0.5 + np.random.default_rng(2).random(N)) / N
    M = sp.diags(mdiag).tocsr()
    Cm = hf.kernel_cov_host(op.points, **kw)
    assert np.array_equal(op.to_dense(), Cm)
    prior = hf.GridKernelPrior(op, M=M, on_indefinite="clip")
    draws = prior.sample_block(4)
    assert draws.shape == (4, N) and np.all(np.isfinite(draws)) and np.abs(draws).max() > 0.0
    results = {}
    for name, Cop in (("grid", op), ("explicit", hf.npToDeviceOperator(Cm, ctx=ctx))):
        holder = _MassOnly()
        holder.M, holder.C = M, Cop
        params = hf.KLEParameterList()
        params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = r, p, False, False
        hf.parRandom.reseed(7)
        kle = hf.KLEProjector(holder, parameters=params, ctx=ctx)
        d, dec, enc = kle.construct_input_subspace("mass")
        d, V, E = np.asarray(d), dec.to_dense(), enc.to_dense()
        assert np.abs(V.T @ (M @ V) - np.eye(r)).max() < 1e-10
        assert np.linalg.norm(E - M @ V) / np.linalg.norm(M @ V) < 1e-10
        results[name] = d
    gap = np.abs(results["grid"] - results["explicit"]).max() / results["explicit"][0]
    print("whittle-matern KLE (nu = 2, 17 x 17): max |delta d| / d_0 between the grid operator and the explicit matrix = %.3g" % gap)
    assert gap <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- 6. arguments
def test_invalid_arguments(ctx):
    pts = L.as_f64(scattered(9, 2, seed=1))
    out = C.c_void_p()
    lib = L.load()
    n, h = np.array([3, 3], dtype=np.int64), np.array([0.1, 0.1])

    def spec(family=5, d=2, sigma=1.0, ell=0.2, nugget=0.0, metric=None, nu=1.25):
        s = L.KernelSpec2(family, d, sigma, ell, nugget)
        for i, v in enumerate(np.zeros(9) if metric is None else np.asarray(metric, dtype=np.float64).ravel()):
            s.metric[i] = v
        s.nu = nu
        return s

    creators = {
        "cov": lambda s: lib.hfmi_op_kernel_cov_spec2(ctx.handle, L.ptr(pts), 9, 2, C.byref(s), C.byref(out)),
        "cross": lambda s: lib.hfmi_op_kernel_cross_cov_spec2(ctx.handle, L.ptr(pts[:3]), 3, L.ptr(pts), 9, 2, C.byref(s), 0, C.byref(out)),
        "rows": lambda s: lib.hfmi_op_kernel_cov_rows_spec2(ctx.handle, L.ptr(pts), 9, 2, C.byref(s), 0, 3, C.byref(out)),
        "grid": lambda s: lib.hfmi_op_kernel_cov_grid_spec2(ctx.handle, 2, L.ptr(n), L.ptr(h), None, 9, C.byref(s), C.byref(out)),
        "grid_long": lambda s: lib.hfmi_op_kernel_cov_grid_long_spec2(ctx.handle, 2, L.ptr(n), L.ptr(h), None, 9, C.byref(s), C.byref(out)),
    }
    bad = [spec(nu=0.0), spec(nu=0.1), spec(nu=8.5), spec(nu=-1.0), spec(nu=np.nan), spec(nu=np.inf),      # the smoothness
           spec(family=1, nu=1.5), spec(family=4, nu=1.0), spec(family=0, nu=np.nan),                       # nu with another family
           spec(family=6), spec(family=-1), spec(ell=0.0), spec(nugget=-1.0), spec(d=3),
           spec(metric=[[2.0, 0.5], [0.6, 1.0]]), spec(metric=[[1.0, 2.0], [2.0, 1.0]]), spec(metric=[[1.0, 0.0], [0.0, np.nan]])]
    for name, create in creators.items():
        for i, s in enumerate(bad):
            assert create(s) == HFMI_ERR_INVALID, (name, i)
        assert create(spec()) == 0, name
        lib.hfmi_op_destroy(out)
        assert create(spec(nu=0.125, metric=[[2.0, 0.5], [0.5, 1.0]])) == 0 and lib.hfmi_op_destroy(out) == 0, name
        assert create(spec(family=4, nu=0.0)) == 0 and lib.hfmi_op_destroy(out) == 0, name
    assert lib.hfmi_op_kernel_cov_spec2(ctx.handle, L.ptr(pts), 9, 2, None, C.byref(out)) == HFMI_ERR_INVALID
    # the old descriptor and the bare family still refuse family 5
    old = L.KernelSpec(5, 2, 1.0, 0.2, 0.0)
    assert lib.hfmi_op_kernel_cov_spec(ctx.handle, L.ptr(pts), 9, 2, C.byref(old), C.byref(out)) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cov_grid_long(ctx.handle, 2, L.ptr(n), L.ptr(h), None, 9, C.byref(old), C.byref(out)) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cov(ctx.handle, L.ptr(pts), 9, 2, 5, 1.0, 0.2, 0.0, C.byref(out)) == HFMI_ERR_INVALID
    # Python: ValueError before the library is asked
    makers = [lambda **kw: hf.KernelCovarianceOperator(pts, ctx=ctx, **kw),
              lambda **kw: hf.KernelCrossCovarianceOperator(pts[:3], pts, ctx=ctx, **kw),
              lambda **kw: hf.KernelCovarianceRowsOperator(pts, kw.pop("family"), 1.0, 0.2, 0.0, 0, 3, ctx=ctx, **kw),
              lambda **kw: hf.GridKernelCovarianceOperator((3, 3), 0.1, ctx=ctx, **kw)]
    for make in makers:
        with pytest.raises(ValueError):
            make(family="matern")
        with pytest.raises(ValueError):
            make(family="matern32", nu=1.5)
        with pytest.raises(ValueError):
            make(family="matern1", nu=1.0)
        for nu in (0.0, 0.1, 8.5, np.nan):
            with pytest.raises(ValueError):
                make(family="matern", nu=nu)
        with pytest.raises(ValueError):
            make(family="matern72")
        assert make(family="matern", nu=1.25).nu == 1.25


def test_spec2_with_a_named_family_gives_the_old_creators_bits(ctx):
    """a valid hfmi_kernel_spec2 with family 1 and nu = 0: the operator of hfmi_op_kernel_cov on the same input, bit for bit"""
    N, k = 200, 20
    pts = L.as_f64(scattered(N, 3, seed=12))
    W = np.random.default_rng(13).standard_normal((N, k))
    lib = L.load()
    ref = apply(hf.KernelCovarianceOperator(pts, family="matern32", sigma=1.2, ell=0.4, nugget=0.1, ctx=ctx), W, ctx).to_dense()
    op = hf.KernelCovarianceOperator.__new__(hf.KernelCovarianceOperator)
    hf.DeviceOperator.__init__(op, ctx, N)
    s = L.KernelSpec2(1, 3, 1.2, 0.4, 0.1)
    assert lib.hfmi_op_kernel_cov_spec2(ctx.handle, L.ptr(pts), N, 3, C.byref(s), C.byref(op._op)) == 0
    assert np.array_equal(apply(op, W, ctx).to_dense(), ref)
