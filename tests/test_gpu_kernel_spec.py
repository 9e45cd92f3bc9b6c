"""GPU suite of the Matern-1 family and of the metric of the kernel covariances (the hfmi_op_kernel_*_spec creators, hfmi_kcov_k1.h,
k_fftcov_column_signed): single entries against the numpy twin of a K_1(a), applies against the dense host matrix, the rectangular and
row-slab forms, the metric on scattered points and on grids, the pivoted Cholesky factor, the sampler's factor, the BiLaplacian's kernel
end to end, and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_factor_twin as gf                     # noqa: E402
import grid_metric_twin as gt                     # noqa: E402
import matern1_twin as m1                         # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
HFMI_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def scattered(N, d, seed):
    """seeded points in the unit cube, two of them coincident"""
    pts = np.random.default_rng(seed).random((N, d))
    if N > 3:
        pts[N - 1] = pts[1]
    return pts


def within_bound(what, Y, Y_ref, N, absCW):
    """entrywise |Y - Y_ref| <= (8 N + 64) eps (|C| |W|): the worst case of a length-N fp64 sum in any order with the 8 of
    tests/test_gpu_kernel_cov.py, and 64 eps for the entries themselves (test_entries)"""
    err, bound = np.abs(Y - Y_ref), (8 * N + 64) * EPS * absCW
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("kernel_spec %s: N=%d k=%d max err/bound = %.3g" % (what, N, Y.shape[1], worst))
    assert np.all(np.isfinite(Y)) and np.all(err <= bound), worst


def apply(op, W, ctx, into=None, accumulate=False):
    Yd = hf.MultiVector(op.shape[0], W.shape[1], ctx=ctx) if into is None else into
    op.matMvMult(hf.MultiVector.from_dense(W, ctx=ctx), Yd, accumulate=accumulate)
    return Yd


# ---------------------------------------------------------------------------------------------------------------- 1. entries
def test_entries(ctx):
    """Row 0 of the operator applied to the identity is sigma^2 phi(a_j), one term per sum: within 64 eps relative of the twin at the same
    a -- 16 for the twin's own error E_phi, 16 for fma contraction and the device's log / exp / sqrt through the series' cancellation
    near a = 2 (the result is 0.28 of its leading term there), and a factor 2 over their sum."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "matern1_phi.npz"))
    a_all = np.unique(z["a"][(z["a"] >= 1e-9) & (z["a"] <= 600.0)])
    near = a_all[np.argsort(np.abs(a_all - 2.0))[:7]]                       # 2 itself and its three neighbours on either side
    assert near.min() < 2.0 < near.max() and 2.0 in near
    rest = np.setdiff1d(a_all, near)
    pick = np.concatenate([near, rest[np.linspace(0, rest.size - 1, 95 - near.size).astype(int)]])
    assert pick.size == 95 and np.unique(pick).size == 95
    x = np.concatenate([[0.0], pick / np.sqrt(2.0)])
    N = x.size
    assert N == 96
    op = hf.KernelCovarianceOperator(x, family="matern1", sigma=1.0, ell=1.0, ctx=ctx)
    Y = apply(op, np.eye(N), ctx).to_dense()
    dx = x[0] - x[1:]
    a = 1.4142135623730951 * np.sqrt(dx * dx) * (1.0 / 1.0)                 # the device's a: ca * sqrt(r2) * inv_ell
    ref = m1.phi(a)
    rel = np.abs(Y[0, 1:] - ref) / ref
    j = int(np.argmax(rel))
    print("matern1 entries: worst |device - twin| / twin = %.3f eps at a = %.6g (64 allowed); near 2: %.3f eps"
          % (rel.max() / EPS, a[j], rel[np.abs(a - 2.0) < 0.01].max() / EPS))
    assert np.all(np.isfinite(Y)) and Y[0, 0] == 1.0 and np.all(np.diag(Y) == 1.0)
    assert rel.max() <= 64 * EPS
    assert np.array_equal(Y, Y.T)
    # coincident points with different indices: phi(0) = 1 exactly, no nugget, nothing undefined
    sigma = 1.3
    pts = np.array([0.25, 0.25, 0.7, 0.25])
    op = hf.KernelCovarianceOperator(pts, family="matern1", sigma=sigma, ell=0.4, nugget=0.5, ctx=ctx)
    Y = apply(op, np.eye(4), ctx).to_dense()
    assert np.all(np.isfinite(Y))
    assert Y[0, 1] == Y[1, 0] == Y[0, 3] == sigma * sigma and Y[0, 0] == sigma * sigma + 0.5


# ---------------------------------------------------------------------------------------------------------------- 2. applies against the host
@pytest.mark.parametrize("N,nvec,d", [(65, 1, 1), (95, 17, 2), (200, 150, 3)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_apply_against_host(ctx, N, nvec, d, accumulate):
    sigma, ell, nugget = 1.3, 0.3, 0.2
    rng = np.random.default_rng(1000 * N + nvec)
    pts = scattered(N, d, seed=N + d)
    Cm = hf.kernel_cov_host(pts, "matern1", sigma, ell, nugget)
    op = hf.KernelCovarianceOperator(pts, family="matern1", sigma=sigma, ell=ell, nugget=nugget, ctx=ctx)
    W = rng.standard_normal((N, nvec))
    Yd = apply(op, W, ctx)
    ref, absCW = Cm @ W, np.abs(Cm) @ np.abs(W)
    if accumulate:
        W2 = rng.standard_normal((N, nvec))
        apply(op, W2, ctx, into=Yd, accumulate=True)
        ref, absCW = ref + Cm @ W2, absCW + np.abs(Cm) @ np.abs(W2)
    within_bound("matern1 acc=%d" % accumulate, Yd.to_dense(), ref, N, absCW)
    assert np.array_equal(op.to_dense(), Cm)


def test_cross_rows_and_determinism(ctx):
    sigma, ell, nugget, N, M, r0, k = 1.1, 0.25, 0.3, 95, 37, 20, 17
    pts = scattered(N, 2, seed=4)
    W = np.random.default_rng(5).standard_normal((N, k))
    cross = hf.KernelCrossCovarianceOperator(pts[r0:r0 + M], pts, family="matern1", sigma=sigma, ell=ell, nugget=nugget, diag_offset=r0, ctx=ctx)
    K = hf.kernel_cross_cov_host(pts[r0:r0 + M], pts, "matern1", sigma, ell, nugget, diag_offset=r0)
    assert cross.shape == (M, N) and np.array_equal(cross.to_dense(), K)
    Yc = apply(cross, W, ctx).to_dense()
    within_bound("matern1 cross", Yc, K @ W, N, np.abs(K) @ np.abs(W))
    op = hf.KernelCovarianceOperator(pts, family="matern1", sigma=sigma, ell=ell, nugget=nugget, ctx=ctx)
    Y1, Y2 = apply(op, W, ctx).to_dense(), apply(op, W, ctx).to_dense()
    assert np.array_equal(Y1, Y2)                                           # two applies are bit-identical
    assert np.array_equal(Yc, Y1[r0:r0 + M])                                # the cross form with a diagonal IS those rows
    slab = op.rows(r0, r0 + M)
    assert slab.family == "matern1"
    Ys = apply(slab, W, ctx).to_dense()
    assert np.array_equal(Ys[r0:r0 + M], Y1[r0:r0 + M]) and not Ys[:r0].any() and not Ys[r0 + M:].any()


# ---------------------------------------------------------------------------------------------------------------- 3. the metric on scattered points
@pytest.mark.parametrize("family", ["matern1", "matern32"])
def test_diagonal_metric_is_a_scaling_of_the_points(ctx, family):
    """G = diag(4, 0.25): L = diag(2, 0.5) exactly, so the library is handed points * (2, 0.5) -- the bits of the isotropic operator"""
    N, k = 130, 9
    pts = scattered(N, 2, seed=8)
    W = np.random.default_rng(9).standard_normal((N, k))
    a = hf.KernelCovarianceOperator(pts, family=family, sigma=1.2, ell=0.4, nugget=0.1, metric=np.diag([4.0, 0.25]), ctx=ctx)
    b = hf.KernelCovarianceOperator(pts * np.array([2.0, 0.5]), family=family, sigma=1.2, ell=0.4, nugget=0.1, ctx=ctx)
    assert np.array_equal(a.points, pts) and np.array_equal(a.metric, np.diag([4.0, 0.25])) and b.metric is None
    assert np.array_equal(apply(a, W, ctx).to_dense(), apply(b, W, ctx).to_dense())


@pytest.mark.parametrize("name,d,G", [("rotated", 2, gt.rotated_metric()), ("full3d", 3, gt.FULL_3D)])
@pytest.mark.parametrize("family", ["matern1", "matern52"])
def test_metric_against_host(ctx, name, d, G, family):
    sigma, ell, nugget, N, k = 0.9, 0.5, 0.15, 150, 20
    pts = scattered(N, d, seed=30 + d)
    W = np.random.default_rng(31).standard_normal((N, k))
    op = hf.KernelCovarianceOperator(pts, family=family, sigma=sigma, ell=ell, nugget=nugget, metric=G, ctx=ctx)
    Cm = hf.kernel_cov_host(pts, family, sigma, ell, nugget, metric=G)
    within_bound("%s %s" % (name, family), apply(op, W, ctx).to_dense(), Cm @ W, N, np.abs(Cm) @ np.abs(W))
    iso = hf.kernel_cov_host(pts, family, sigma, ell, nugget)
    assert np.abs(Cm - iso).max() > 1e-3                                    # the metric is not a no-op here
    # the derived operators carry it
    T = scattered(11, d, seed=77)
    cross = hf.KernelCrossCovarianceOperator(T, pts, family=family, sigma=sigma, ell=ell, metric=G, ctx=ctx)
    K = hf.kernel_cross_cov_host(T, pts, family, sigma, ell, metric=G)
    within_bound("%s %s cross" % (name, family), apply(cross, W, ctx).to_dense(), K @ W, N, np.abs(K) @ np.abs(W))
    assert np.array_equal(cross.transpose().metric, G)
    Y = apply(op, W, ctx).to_dense()
    slab = op.rows(40, 90)
    assert np.array_equal(slab.metric, G) and np.array_equal(apply(slab, W, ctx).to_dense()[40:90], Y[40:90])
    assert np.array_equal(slab.to_dense()[40:90], Cm[40:90])


# ---------------------------------------------------------------------------------------------------------------- 4. pivoted Cholesky
def test_pivoted_cholesky_matern1_with_a_rotated_metric(ctx):
    """N = 300, rank 40: the order-free properties of tests/helpers/pchol_checks.py with its tolerances -- L L^T reproduces C on the
    pivot columns within 8 (rank + 2) eps (|L| |L_P|^T + |C_P|); the reported trace is N d0 - ||L[:, :j]||_F^2 within 8 (j + 2) N eps d0
    and bounds lam_i(C) - lam_i(L L^T) from above (0 from below) up to 16 N eps lam_0; the pivots are distinct."""
    N, rank, sigma, ell, nugget = 300, 40, 1.3, 0.4, 0.0
    G = gt.rotated_metric()
    pts = scattered(N, 2, seed=N + 2)
    op = hf.KernelCovarianceOperator(pts, family="matern1", sigma=sigma, ell=ell, nugget=nugget, metric=G, ctx=ctx)
    f = hf.pivoted_cholesky(op, rank)
    Lh, piv, trace = f.L.to_dense(), f.pivots, f.trace
    d0 = sigma * sigma + nugget
    assert f.rank == rank and Lh.shape == (N, rank) and piv[0] == 0
    assert len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < N
    assert not ({1, N - 1} <= set(piv.tolist())), "both points of the coincident pair were chosen"
    assert np.all(np.isfinite(Lh)) and np.all(np.diff(trace) <= 0.0)
    Cp = hf.kernel_cov_host(pts, "matern1", sigma, ell, nugget, rows=piv, metric=G).T
    Lp = Lh[piv, :]
    err = np.abs(Cp - Lh @ Lp.T)
    bound = 8 * (rank + 2) * EPS * (np.abs(Lh) @ np.abs(Lp).T + np.abs(Cp))
    print("pchol matern1 + metric: pivot columns max err/bound = %.3g" % float(np.max(err / bound)))
    assert np.all(err <= bound)
    sq = np.concatenate([[0.0], np.cumsum(np.sum(np.ascontiguousarray(Lh.T) ** 2, axis=1))])
    terr, tbound = np.abs(trace - (N * d0 - sq)), 8 * (np.arange(rank + 1) + 2) * N * EPS * d0
    print("pchol matern1 + metric: trace identity max err/bound = %.3g" % float(np.max(terr / tbound)))
    assert np.all(terr <= tbound)
    lam = np.linalg.eigvalsh(op.to_dense())[::-1]
    mu = np.zeros(N)
    mu[:rank] = np.linalg.eigvalsh(Lh.T @ Lh)[::-1]
    gap, slack = lam - mu, 16 * N * EPS * lam[0]
    print("pchol matern1 + metric: lam(C) - lam(L L^T) in [%.3g, %.3g], residual trace %.3g" % (gap.min(), gap.max(), trace[-1]))
    assert np.all(gap >= -slack) and np.all(gap <= trace[-1] + slack)
    # the factor at other points goes through the cross-covariance with the same metric: at the operator's own points it is L
    back = f.extend(pts[:50]).to_dense()
    assert np.abs(back - Lh[:50]).max() <= 1e-9 * np.abs(Lh).max()


# ---------------------------------------------------------------------------------------------------------------- 5. grids
def even_rule_apply(shape, spacing, family, sigma, ell, nugget, W, nodes, G):
    """what a column that kept min(j, P - j) would apply: the metric's quadratic form of the UNSIGNED offsets"""
    d = len(shape)
    P = [gt.embed_len(n) for n in shape]
    Lf = np.linalg.cholesky(G)
    view = lambda c: [-1 if a == c else 1 for a in range(d)][::-1]
    u = [(np.minimum(np.arange(P[c]), P[c] - np.arange(P[c])) * spacing[c]).reshape(view(c)) for c in range(d)]
    r2 = 0.0
    for c in range(d):
        r2 = r2 + sum(Lf[e, c] * u[e] for e in range(c, d)) ** 2
    col = sigma ** 2 * gt.phi(family, np.sqrt(r2) / ell)
    col[(0,) * d] += nugget
    lam = np.fft.fftn(col).real
    g = np.arange(int(np.prod(shape))) if nodes is None else nodes
    idx, rest = [], g
    for n in shape:
        idx.append(rest % n)
        rest = rest // n
    idx = tuple(idx[::-1])
    Y = np.empty(W.shape)
    for j in range(W.shape[1]):
        zpad = np.zeros(lam.shape)
        zpad[idx] = W[:, j]
        Y[:, j] = np.fft.ifftn(lam * np.fft.fftn(zpad))[idx].real
    return Y


@pytest.mark.parametrize("cid,shape,spacing,G,subset", gt.GRID_CASES, ids=[c[0] for c in gt.GRID_CASES])
@pytest.mark.parametrize("family", ["matern1", "matern32"])
def test_grid_apply_against_host(ctx, cid, shape, spacing, G, subset, family):
    """per column ||Y_j - Yref_j||_2 <= 32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W_j||_2 + 8 N eps || |C| |W_j| ||_2, the bound of
    tests/test_gpu_grid_kernel_cov.py::test_apply_against_host with the signed column c; a column of unsigned offsets misses it"""
    sigma, ell, nugget, k = 1.3, 0.45, 0.2, 5
    nodes = gt.case_nodes(shape, subset)
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=sigma, ell=ell, nugget=nugget, nodes=nodes, metric=G, ctx=ctx)
    pts = gt.points(shape, spacing, nodes)
    N = pts.shape[0]
    assert op.shape == (N, N) and np.array_equal(op.points, pts) and np.array_equal(op.metric, G)
    W = np.random.default_rng(N).standard_normal((N, k))
    Cm = hf.kernel_cov_host(pts, family, sigma, ell, nugget, metric=G)
    bound = gt.column_bounds(shape, spacing, family, sigma, ell, nugget, W, np.abs(Cm) @ np.abs(W), G)
    Y = apply(op, W, ctx).to_dense()
    ratio = np.linalg.norm(Y - Cm @ W, axis=0) / bound
    print("grid metric %s %s: worst err/bound = %.3g" % (cid, family, ratio.max()))
    assert np.all(np.isfinite(Y)) and ratio.max() <= 1.0
    wrong = even_rule_apply(shape, spacing, family, sigma, ell, nugget, W, nodes, G)
    assert (np.linalg.norm(wrong - Cm @ W, axis=0) / bound).min() > 1e6      # min(j, P - j) fails this test by orders of magnitude
    # matrix_free() is the scattered operator with the same kernel and metric
    mf = op.matrix_free()
    assert mf.family == family and np.array_equal(mf.metric, G)
    within_bound("grid matrix_free %s %s" % (cid, family), apply(mf, W, ctx).to_dense(), Cm @ W, N, np.abs(Cm) @ np.abs(W))


def test_grid_matern1_without_a_metric_and_scalar_metric(ctx):
    sigma, ell, k = 1.0, 0.3, 4
    for shape, spacing, G in (((6, 5), (0.2, 0.25), None), ((17,), (0.05,), 2.5), ((1, 7), (0.1, 0.3), None)):
        op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern1", sigma=sigma, ell=ell, metric=G, ctx=ctx)
        N = op.shape[0]
        W = np.random.default_rng(N).standard_normal((N, k))
        Gm = None if G is None else np.array([[G]])
        Cm = hf.kernel_cov_host(op.points, "matern1", sigma, ell, metric=Gm)
        bound = gt.column_bounds(shape, spacing, "matern1", sigma, ell, 0.0, W, np.abs(Cm) @ np.abs(W), Gm)
        ratio = np.linalg.norm(apply(op, W, ctx).to_dense() - Cm @ W, axis=0) / bound
        print("grid matern1 %r metric %r: worst err/bound = %.3g" % (shape, G, ratio.max()))
        assert ratio.max() <= 1.0


def test_grid_factor_of_the_rotated_kernel(ctx):
    """(6, 5): S S^T = C within cov_error_bound plus the rounding of tests/test_gpu_grid_factor.py -- the composition's
    bound_S(S^T X) + ||S||_2 bound_St(X) for X = I and the fp64 twin's own 64 eps log2(P) (sigma^2 + nugget)"""
    cid, shape, spacing, G, _ = gt.GRID_CASES[0]
    sigma, ell, nugget = 1.3, 0.45, 0.0
    for family in ("matern1", "matern32"):
        op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=sigma, ell=ell, nugget=nugget, metric=G, ctx=ctx)
        s = op.sampler(max_growth=3, on_indefinite="clip")
        S = s.factor()
        N, Ptot = S.shape
        assert Ptot == int(np.prod(s.embedding))
        X = np.eye(N)
        V, Y = hf.MultiVector(Ptot, N, ctx=ctx), hf.MultiVector(N, N, ctx=ctx)
        S.transpose().matMvMult(hf.MultiVector.from_dense(X, ctx=ctx), V)
        S.matMvMult(V, Y)
        lam = gt.spectrum(shape, spacing, family, sigma, ell, nugget, G, growth=s.growth).real
        root = np.sqrt(np.maximum(lam, 0.0))
        rounding = gf.column_bounds(root, V.to_dense()) + root.max() * gf.column_bounds(root, X) + gf.twin_tolerance(Ptot, sigma, nugget)
        diff = np.abs(Y.to_dense() - op.to_dense()).max(axis=0)
        print("grid factor %s: growth %d clipped %d bound %.3g; max |S S^T - C| %.3g, allowed %.3g"
              % (family, s.growth, s.n_clipped, s.cov_error_bound, diff.max(), (s.cov_error_bound + rounding).min()))
        assert np.all(diff <= s.cov_error_bound + rounding)
        draws = s.sample(4, seed=3).to_dense()
        assert draws.shape == (N, 4) and np.all(np.isfinite(draws)) and np.abs(draws).max() > 0.0


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
class _MassOnly:
    pass


def test_bilaplacian_prior_end_to_end(ctx):
    """GridKernelPrior of the BiLaplacian's kernel on a 9 x 8 grid: draws are finite, and the KLE through KLEProjector has the eigenvalues
    of the dense host pencil -- V^T M V = I and E = M V to 1e-10, residual below 1e-4, eigenvalues within 1e-10 d_0 of those the explicit
    matrix gives on the same route (the tolerances of test_gpu_kernel_cov.py::test_kle_equivalence_with_the_explicit_matrix), and within the
    residual of scipy's eigh."""
    import scipy.linalg as sla
    shape, spacing = (9, 8), (0.11, 0.13)
    kw = hf.bilaplacian_kernel_2d(0.1, 1.0)
    op = hf.GridKernelCovarianceOperator(shape, spacing, ctx=ctx, **kw)
    N, r = op.shape[0], 12
    # the kernel is rough: the pencil's eigenvalues fall like k^-2 (lambda_60 / lambda_1 = 1e-3), and in numpy the one-pass residual with 60
    # probes is 2e-3.  With as many probes as points the pass spans the space and the 1e-4 below tests the operators, not the sketch.
    p = N - r
    mdiag = (0.5 + np.random.default_rng(2).random(N)) / N
    M = sp.diags(mdiag).tocsr()
    prior = hf.GridKernelPrior(op, M=M, on_indefinite="clip")
    draws = prior.sample_block(4)
    assert draws.shape == (4, N) and np.all(np.isfinite(draws)) and np.abs(draws).max() > 0.0
    Cm = hf.kernel_cov_host(op.points, **kw)
    assert np.array_equal(op.to_dense(), Cm)
    MCM = mdiag[:, None] * Cm * mdiag[None, :]
    exact = sla.eigh(MCM, np.diag(mdiag), eigvals_only=True)[::-1]
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
        res = np.linalg.norm(MCM @ V - (M @ V) * d) / np.linalg.norm(MCM @ V)
        print("bilaplacian KLE [%s]: residual %.3g, max |d - eigh| / d_0 = %.3g" % (name, res, np.abs(d - exact[:r]).max() / exact[0]))
        assert res < 1e-4 and np.abs(d - exact[:r]).max() <= 1e-4 * exact[0]
        results[name] = d
    gap = np.abs(results["grid"] - results["explicit"]).max() / results["explicit"][0]
    print("bilaplacian KLE: max |delta d| / d_0 between the grid operator and the explicit matrix = %.3g" % gap)
    assert gap <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- 7. arguments
def test_invalid_arguments(ctx):
    pts = L.as_f64(scattered(9, 2, seed=1))
    out = C.c_void_p()
    lib = L.load()

    def spec(family=4, d=2, sigma=1.0, ell=0.2, nugget=0.0, metric=None):
        s = L.KernelSpec(family, d, sigma, ell, nugget)
        for i, v in enumerate(np.zeros(9) if metric is None else np.asarray(metric, dtype=np.float64).ravel()):
            s.metric[i] = v
        return s

    def cov(s, d=2):
        return lib.hfmi_op_kernel_cov_spec(ctx.handle, L.ptr(pts), 9, d, C.byref(s), C.byref(out))

    bad = [spec(metric=[[2.0, 0.5], [0.6, 1.0]]), spec(metric=[[1.0, 2.0], [2.0, 1.0]]), spec(metric=[[1.0, 0.0], [0.0, np.nan]]),
           spec(family=5), spec(family=-1), spec(ell=0.0), spec(nugget=-1.0), spec(d=3)]
    for s in bad:
        assert cov(s) == HFMI_ERR_INVALID
    assert cov(spec(d=0), d=0) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cov_spec(ctx.handle, L.ptr(pts), 9, 2, None, C.byref(out)) == HFMI_ERR_INVALID
    n, h = np.array([3, 3], dtype=np.int64), np.array([0.1, 0.1])
    for s in bad:
        assert lib.hfmi_op_kernel_cross_cov_spec(ctx.handle, L.ptr(pts[:3]), 3, L.ptr(pts), 9, 2, C.byref(s), 0, C.byref(out)) == HFMI_ERR_INVALID
        assert lib.hfmi_op_kernel_cov_rows_spec(ctx.handle, L.ptr(pts), 9, 2, C.byref(s), 0, 3, C.byref(out)) == HFMI_ERR_INVALID
        assert lib.hfmi_op_kernel_cov_grid_spec(ctx.handle, 2, L.ptr(n), L.ptr(h), None, 9, C.byref(s), C.byref(out)) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cov_grid_spec(ctx.handle, 0, L.ptr(n), L.ptr(h), None, 9, C.byref(spec(d=0)), C.byref(out)) == HFMI_ERR_INVALID
    # a good descriptor works, and the creators with a bare family still refuse family 4
    good = spec(metric=[[2.0, 0.5], [0.5, 1.0]])
    assert cov(good) == 0
    lib.hfmi_op_destroy(out)
    assert lib.hfmi_op_kernel_cov(ctx.handle, L.ptr(pts), 9, 2, 4, 1.0, 0.2, 0.0, C.byref(out)) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cross_cov(ctx.handle, L.ptr(pts[:3]), 3, L.ptr(pts), 9, 2, 4, 1.0, 0.2, 0.0, 0, C.byref(out)) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cov_rows(ctx.handle, L.ptr(pts), 9, 2, 4, 1.0, 0.2, 0.0, 0, 3, C.byref(out)) == HFMI_ERR_INVALID
    assert lib.hfmi_op_kernel_cov_grid(ctx.handle, 2, L.ptr(n), L.ptr(h), None, 9, 4, 1.0, 0.2, 0.0, C.byref(out)) == HFMI_ERR_INVALID
    # Python: ValueError before the library is asked
    for G in ([[2.0, 0.5], [0.6, 1.0]], [[1.0, 2.0], [2.0, 1.0]], [[1.0, 0.0], [0.0, np.nan]]):
        with pytest.raises(ValueError):
            hf.KernelCovarianceOperator(pts, family="matern1", metric=G, ctx=ctx)
        with pytest.raises(ValueError):
            hf.GridKernelCovarianceOperator((3, 3), 0.1, family="matern32", metric=G, ctx=ctx)
    with pytest.raises(ValueError):
        hf.KernelCovarianceOperator(pts, family="matern72", ctx=ctx)
