"""The factor K = F F^T, F = [W S | diag(sqrt(delta))], of the interpolated grid covariance (``InterpolatedFieldSampler.factor`` ->
``InterpolatedCovarianceFactor``, hfmi_op_interp_factor, hfmi_interp.hip) and the prior over it (``InterpolatedKernelPrior``) on the
device: F and F^T against the public steps they are made of (bit for bit where the kernels are the same), adjointness against the
numpy twin's own defect (tests/helpers/interp_factor_twin.py), F (F^T X) against K X, the clipped embedding against the reported bound,
repetition / chunking / point order, the block storage contract, lifetimes and refusals, the prior protocol, ``doublePassC`` and the
active-subspace projector over scattered points, and ``KLEProjector.extend`` through ``C.cross``."""
import ctypes as C
import functools
import gc
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402
import fake_pde as fp                             # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import grid_factor_twin as gf                     # noqa: E402
import interp_factor_twin as tw                   # noqa: E402
import interp_twin as it                          # noqa: E402
from oracle import hippylib_restated as hl        # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = tw.EPS
TINY = np.finfo(np.float64).tiny
SIGMA = tw.SIGMA
COLUMNS = (1, 2, 3, 5)
# grid and points: tests/test_gpu_grid_interp.py::_points (interp_factor_twin.points); (family, ell, nugget)
KERNELS = {"d1": ("matern32", 1.0, 0.0), "d2": ("matern52", 0.45, 0.01), "d3": ("matern32", 0.3, 0.02), "big": ("matern52", 0.2, 0.0)}
# (case, forced growth): d2 at growth 0 is clipped, the others are definite (d3 at growth 2: lambda_min / lambda_max = 4.3e-6)
CASES = [("d1", 0), ("d2", 2), ("d2", 0), ("d3", 2), ("big", 0)]
DEFINITE = [c for c in CASES if c != ("d2", 0)]
PTOT = {("d2", 2): 8192, ("d3", 2): 262144, ("big", 0): 256 * 256}


def ids(cases):
    return ["%s-g%d" % c for c in cases]


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def sampler_at(K, growth):
    """a sampler of K on the embedding of growth ``growth`` whatever its spectrum (negative eigenvalues clipped)"""
    L.call("hfmi_tuning_set", b"fftcov_min_growth", growth)
    try:
        s = K.sampler(max_growth=growth, on_indefinite="clip")
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
    assert s.growth == growth
    return s


def make(ctx, name, growth, nugget=None, diag_correction=True, pts=None):
    shape, h, o, p0 = tw.points(name)
    family, ell, nug = KERNELS[name]
    grid = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, origin=o, ctx=ctx)
    K = hf.InterpolatedKernelCovarianceOperator.on_grid(grid, p0 if pts is None else pts, nugget=nug if nugget is None else nugget,
                                                        diag_correction=diag_correction)
    s = sampler_at(K, growth)
    return K, s, s.factor()


def dev(A, ctx):
    return hf.MultiVector.from_dense(np.asfortranarray(A), ctx=ctx)


def apply(op, X, ctx, accumulate_onto=None):
    Y = hf.MultiVector(op.shape[0], X.shape[1], ctx=ctx) if accumulate_onto is None else dev(accumulate_onto, ctx)
    op.matMvMult(dev(X, ctx), Y, accumulate=accumulate_onto is not None)
    return Y.to_dense()


@functools.lru_cache(maxsize=None)
def twin_dense(name):
    """(W, Cg, ||W||_2) of a case from the twin's weights, computed once (as tests/test_gpu_grid_interp.py::twin_dense)"""
    shape, h, o, pts = tw.points(name)
    family, ell, _ = KERNELS[name]
    base, w, _ = it.cell_and_weights(shape, h, o, pts)
    W = it.dense_W(shape, base, w)
    Cg = hf.kernel_cov_host(ft.points(shape, h, origin=o), family, SIGMA, ell)
    nW = float(scipy.sparse.linalg.svds(W, k=1, return_singular_vectors=False)[0]) if min(W.shape) > 2 else float(np.linalg.norm(W, 2))
    return W, Cg, nW


@functools.lru_cache(maxsize=None)
def root_of(name, growth):
    shape, h, _, _ = tw.points(name)
    family, ell, _ = KERNELS[name]
    return gf.root_spectrum(shape, h, family, SIGMA, ell, 0.0, growth)


def rounding_bound(name, growth, X, delta):
    """per column, what F (F^T X) and K X may differ by in rounding: the sum of the component bounds as
    test_gpu_grid_factor.py::test_factor_times_transpose_is_the_operators_apply composes them on the spread column G = W^T X -- the grid
    apply's FFT term, bound_S(S^T G) + ||S||_2 bound_St(G) -- scaled by ||W||_2^2, plus 64 eps 4^d per gather or spread (two each way) on
    the size of the sums they form, (|W| |Cg| |W^T| + diag(delta)) |X|"""
    shape, h, _, _ = tw.points(name)
    family, ell, _ = KERNELS[name]
    Wd, Cg, nW = twin_dense(name)
    root = root_of(name, growth)
    G = Wd.T @ X
    v = gf.apply_St(root, shape, G)
    comp = ft.column_bounds(shape, h, family, SIGMA, ell, 0.0, G, np.zeros_like(G)) + gf.column_bounds(root, v) + root.max() * gf.column_bounds(root, G)
    mag = np.abs(Wd) @ (np.abs(Cg) @ (np.abs(Wd.T) @ np.abs(X))) + delta[:, None] * np.abs(X)
    return nW ** 2 * comp + 4 * 64.0 * EPS * 4 ** len(shape) * mag.max(axis=0)


# ------------------------------------------------------------------------------------------------- 1. against the public steps
@pytest.mark.parametrize("name,growth", CASES, ids=ids(CASES))
def test_factor_and_transpose_against_the_public_steps(ctx, name, growth):
    """1, 2, 3 and 5 columns, overwriting and accumulating.  F^T X: the first Ptot rows are the bits of S^T (W^T X) through the public
    operators (the same kernels in the same order), the tail is sqrt(delta) X exactly.  F Xi: with g = W (S Xi_top) from the public
    operators and t = sqrt(delta) Xi_tail, |F Xi - (g + t)| <= 2 eps (|g| + |t|), one fused multiply-add against a multiply and an add.
    An accumulating apply may round its sum once more: 2 eps (|Y0| + |ref|) on top."""
    K, s, F = make(ctx, name, growth)
    S, W = s.grid_sampler.factor(), K.W
    N, Ptot = K.shape[0], int(np.prod(s.embedding))
    assert F.shape == (N, Ptot + N) and F.noise_split == (Ptot, N) and F.transpose().shape == (Ptot + N, N)
    assert F.transpose().transpose() is F and s.factor().sampler is s and PTOT.get((name, growth), Ptot) == Ptot
    assert (s.n_clipped > 0) == ((name, growth) == ("d2", 0))
    assert F.factor_error_bound == 1.25 ** (2 * len(s.embedding)) * s.cov_error_bound and (s.n_clipped > 0 or F.factor_error_bound == 0.0)
    sd = np.sqrt(K.delta)
    rng = np.random.default_rng(Ptot + N)
    worst = 0.0
    for k in COLUMNS:
        Xi, X = rng.standard_normal((Ptot + N, k)), rng.standard_normal((N, k))
        top = apply(S.transpose(), apply(W.transpose(), X, ctx), ctx)
        Z = apply(F.transpose(), X, ctx)
        assert np.array_equal(Z[:Ptot], top) and np.array_equal(Z[Ptot:], sd[:, None] * X) and np.abs(top).max() > 0.01
        ref = np.concatenate([top, sd[:, None] * X])
        Z0 = rng.standard_normal((Ptot + N, k))
        Za = apply(F.transpose(), X, ctx, accumulate_onto=Z0)
        assert np.all(np.abs(Za - Z0 - ref) <= 2.0 * EPS * (np.abs(Z0) + np.abs(ref)))
        g, t = apply(W, apply(S, Xi[:Ptot], ctx), ctx), sd[:, None] * Xi[Ptot:]
        Y = apply(F, Xi, ctx)
        fma = 2.0 * EPS * (np.abs(g) + np.abs(t)) + TINY
        worst = max(worst, np.max(np.abs(Y - (g + t)) / fma))
        Y0 = rng.standard_normal((N, k))
        Ya = apply(F, Xi, ctx, accumulate_onto=Y0)
        assert np.all(np.abs(Ya - Y0 - (g + t)) <= fma + 2.0 * EPS * (np.abs(Y0) + np.abs(g + t)))
    print("interp factor %s g=%d (Ptot = %d, N = %d): worst |F Xi - (g + t)| / bound = %.3g" % (name, growth, Ptot, N, worst))
    assert worst <= 1.0
    # single-vector route and the lengths init_vector gives
    x1, y1 = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    F.init_vector(x1, 1)
    F.init_vector(y1, 0)
    assert (x1.size(), y1.size()) == (Ptot + N, N)


@pytest.mark.parametrize("name,growth", CASES, ids=ids(CASES))
def test_without_a_diagonal_the_factor_is_the_gather(ctx, name, growth):
    """nugget 0 and no diagonal correction: delta = 0, F Xi is W (S Xi_top) bit for bit whatever the tail holds, the tail of F^T X is +0.0"""
    K, s, F = make(ctx, name, growth, nugget=0.0, diag_correction=False)
    assert np.all(K.delta == 0.0)
    N, Ptot = F.noise_split[1], F.noise_split[0]
    rng = np.random.default_rng(N)
    Xi, X = rng.standard_normal((Ptot + N, 3)), rng.standard_normal((N, 3))
    g = apply(K.W, apply(s.grid_sampler.factor(), Xi[:Ptot], ctx), ctx)
    assert np.array_equal(apply(F, Xi, ctx), g) and np.abs(g).max() > 0.01
    tail = apply(F.transpose(), X, ctx)[Ptot:]
    assert np.all(tail == 0.0)


# ------------------------------------------------------------------------------------------------- 2. adjointness
@pytest.mark.parametrize("name,growth", [("d1", 0), ("d2", 2)], ids=ids([("d1", 0), ("d2", 2)]))
def test_adjointness_against_the_twins_own_defect(ctx, name, growth):
    """<F Xi, X> = <Xi, F^T X> per column with a defect, relative to |F Xi| |X|, of at most 4 times the numpy twin's own on the same
    inputs plus 64 eps"""
    K, s, F = make(ctx, name, growth)
    family, ell, nugget = KERNELS[name]
    t = tw.build(name, family, ell, growth, nugget=nugget)
    N, Ptot = t["N"], t["Ptot"]
    assert F.noise_split == (Ptot, N)
    rng = np.random.default_rng(Ptot)
    worst = 0.0
    for k in COLUMNS:
        Xi, X = rng.standard_normal((Ptot + N, k)), rng.standard_normal((N, k))
        refF = tw.apply_F(t, Xi)
        scale = np.linalg.norm(refF, axis=0) * np.linalg.norm(X, axis=0)
        twin = tw.adjoint_defect(t, Xi, X)
        Yd, Zd = apply(F, Xi, ctx), apply(F.transpose(), X, ctx)
        mine = np.abs(np.sum(Yd * X, axis=0) - np.sum(Xi * Zd, axis=0)) / scale
        worst = max(worst, (mine / (4.0 * twin + 64.0 * EPS)).max())
    print("interp factor %s g=%d: worst adjointness defect / allowance = %.3g" % (name, growth, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- 3. F F^T X against K X
def factor_times_transpose(ctx, K, F, X):
    Xd = dev(X, ctx)
    n, k = F.shape[1], X.shape[1]
    V, Y, KX = hf.MultiVector(n, k, ctx=ctx), hf.MultiVector(F.shape[0], k, ctx=ctx), hf.MultiVector(F.shape[0], k, ctx=ctx)
    F.transpose().matMvMult(Xd, V)
    F.matMvMult(V, Y)
    K.matMvMult(Xd, KX)
    return Y.to_dense(), KX.to_dense()


@pytest.mark.parametrize("name,growth", DEFINITE, ids=ids(DEFINITE))
def test_factor_times_transpose_is_the_operators_apply(ctx, name, growth):
    """Definite embeddings: F (F^T X) against the operator's own K X within ``rounding_bound``"""
    K, s, F = make(ctx, name, growth)
    assert s.n_clipped == 0 and F.factor_error_bound == 0.0
    N = K.shape[0]
    X = np.random.default_rng(N).standard_normal((N, 3))
    Y, KX = factor_times_transpose(ctx, K, F, X)
    ratio = (np.abs(Y - KX).max(axis=0) / rounding_bound(name, growth, X, K.delta)).max()
    print("F F^T X - K X %s g=%d: worst ratio to the sum of the bounds %.3g" % (name, growth, ratio))
    assert ratio <= 1.0 and np.abs(KX).max() > 0.1


def test_clipped_factor_misses_the_apply_by_the_reported_bound(ctx):
    """d2 at growth 0: S S^T = Cg + E with |E_ij| <= cov_error_bound, F F^T = K + W E W^T with |W E W^T|_ij <= factor_error_bound, so column
    by column max_i |F F^T X - K X| <= factor_error_bound ||X_j||_1 plus the rounding bound of the definite case -- and it is larger than
    that rounding bound, so the reported bound is what holds it"""
    K, s, F = make(ctx, "d2", 0)
    assert s.n_clipped > 0 and s.cov_error_bound > 0.0 and F.factor_error_bound == 1.25 ** 4 * s.cov_error_bound
    N = K.shape[0]
    X = np.random.default_rng(4).standard_normal((N, 4))
    Y, KX = factor_times_transpose(ctx, K, F, X)
    diff = np.abs(Y - KX).max(axis=0)
    rounding = rounding_bound("d2", 0, X, K.delta)
    allowed = F.factor_error_bound * np.abs(X).sum(axis=0) + rounding
    print("clipped d2: max |F F^T X - K X| %s, allowed %s, rounding %s" % (diff, allowed, rounding))
    assert np.all(diff <= allowed) and np.all(diff > rounding)


# ------------------------------------------------------------------------------------------------- 5. repetition, chunking, point order
@pytest.mark.parametrize("name,growth", [("d3", 2), ("big", 0)], ids=ids([("d3", 2), ("big", 0)]))
def test_repetition_chunking_and_point_order(ctx, name, growth):
    """Two applies are bit-identical; "fftcov_pairs" = 1, 2 and the default give the same bits both ways (5 columns: three chunks at 1);
    the same points in another order permute the rows of F and the noise tail and change nothing else, bit for bit.  (The spread sums
    the points of a cell in ascending point index, so F^T keeps its bits under the permutations that keep that order inside every
    cell: the cell binning's own is one, and it moves almost every point of the 5000.)"""
    K, s, F = make(ctx, name, growth)
    N, Ptot = K.shape[0], F.noise_split[0]
    rng = np.random.default_rng(N + 5)
    Xi, X = rng.standard_normal((Ptot + N, 5)), rng.standard_normal((N, 5))
    y0, z0 = apply(F, Xi, ctx), apply(F.transpose(), X, ctx)
    assert np.array_equal(apply(F, Xi, ctx), y0) and np.array_equal(apply(F.transpose(), X, ctx), z0)
    assert np.abs(y0).max() > 0.1 and np.abs(z0[:Ptot]).max() > 0.01
    try:
        for pairs in (1, 2, 0):
            L.call("hfmi_tuning_set", b"fftcov_pairs", pairs)
            assert np.array_equal(apply(F, Xi, ctx), y0) and np.array_equal(apply(F.transpose(), X, ctx), z0), pairs
    finally:
        L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    shape, h, o, pts = tw.points(name)
    for p in (rng.permutation(N), K.W.weights(bins=True)[3]):
        Kp, sp, Fp = make(ctx, name, growth, pts=pts[p])
        assert np.array_equal(Kp.delta, K.delta[p])
        assert np.array_equal(apply(Fp, np.concatenate([Xi[:Ptot], Xi[Ptot:][p]]), ctx), y0[p])
        zp = apply(Fp.transpose(), X[p], ctx)
        assert np.array_equal(zp[Ptot:], z0[Ptot:][p])
    assert not np.array_equal(p, np.arange(N)) and np.array_equal(zp[:Ptot], z0[:Ptot])      # the binning's permutation, the last one


# ------------------------------------------------------------------------------------------------- 6. block contract
@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
@pytest.mark.parametrize("name,growth", [("d2", 2), ("big", 0)], ids=ids([("d2", 2), ("big", 0)]))
def test_block_contract_of_both_operators(ctx, name, growth, layout):
    """Y a view inside a wider parent with guard columns, for F (length N) and for F^T (length Ptot + N): padding rows stay +0.0,
    nothing outside Y's window changes, an overwriting apply equals the apply into a plain block bit for bit and an accumulating one
    adds it; the input a column view of a wider block; blocks of another length are refused with a message that names the operator
    and the four lengths.  (A block has at least one column -- hfmi_block_create and hfmi_block_view refuse fewer -- so the no-op on
    zero columns that the C entry keeps cannot be reached from here.)"""
    K, s, F = make(ctx, name, growth)
    N, Ptot = F.noise_split[1], F.noise_split[0]
    k, guard = 3, 2
    rng = np.random.default_rng(N)
    for fac, nin, nout in ((F, Ptot + N, N), (F.transpose(), N, Ptot + N)):
        wide = dev(rng.standard_normal((nin, k + 2)), ctx)
        Xin = wide.view(1, k)                                   # columns 1 .. k of a wider block
        plain = hf.MultiVector(nout, k, ctx=ctx)
        fac.matMvMult(dev(wide.to_dense()[:, 1:1 + k], ctx), plain)
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
            fac.matMvMult(Xin, y.mv, accumulate=accumulate)
            a.check(written=[y], what="hfmi_op_apply of %s accumulate=%d [%s]" % ("F^T" if fac.is_transpose else "F", accumulate, layout))
            assert np.array_equal(y.mv.to_dense(), before + D if accumulate else D), accumulate
        for bad_in, bad_out in ((nin + 1, nout), (nin, nout + 1), (nout, nin)):
            with pytest.raises(hf.HfmiError, match=r"F\^T maps" if fac.is_transpose else "F maps") as e:
                fac.matMvMult(hf.MultiVector(bad_in, k, ctx=ctx), hf.MultiVector(bad_out, k, ctx=ctx))
            assert all(str(v) in str(e.value) for v in (nin, nout, bad_in, bad_out))


# ------------------------------------------------------------------------------------------------- 7. lifetimes and refusals
def test_the_factor_outlives_sampler_and_prior_and_refusals(ctx):
    K, s, F = make(ctx, "d2", 2)
    N, Ptot = F.noise_split[1], F.noise_split[0]
    rng = np.random.default_rng(0)
    Xi = rng.standard_normal((Ptot + N, 2))
    y0 = apply(F, Xi, ctx)
    # the Python objects: the factor keeps its sampler alive, the sampler the operator
    prior = hf.InterpolatedKernelPrior(K, max_growth=3)
    F2 = prior.F
    assert F2.noise_split == (Ptot, N) and prior.growth == 2
    del prior, s, K
    gc.collect()
    assert np.array_equal(apply(F2, Xi, ctx), y0) and np.array_equal(apply(F, Xi, ctx), y0)
    # the C objects: destroy the grid sampler first, the operator made from it still applies (shared state)
    K, s, F = make(ctx, "d2", 2)
    handle, fac, out = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.call("hfmi_grid_sampler_create", K.grid._op, 3, 0, C.byref(handle))
    L.call("hfmi_op_interp_factor", K._op, handle, 0, C.byref(fac))
    L.call("hfmi_grid_sampler_destroy", handle)
    gc.collect()
    Xd, Y2 = dev(Xi, ctx), hf.MultiVector(N, 2, ctx=ctx)       # named: a block must outlive the raw call that takes its handle
    L.call("hfmi_op_apply", fac, Xd.handle, Y2.handle, 0)
    L.call("hfmi_op_destroy", fac)
    assert np.array_equal(Y2.to_dense(), y0)
    # refusals
    for transpose in (-1, 2):
        with pytest.raises(hf.HfmiError, match="transpose = %d" % transpose):
            L.call("hfmi_op_interp_factor", K._op, s.grid_sampler.handle, transpose, C.byref(out))
    with pytest.raises(hf.HfmiError, match="hfmi_op_kernel_cov_interp"):
        L.call("hfmi_op_interp_factor", K.grid._op, s.grid_sampler.handle, 0, C.byref(out))         # not an interpolated operator
    with pytest.raises(hf.HfmiError):
        L.call("hfmi_op_interp_factor", K._op, None, 0, C.byref(out))
    shape, h, o, pts = tw.points("d2")
    family, ell, _ = KERNELS["d2"]
    other = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=2 * ell, origin=o, ctx=ctx)
    with pytest.raises(hf.HfmiError, match="grid covariance"):
        L.call("hfmi_op_interp_factor", K._op, other.sampler(on_indefinite="clip").handle, 0, C.byref(out))
    assert not out.value
    with pytest.raises(ValueError):
        hf.InterpolatedCovarianceFactor(K)
    with pytest.raises(ValueError):
        hf.InterpolatedCovarianceFactor(K.grid.sampler(on_indefinite="clip"))
    with pytest.raises(ValueError):
        hf.InterpolatedKernelPrior(K.grid)
    for bad_in, bad_out in ((Ptot + N + 1, N), (Ptot + N, N + 1), (Ptot, N)):
        with pytest.raises(hf.HfmiError):
            F.matMvMult(hf.MultiVector(bad_in, 2, ctx=ctx), hf.MultiVector(bad_out, 2, ctx=ctx))


def test_a_long_route_operator_gives_the_default_routes_values(ctx):
    """d2 at growth 2 with ``long_axes=True`` and "fftcov_max_line" = 16 at creation, so the axis padded to 128 is split: F and F^T agree
    with the default route's within the long route's tolerance (tests/test_gpu_grid_long.py: whole columns within twice the FFT term of
    the column bound), here for both routes' transforms and passed through W: ||diff_j||_2 <= 2 ||W||_2 bound_S(Xi_top) for F, and
    2 bound_St(W^T X) for the first Ptot rows of F^T; the tail is the same bits."""
    K, s, F = make(ctx, "d2", 2)
    shape, h, o, pts = tw.points("d2")
    family, ell, nugget = KERNELS["d2"]
    L.call("hfmi_tuning_set", b"fftcov_max_line", 16)
    try:
        grid = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, origin=o, ctx=ctx, long_axes=True)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_max_line", 4096)
    Kl = hf.InterpolatedKernelCovarianceOperator.on_grid(grid, pts, nugget=nugget)
    sl = sampler_at(Kl, 2)
    Fl = sl.factor()
    assert Kl.long_axes and sl.embedding == s.embedding == (128, 64) and Fl.shape == F.shape and np.array_equal(Kl.delta, K.delta)
    N, Ptot = F.noise_split[1], F.noise_split[0]
    Wd, _, nW = twin_dense("d2")
    root = root_of("d2", 2)
    rng = np.random.default_rng(16)
    Xi, X = rng.standard_normal((Ptot + N, 3)), rng.standard_normal((N, 3))
    dy = np.linalg.norm(apply(Fl, Xi, ctx) - apply(F, Xi, ctx), axis=0)
    zl, z = apply(Fl.transpose(), X, ctx), apply(F.transpose(), X, ctx)
    dz = np.linalg.norm(zl[:Ptot] - z[:Ptot], axis=0)
    by, bz = 2.0 * nW * gf.column_bounds(root, Xi[:Ptot]), 2.0 * gf.column_bounds(root, Wd.T @ X)
    print("long route against the default: F %.3g, F^T %.3g of the bounds" % ((dy / by).max(), (dz / bz).max()))
    assert np.all(dy <= by) and np.all(dz <= bz) and np.array_equal(zl[Ptot:], z[Ptot:])


# ------------------------------------------------------------------------------------------------- 8. the prior protocol
def host_vector(values=None, n=None):
    v = hf.HostVector()
    v.init(len(values) if values is not None else n)
    if values is not None:
        v.set_local(np.asarray(values, dtype=np.float64))
    return v


@pytest.mark.parametrize("name", ["d1", "d2"])
def test_sample_is_the_mean_plus_the_factor_of_the_noise(ctx, name):
    shape, h, o, pts = tw.points(name)
    family, ell, nugget = KERNELS[name]
    grid = hf.GridKernelCovarianceOperator(shape, h, family=family, sigma=SIGMA, ell=ell, origin=o, ctx=ctx)
    K = hf.InterpolatedKernelCovarianceOperator.on_grid(grid, pts, nugget=nugget)
    N = K.shape[0]
    mean = 0.2 * np.cos(np.linspace(0.0, np.pi, N))
    prior = hf.InterpolatedKernelPrior(K, mean=mean, max_growth=3)
    Ptot = int(np.prod(prior.embedding))
    assert prior.F.shape == (N, Ptot + N) and prior.C is K and prior.n_clipped == 0
    assert prior.cov_error_bound == 0.0 and prior.factor_error_bound == 0.0
    assert prior.growth == prior.sampler.growth and np.array_equal(prior.mean.get_local(), mean)
    noise, m, x = hf.HostVector(), hf.HostVector(), hf.HostVector()
    prior.init_vector(noise, "noise")
    prior.init_vector(m, 0)
    prior.init_vector(x, 1)
    assert (noise.size(), m.size(), x.size()) == (Ptot + N, N, N)
    hf.parRandom.reseed(5)
    hf.parRandom.normal(1.0, noise)                       # the reference's loop: parRandom.normal(1., noise); prior.sample(noise, m)
    xi = noise.get_local().copy()
    assert abs(xi.std() - 1.0) < 5.0 / np.sqrt(2.0 * xi.size)      # five standard errors of a sample deviation (39 entries on d1)
    prior.sample(noise, m)
    Y = apply(prior.F, xi[:, None], ctx)[:, 0]
    assert np.array_equal(m.get_local(), mean + Y)
    prior.sample(noise, m, add_mean=False)
    assert np.array_equal(m.get_local(), Y)
    # device vectors take the same route
    nd, md = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    prior.init_vector(nd, "noise")
    prior.init_vector(md, 0)
    L.call("hfmi_block_upload", nd._mv.handle, L.ptr(L.as_f64(xi[None, :])), L.LAYOUT_VECTORS)
    prior.sample(nd, md)
    assert np.array_equal(md._mv.to_vectors()[0], mean + Y)
    # the precision is absent by design, and says where to go instead
    assert not hasattr(prior, "R") and not hasattr(prior, "Hlr")
    with pytest.raises(AttributeError, match="doublePassC"):
        prior.R
    # Rsolver.solve(y, x) is y = K x on host vectors
    y = host_vector(n=N)
    prior.Rsolver.solve(y, host_vector(values=mean))
    assert np.array_equal(y.get_local(), apply(K, mean[:, None], ctx)[:, 0])
    # sample_block stays the generated-noise draw
    blk = prior.sample_block(4)
    ref = K.sampler(max_growth=3).sample_block(4) + mean[None, :]
    assert blk.shape == (4, N) and np.array_equal(blk, ref)
    with pytest.raises(ValueError, match="the noise has"):
        prior.sample(host_vector(n=Ptot), m)
    with pytest.raises(ValueError):
        hf.InterpolatedKernelPrior(hf.npToDeviceOperator(np.eye(4), ctx=ctx))
    with pytest.raises(ValueError, match="the mean has"):
        hf.InterpolatedKernelPrior(K, mean=np.zeros(N + 1))


def test_the_statistics_of_the_factor_of_white_noise(ctx):
    """4000 ``parRandom`` noise vectors through F on d1: the sample variance of every point (mean known to be zero) within 5 standard
    errors K_ii sqrt(2 / n) of a chi-square variance estimate of ``K.to_dense()``'s diagonal, and the covariances within 5 standard
    errors sqrt((K_ii K_jj + K_ij^2) / n)"""
    K, s, F = make(ctx, "d1", 0)
    N, Ptot = F.noise_split[1], F.noise_split[0]
    n = 4000
    Xi = hf.MultiVector(Ptot + N, n, ctx=ctx)
    hf.parRandom.reseed(13)
    hf.parRandom.normal(1.0, Xi)
    Y = hf.MultiVector(N, n, ctx=ctx)
    F.matMvMult(Xi, Y)
    Yd = Y.to_dense()
    Kd = K.to_dense()
    cov = Yd @ Yd.T / n
    dg = np.diag(Kd)
    se = np.sqrt((np.outer(dg, dg) + Kd ** 2) / n)          # sqrt(2 / n) K_ii on the diagonal
    print("factor statistics d1: worst |cov - K| / standard error = %.3g" % np.max(np.abs(cov - Kd) / se))
    assert np.all(np.abs(np.diag(cov) - dg) <= 5.0 * dg * np.sqrt(2.0 / n)) and np.all(np.abs(cov - Kd) <= 5.0 * se)


# ------------------------------------------------------------------------------------------------- 9. doublePassC, the projector
DPC_RANK, DPC_OVERSAMPLING = 7, 3


@pytest.fixture(scope="module")
def scattered(ctx):
    """300 random points in [0, 1] x [0, 0.6], the operator placing its own grid (matern32, ell 0.2), and the numpy record of the double
    pass on its dense K: A = J^T J of EXACT rank k + p (J = (G diag(exp(-0.15 j))) G' as ``grid_factor_twin.dpc_problem``, q = k + p = 10
    rows), so that the k + p probes span the range of A, the Rayleigh-Ritz values are exact and no choice of probes -- in parameter or
    in noise coordinates -- changes an eigenvalue beyond rounding"""
    rng = np.random.default_rng(8)
    pts = rng.random((300, 2)) * np.array([1.0, 0.6])
    K = hf.InterpolatedKernelCovarianceOperator(pts, "matern32", 1.0, 0.2, ctx=ctx)
    Kd = K.to_dense()
    Kd = 0.5 * (Kd + Kd.T)
    N, k, q = 300, DPC_RANK, DPC_RANK + DPC_OVERSAMPLING
    rng = np.random.default_rng(0)
    G, G2 = rng.standard_normal((q, q)), rng.standard_normal((q, N))
    J = (G * np.exp(-0.15 * np.arange(q))[None, :]) @ G2
    A, Omega = J.T @ J, rng.standard_normal((N, q))
    R = np.linalg.inv(Kd)
    R = 0.5 * (R + R.T)

    class _Solve:
        def solve(self, y, x):
            y[...] = Kd @ x

    d_ref, U_ref = hl.double_pass_g(hl.DenseOperator(A), hl.DenseOperator(R), _Solve(), Omega, k)
    d, U, E = gf.double_pass_c(A, Kd, Omega, k)
    U = gf.fix_signs(U, U_ref)
    r = dict(K=Kd, A=A, Omega=Omega, R=R, d=d, dd=float(np.max(np.abs(d - d_ref) / np.abs(d_ref))), dU=float(np.abs(U - U_ref).max()),
             defect=float(np.abs(U.T @ R @ U - np.eye(k)).max()))
    return K, pts, r


def test_double_pass_c_against_the_devices_double_pass_g(ctx, scattered):
    """doublePassC(A, K) with K the interpolated operator against doublePassG(A, R, C) with R = inv(K.to_dense()) and C = K.to_dense()
    dense operators and the same Omega: d (relative), U (after fixing signs) and U^T R U - I each within 4 times the numpy
    restatement's own difference / defect plus 64 eps k; E^T U - I <= 1e-12.  doublePass on F^T A F (``ComposedOperator(F, A,
    F.transpose())``, probes in noise coordinates) gives the same eigenvalues to that tolerance."""
    K, pts, r = scattered
    k = DPC_RANK
    A = hf.npToDeviceOperator(r["A"], ctx=ctx)
    Omega = dev(r["Omega"], ctx)
    d, U, E = hf.doublePassC(A, K, Omega, k)
    dg, Ug = hf.doublePassG(A, hf.npToDeviceOperator(r["R"], ctx=ctx), hf.npToDeviceOperator(r["K"], ctx=ctx), Omega, k)
    Ug = Ug.to_dense()
    U, E = gf.fix_signs(U.to_dense(), Ug), gf.fix_signs(E.to_dense(), Ug)
    slack = 64.0 * EPS * k
    dd = np.max(np.abs(d - dg) / np.abs(dg))
    dU = np.abs(U - Ug).max()
    defect = np.abs(U.T @ r["R"] @ U - np.eye(k)).max()
    EtU = np.abs(E.T @ U - np.eye(k)).max()
    F = hf.InterpolatedKernelPrior(K).F
    Om2 = hf.MultiVector(F.shape[1], k + DPC_OVERSAMPLING, ctx=ctx)
    hf.parRandom.reseed(3)
    hf.parRandom.normal(1.0, Om2)
    dw, _ = hf.doublePass(hf.ComposedOperator(F, A, F.transpose()), Om2, k)
    dw_err = np.max(np.abs(np.asarray(dw) - d) / np.abs(d))
    print("device doublePassC on 300 scattered points: d %.3g (allowed %.3g), U %.3g (%.3g), U^T R U - I %.3g (%.3g), E^T U - I %.3g; "
          "whitened doublePass d %.3g (allowed %.3g); against numpy d %.3g"
          % (dd, 4 * r["dd"] + slack, dU, 4 * r["dU"] + slack, defect, 4 * r["defect"] + slack, EtU, dw_err, 4 * r["dd"] + slack,
             np.max(np.abs(d - r["d"]) / np.abs(r["d"]))))
    assert dd <= 4.0 * r["dd"] + slack
    assert dU <= 4.0 * r["dU"] + slack
    assert defect <= 4.0 * r["defect"] + slack
    assert EtU <= 1e-12
    assert dw_err <= 4.0 * r["dd"] + slack


class _PrecisionPrior:
    """The same Gaussian as an ``InterpolatedKernelPrior`` with the dense precision R = inv(K) and Rsolver on top and no ``C``: the prior
    the reference's default path (doublePassG(A, prior.R, prior.Rsolver)) takes.  Draws are the kernel prior's."""

    def __init__(self, kernel_prior, R):
        self._k = kernel_prior
        self.R = fp.MatrixOperator(R)
        self.Rsolver = kernel_prior.Rsolver
        self.mean = kernel_prior.mean

    def init_vector(self, x, dim):
        self._k.init_vector(x, dim)

    def sample(self, noise, m, add_mean=True):
        self._k.sample(noise, m, add_mean=add_mean)


def run_projector(prior, n, q, tmp, tag):
    obs = fp.ProtocolObservable(fp.NumpyProblem(n, hf.HostVector), fp.MatrixOperator(fp.observation_matrix(q, n)))
    hf.parRandom.reseed(11)
    hf.parRandom.split(0)
    params = hf.ActiveSubspaceParameterList()
    params['samples_per_process'], params['rank'], params['oversampling'] = 6, 7, 3
    params['serialized_sampling'], params['verbose'], params['save_and_plot'] = False, False, True
    out = os.path.join(str(tmp), tag) + "/"
    os.makedirs(out)
    params['output_directory'] = out
    AS = hf.ActiveSubspaceProjector(obs, prior, parameters=params)
    d, dec, enc = AS.construct_input_subspace(prior_preconditioned=True)
    return AS, d, dec.to_dense(), enc.to_dense(), sorted(f for f in os.listdir(out) if f.endswith(".npy"))


def test_active_subspace_projector_with_an_interpolated_kernel_prior(ctx, scattered, tmp_path):
    """The fake PDE of 300 unknowns -- the scattered points -- with 14 observations: the projector with an ``InterpolatedKernelPrior``
    (doublePassC, no R anywhere) against the same projector with the dense R = inv(K) and the same seeds; tolerances and file names as
    test_gpu_kernel_prior.py::test_active_subspace_projector_with_a_kernel_prior, from this K's numpy record."""
    K, pts, r = scattered
    k, N = 7, 300
    mean = 0.2 * np.cos(np.linspace(0.0, np.pi, N))
    kp = hf.InterpolatedKernelPrior(K, mean=mean)
    AS1, d1, dec1, enc1, files1 = run_projector(kp, N, 14, tmp_path, "kernel")
    AS2, d2, dec2, enc2, files2 = run_projector(_PrecisionPrior(hf.InterpolatedKernelPrior(K, mean=mean), r["R"]), N, 14, tmp_path, "precision")
    assert AS1.E_GN is not None and AS2.E_GN is None and AS1.prior_preconditioned and AS2.prior_preconditioned
    assert files1 == files2 and len(files1) >= 2
    dec1, enc1 = gf.fix_signs(dec1, dec2), gf.fix_signs(enc1, enc2)
    slack = 64.0 * EPS * k
    dd, dU, dE = np.max(np.abs(d1 - d2) / np.abs(d2)), np.abs(dec1 - dec2).max(), np.abs(enc1 - enc2).max()
    print("AS projector, interpolated kernel prior against dense R: d %.3g (allowed %.3g), decoder %.3g (%.3g), encoder %.3g (%.3g)"
          % (dd, 4 * r["dd"] + slack, dU, 4 * r["dU"] + slack, dE, 4 * r["dU"] + slack))
    assert d1.shape == (k,) and d1[-1] > 0
    assert dd <= 4.0 * r["dd"] + slack
    assert dU <= 4.0 * r["dU"] + slack
    assert dE <= 4.0 * r["dU"] + slack
    assert np.abs(enc1.T @ dec1 - np.eye(k)).max() <= 1e-12
    for f in files1:
        a, b = np.load(os.path.join(str(tmp_path), "kernel", f)), np.load(os.path.join(str(tmp_path), "precision", f))
        assert a.shape == b.shape


# ------------------------------------------------------------------------------------------------- 10. KLEProjector.extend
class _Prior:
    pass


def test_projector_extend_takes_the_interpolated_cross(ctx):
    """With an ``InterpolatedKernelCovarianceOperator`` as prior.C, ``KLEProjector.extend(points)`` is ``nystrom_extend(C.cross(points),
    encoder, d)`` bit for bit; at the projector's own points, with nugget 0 and no diagonal correction (K = W Cg W^T = cross at its own
    points), it reproduces the decoder to the eigensolve's accuracy: |extend - decoder|_ij <= ||R||_F / lambda_r + 8 N eps (|K| |encoder|)_ij
    / d_j with R = K encoder - decoder Lambda, as test_gpu_kernel_cross_cov.py::test_projector_extend_reproduces_its_decoder."""
    rng = np.random.default_rng(8)
    pts, tg = rng.random((300, 2)) * np.array([1.0, 0.6]), 0.1 + rng.random((70, 2)) * np.array([0.8, 0.4])
    N, r = 300, 10
    prior = _Prior()
    prior.M = scipy.sparse.identity(N, format="csr") * (0.6 / N)     # a lumped mass matrix of the box; 'identity' orthogonality does not use it
    prior.C = hf.InterpolatedKernelCovarianceOperator(pts, "sqexp", SIGMA, 0.25, nugget=0.0, diag_correction=False, ctx=ctx)
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = r, 30, False, False
    hf.parRandom.reseed(9)
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    with pytest.raises(ValueError):
        kle.extend(pts)                                            # no subspace yet
    d, dec, enc = kle.construct_input_subspace("identity")
    d, dec_h, enc_h = np.asarray(d), dec.to_dense(), enc.to_dense()
    ext = kle.extend(tg)
    ref = hf.nystrom_extend(prior.C.cross(tg), kle._kle_encoder, kle.d_KLE)
    assert (ext.size(), ext.nvec()) == (70, r) and np.array_equal(ext.to_dense(), ref.to_dense())
    Kd = prior.C.to_dense()
    resid = np.linalg.norm(Kd @ enc_h - dec_h * d)
    tol = resid / d[-1] + 8 * N * EPS * (np.abs(Kd) @ np.abs(enc_h)) / d
    err = np.abs(kle.extend(pts).to_dense() - dec_h)
    print("projector extend, interpolated: ||R||_F / lambda_r = %.3g, max err = %.3g, max err/tol = %.3g" % (resid / d[-1], err.max(), (err / tol).max()))
    assert np.all(err <= tol)
