"""The factor C = S S^T of a grid sampler's embedding (``GridFieldSampler.factor`` -> ``GridCovarianceFactor``, hfmi_op_grid_factor,
hfmi_fftcov.hip) on the device: S and S^T against the numpy twin (tests/helpers/grid_factor_twin.py) within a bound built from the
root spectrum, adjointness measured against the twin's own defect, S (S^T X) against the operator's apply, independence of chunking,
repeatability, the block storage contract of both operators through ``hfmi_op_apply``, and the lifetime of the shared state."""
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import grid_sampler_twin as gs                    # noqa: E402
import grid_factor_twin as tw                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = tw.EPS


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def sampler_at(op, growth):
    """a sampler on the embedding of growth ``growth`` whatever its spectrum (negative eigenvalues clipped)"""
    L.call("hfmi_tuning_set", b"fftcov_min_growth", growth)
    try:
        s = op.sampler(max_growth=growth, on_indefinite="clip")
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
    assert s.growth == growth
    return s


def make(ctx, case, growth):
    name, shape, spacing, subset, family, ell, nugget, _ = case
    nodes = tw.gpu_case_nodes(shape, subset)
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=tw.GPU_SIGMA, ell=ell, nugget=nugget, nodes=nodes, ctx=ctx)
    s = sampler_at(op, growth)
    root = tw.root_spectrum(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, growth)
    assert s.embedding == tuple(root.shape[::-1])
    return op, s, s.factor(), root, nodes


def dev(A, ctx):
    return hf.MultiVector.from_dense(np.ascontiguousarray(A), ctx=ctx)


CASE_GROWTHS = [(c, g) for c in tw.GPU_CASES for g in c[7]]
IDS = ["%s-g%d" % (c[0], g) for c, g in CASE_GROWTHS]


# ---------------------------------------------------------------------------------------------------------------- 1. the twin, adjointness
@pytest.mark.parametrize("case,growth", CASE_GROWTHS, ids=IDS)
def test_factor_and_transpose_against_the_twin(ctx, case, growth):
    """For 1, 2, 3 and 5 columns, each overwriting AND accumulating: |device - twin| per column <= 32 max(1, log2 P) eps ||root||_2 ||column||_2
    (``grid_factor_twin.column_bounds``), and <S Xi, X> = <Xi, S^T X> column by column with a defect, relative to |S Xi| |X|, of at most
    4 times the twin's own on the same inputs plus 64 eps (on the overwriting applies: an accumulated result minus what was there
    carries the rounding of that sum and difference, which is no property of the operator)."""
    op, s, S, root, nodes = make(ctx, case, growth)
    shape = case[1]
    N, Ptot = S.shape
    assert (N, Ptot) == (op.shape[0], root.size) and S.transpose().shape == (Ptot, N) and S.transpose().transpose() is S
    rng = np.random.default_rng(Ptot + growth)
    worst = worst_adj = 0.0
    for k in tw.GPU_NVECS:
        Xi, X = rng.standard_normal((Ptot, k)), rng.standard_normal((N, k))
        refS, refT = tw.apply_S(root, shape, Xi, nodes), tw.apply_St(root, shape, X, nodes)
        Xid, Xd = dev(Xi, ctx), dev(X, ctx)
        for accumulate in (False, True):
            Y0, Z0 = rng.standard_normal((N, k)), rng.standard_normal((Ptot, k))
            Y, Z = dev(Y0, ctx), dev(Z0, ctx)
            S.matMvMult(Xid, Y, accumulate=accumulate)
            S.matMvTranspmult(Xd, Z, accumulate=accumulate)
            Yd, Zd = Y.to_dense() - (Y0 if accumulate else 0.0), Z.to_dense() - (Z0 if accumulate else 0.0)
            assert np.all(np.isfinite(Yd)) and np.all(np.isfinite(Zd))
            # an accumulating apply rounds its sum once more: one ulp of what was there and what was added
            extra_S = 2.0 * EPS * (np.abs(Y0) + np.abs(refS)).max(axis=0) if accumulate else 0.0
            extra_T = 2.0 * EPS * (np.abs(Z0) + np.abs(refT)).max(axis=0) if accumulate else 0.0
            worst = max(worst, (np.abs(Yd - refS).max(axis=0) / (tw.column_bounds(root, Xi) + extra_S)).max(),
                        (np.abs(Zd - refT).max(axis=0) / (tw.column_bounds(root, X) + extra_T)).max())
            if not accumulate:
                scale = np.linalg.norm(refS, axis=0) * np.linalg.norm(X, axis=0)
                twin = np.abs(np.sum(refS * X, axis=0) - np.sum(Xi * refT, axis=0)) / scale
                mine = np.abs(np.sum(Yd * X, axis=0) - np.sum(Xi * Zd, axis=0)) / scale
                worst_adj = max(worst_adj, (mine / (4.0 * twin + 64.0 * EPS)).max())
    print("grid factor %s g=%d (P = %s): worst |device - twin| / bound = %.3g, worst adjointness defect / allowance = %.3g"
          % (case[0], growth, "x".join(map(str, s.embedding)), worst, worst_adj))
    assert worst <= 1.0
    assert worst_adj <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. S S^T X against C X
DEFINITE = [(c, g) for c, g in CASE_GROWTHS if tw.gpu_case_is_definite(c, g)]      # all but 4x3x3 and 9x8x7 at growth 0


@pytest.mark.parametrize("case,growth", DEFINITE, ids=["%s-g%d" % (c[0], g) for c, g in DEFINITE])
def test_factor_times_transpose_is_the_operators_apply(ctx, case, growth):
    """Definite embeddings: S (S^T X) against the operator's own FFT apply C X within the sum of both bounds -- the apply's FFT term
    (``fftcov_twin.column_bounds`` without the dense reference's part) and the composition's, bound_S(S^T X) + ||S||_2 bound_St(X)."""
    op, s, S, root, nodes = make(ctx, case, growth)
    name, shape, spacing, subset, family, ell, nugget, _ = case
    assert s.n_clipped == 0 and len(DEFINITE) == len(CASE_GROWTHS) - 2
    N, Ptot = S.shape
    X = np.random.default_rng(N).standard_normal((N, 3))
    Xd = dev(X, ctx)
    V, Y, CX = hf.MultiVector(Ptot, 3, ctx=ctx), hf.MultiVector(N, 3, ctx=ctx), hf.MultiVector(N, 3, ctx=ctx)
    S.transpose().matMvMult(Xd, V)
    S.matMvMult(V, Y)
    op.matMvMult(Xd, CX)
    v = tw.apply_St(root, shape, X, nodes)
    bound = (ft.column_bounds(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, X, np.zeros_like(X))
             + tw.column_bounds(root, v) + root.max() * tw.column_bounds(root, X))
    ratio = (np.abs(Y.to_dense() - CX.to_dense()).max(axis=0) / bound).max()
    print("S S^T X - C X %s g=%d: worst ratio to the sum of the bounds %.3g" % (name, growth, ratio))
    assert ratio <= 1.0 and np.abs(CX.to_dense()).max() > 0.1


def test_clipped_factor_misses_the_apply_by_the_reported_bound(ctx):
    """(4, 3, 3), matern12, max_growth = 0: the embedding is indefinite, S S^T = C + E with |E_ij| <= cov_error_bound, so
    |S S^T X - C X|_i <= cov_error_bound ||X_j||_1 (plus the rounding bounds of the definite case)."""
    case = [c for c in tw.GPU_CASES if c[0] == "4x3x3"][0]
    name, shape, spacing, subset, family, ell, nugget, _ = case
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=tw.GPU_SIGMA, ell=ell, nugget=nugget, ctx=ctx)
    with pytest.raises(hf.HfmiError):
        op.sampler(max_growth=0)
    s = op.sampler(max_growth=0, on_indefinite="clip")
    info = gs.info(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, max_growth=0, clip=True)
    assert s.growth == 0 and s.n_clipped == info["n_clipped"] > 0
    assert abs(s.cov_error_bound / info["cov_error_bound"] - 1.0) < 1e-12
    S = s.factor()
    N, Ptot = S.shape
    root = tw.root_spectrum(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, 0)
    X = np.random.default_rng(3).standard_normal((N, 4))
    Xd = dev(X, ctx)
    V, Y, CX = hf.MultiVector(Ptot, 4, ctx=ctx), hf.MultiVector(N, 4, ctx=ctx), hf.MultiVector(N, 4, ctx=ctx)
    S.transpose().matMvMult(Xd, V)
    S.matMvMult(V, Y)
    op.matMvMult(Xd, CX)
    diff = Y.to_dense() - CX.to_dense()
    rounding = (ft.column_bounds(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, X, np.zeros_like(X))
                + tw.column_bounds(root, tw.apply_St(root, shape, X, None)) + root.max() * tw.column_bounds(root, X))
    allowed = s.cov_error_bound * np.abs(X).sum(axis=0) + rounding
    # E is the restriction of a circulant with constant diagonal cov_error_bound: the twin's E X is what the difference must be
    Sd = tw.dense_S(root, shape)
    E = Sd @ Sd.T - op.to_dense()
    print("clipped 4x3x3: max |S S^T X - C X| %.3g, allowed %.3g, against the twin's E X %.3g" % (np.abs(diff).max(), allowed.min(), np.abs(diff - E @ X).max()))
    assert np.all(np.abs(diff).max(axis=0) <= allowed) and np.abs(diff).max() > 0.01 * s.cov_error_bound
    assert np.all(np.abs(diff - E @ X).max(axis=0) <= rounding + tw.twin_tolerance(Ptot, tw.GPU_SIGMA, nugget) * np.abs(X).sum(axis=0))


# ---------------------------------------------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("name,growth", [("33-subset", 2), ("17x12-subset", 1), ("9x8x7", 0)])
def test_chunking_and_repetition_change_no_bit(ctx, name, growth):
    """``fftcov_pairs`` = 1, 2 and the default give identical bits for both operators, two applies of the same block are identical, and
    making the factor changes no bit of the sampler's draws or of the operator's apply"""
    case = [c for c in tw.GPU_CASES if c[0] == name][0]
    nodes = tw.gpu_case_nodes(case[1], case[3])
    op = hf.GridKernelCovarianceOperator(case[1], case[2], family=case[4], sigma=tw.GPU_SIGMA, ell=case[5], nugget=case[6], nodes=nodes, ctx=ctx)
    s = sampler_at(op, growth)
    draws0 = s.sample(5, 17).to_dense()
    S = s.factor()
    N, Ptot = S.shape
    rng = np.random.default_rng(5)
    Xi, X = dev(rng.standard_normal((Ptot, 5)), ctx), dev(rng.standard_normal((N, 5)), ctx)
    Y, Z, CX = hf.MultiVector(N, 5, ctx=ctx), hf.MultiVector(Ptot, 5, ctx=ctx), hf.MultiVector(N, 5, ctx=ctx)
    op.matMvMult(X, CX)
    cx0 = CX.to_dense()

    def both():
        S.matMvMult(Xi, Y)
        S.transpose().matMvMult(X, Z)
        return Y.to_dense(), Z.to_dense()

    y0, z0 = both()
    y1, z1 = both()
    assert np.array_equal(y0, y1) and np.array_equal(z0, z1) and np.abs(y0).max() > 0.1 and np.abs(z0).max() > 0.01
    try:
        for pairs in (1, 2, 0):
            L.call("hfmi_tuning_set", b"fftcov_pairs", pairs)
            y, z = both()
            assert np.array_equal(y, y0) and np.array_equal(z, z0), pairs
    finally:
        L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    assert np.array_equal(s.sample(5, 17).to_dense(), draws0)
    op.matMvMult(X, CX)
    assert np.array_equal(CX.to_dense(), cx0)
    # single-vector route: mult / transpmult are column 0 of a one-column block
    x1, y1v = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    S.init_vector(x1, 1)
    S.init_vector(y1v, 0)
    assert (x1.size(), y1v.size()) == (Ptot, N)


# ---------------------------------------------------------------------------------------------------------------- 4. block contract
@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
@pytest.mark.parametrize("name,growth", [("33-subset", 0), ("6x5", 1), ("17x12-subset", 0), ("4x3x3", 1)])
def test_block_contract_of_both_operators(ctx, name, growth, layout):
    """Y a view inside a wider parent with guard columns, for S (length N) and for S^T (length prod P_c): padding rows stay +0.0,
    nothing outside Y's window changes (rows below the length of the OTHER columns included), an overwriting apply equals the apply
    into a plain block bit for bit and an accumulating one adds it; blocks of another length are refused."""
    case = [c for c in tw.GPU_CASES if c[0] == name][0]
    op, s, S, root, nodes = make(ctx, case, growth)
    N, Ptot = S.shape
    k, guard = 3, 2
    rng = np.random.default_rng(N)
    for fac, nin, nout in ((S, Ptot, N), (S.transpose(), N, Ptot)):
        Xin = dev(rng.standard_normal((nin, k)), ctx)
        plain = hf.MultiVector(nout, k, ctx=ctx)
        fac.matMvMult(Xin, plain)
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
            a.check(written=[y], what="hfmi_op_apply of %s accumulate=%d [%s]" % ("S^T" if fac.is_transpose else "S", accumulate, layout))
            assert np.array_equal(y.mv.to_dense(), before + D if accumulate else D), accumulate
        # wrong lengths: input, output, both swapped
        for bad_in, bad_out in ((nin + 1, nout), (nin, nout + 1), (nout, nin) if nin != nout else (nin + 2, nout)):
            with pytest.raises(hf.HfmiError):
                fac.matMvMult(hf.MultiVector(bad_in, k, ctx=ctx), hf.MultiVector(bad_out, k, ctx=ctx))


# ---------------------------------------------------------------------------------------------------------------- 5. lifetime, refusals
def test_the_factor_outlives_its_sampler_and_refusals(ctx):
    case = tw.GPU_CASES[3]
    op, s, S, root, nodes = make(ctx, case, 1)
    N, Ptot = S.shape
    Xi = dev(np.random.default_rng(0).standard_normal((Ptot, 2)), ctx)
    Y = hf.MultiVector(N, 2, ctx=ctx)
    S.matMvMult(Xi, Y)
    y0 = Y.to_dense()
    # the C objects: destroy the sampler first, the operator made from it still applies (shared state)
    import ctypes as C
    handle = C.c_void_p()
    L.call("hfmi_tuning_set", b"fftcov_min_growth", 1)
    try:
        L.call("hfmi_grid_sampler_create", op._op, 1, 1, C.byref(handle))
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
    fac = C.c_void_p()
    L.call("hfmi_op_grid_factor", handle, 0, C.byref(fac))
    L.call("hfmi_grid_sampler_destroy", handle)
    gc.collect()
    Y2 = hf.MultiVector(N, 2, ctx=ctx)
    L.call("hfmi_op_apply", fac, Xi.handle, Y2.handle, 0)
    L.call("hfmi_op_destroy", fac)
    assert s.growth == 1 and np.array_equal(Y2.to_dense(), y0)
    out = C.c_void_p()
    with pytest.raises(hf.HfmiError):
        L.call("hfmi_op_grid_factor", None, 0, C.byref(out))
    for transpose in (-1, 2):
        with pytest.raises(hf.HfmiError):
            L.call("hfmi_op_grid_factor", s.handle, transpose, C.byref(out))
    with pytest.raises(ValueError):
        hf.GridCovarianceFactor(op)
    # the Python operator keeps its sampler alive
    S2 = op.sampler(max_growth=3).factor()
    gc.collect()
    Y3 = hf.MultiVector(S2.shape[0], 2, ctx=ctx)
    S2.matMvMult(dev(np.ones((S2.shape[1], 2)), ctx), Y3)
    assert np.all(np.isfinite(Y3.to_dense()))
