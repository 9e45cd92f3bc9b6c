"""Exact Gaussian field draws on regular grids by circulant embedding (``GridKernelCovarianceOperator.sampler`` ->
``GridFieldSampler``, hfmi_grid_sampler_*, hfmi_fftcov.hip) on the device: parity with the numpy twin (tests/helpers/grid_sampler_twin.py)
at the same seed, independence of chunking, the block storage contract, the statistics of 8192 draws against the dense covariance,
the info record and the refusals, and the projection-error test fed from ``sample_block``."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import grid_sampler_twin as tw                    # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = tw.EPS


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def sampler_at(op, growth, seed=0):
    """a sampler on the embedding of growth ``growth`` whatever its spectrum (negative eigenvalues clipped)"""
    L.call("hfmi_tuning_set", b"fftcov_min_growth", growth)
    try:
        s = op.sampler(max_growth=growth, on_indefinite="clip", seed=seed)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
    assert s.growth == growth
    return s


def own_counts():
    live, acquired, pooled = (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int64(0)
    L.call("hfmi_test_own_counts", None, live, acquired, C.byref(pooled))
    return list(live)


# ---------------------------------------------------------------------------------------------------------------- 1. parity with the twin
@pytest.mark.parametrize("growth", tw.PARITY_GROWTHS)
@pytest.mark.parametrize("family", list(tw.PARITY_KERNELS))
@pytest.mark.parametrize("case", tw.PARITY_SHAPES, ids=["x".join(map(str, c[0])) for c in tw.PARITY_SHAPES])
def test_parity_with_the_twin(ctx, case, family, growth):
    """|device - twin| <= 64 eps log2(prod P_c) sqrt(sigma^2 + nugget) 8 for 1, 2 and 7 columns, at growth 0 and at a forced growth 2 (clipped
    where the embedding is indefinite: the twin clips the same way).  The noise is bit-defined; the transforms and the spectrum differ
    by rounding.  tests/test_grid_sampler_twin_cpu.py measures what the spectrum's rounding alone does to these cases (at most 0.052 of
    the bound) and what the fp64 twin's own transform does (1e-3 of it), and says why the two smoothest families carry a nugget."""
    shape, spacing, subset = case
    ell, nugget = tw.PARITY_KERNELS[family]
    nodes = ft.case_nodes(shape, subset, 3)
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=tw.PARITY_SIGMA, ell=ell, nugget=nugget, nodes=nodes, ctx=ctx)
    s = sampler_at(op, growth)
    assert s.embedding == tuple(tw.embedding(shape, growth))
    bound = tw.parity_bound(int(np.prod(s.embedding)), tw.PARITY_SIGMA, nugget)
    ref = tw.draws(shape, spacing, family, tw.PARITY_SIGMA, ell, nugget, growth, max(tw.PARITY_COLUMNS), 77, nodes=nodes)
    worst = 0.0
    for n in tw.PARITY_COLUMNS:
        X = s.sample(n, 77).to_dense()
        assert X.shape == (op.shape[0], n) and np.all(np.isfinite(X))
        worst = max(worst, np.abs(X - ref[:, :n]).max() / bound)
    print("grid sampler parity %s %s g=%d: worst |delta| / bound = %.3g (max |draw| %.3g)" % (shape, family, growth, worst, np.abs(ref).max()))
    assert worst <= 1.0 and np.abs(ref).max() > 0.5


# ---------------------------------------------------------------------------------------------------------------- 2. chunk independence
@pytest.mark.parametrize("case", [tw.PARITY_SHAPES[2], tw.PARITY_SHAPES[3], tw.PARITY_SHAPES[0]], ids=["19x5-subset", "7x6x5", "33"])
def test_draws_do_not_depend_on_the_chunking(ctx, case):
    shape, spacing, subset = case
    nodes = ft.case_nodes(shape, subset, 3)
    op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern32", sigma=1.0, ell=0.4, nodes=nodes, ctx=ctx)
    s = op.sampler(max_growth=3)
    a = s.sample(7, 5).to_dense()
    assert np.array_equal(a, s.sample(7, 5).to_dense()) and np.all(np.isfinite(a)) and np.abs(a).max() > 0.5
    assert not np.array_equal(a, s.sample(7, 6).to_dense())
    try:
        for pairs in (1, 2, 0):
            L.call("hfmi_tuning_set", b"fftcov_pairs", pairs)
            assert np.array_equal(a, s.sample(7, 5).to_dense()), pairs
            L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    whole = s.sample(8, 5).to_dense()
    assert np.array_equal(whole[:, :7], a)                                  # an odd count drops the last imaginary part, nothing else
    parts = np.hstack([s.sample(4, 5, first=0).to_dense(), s.sample(4, 5, first=4).to_dense()])
    assert np.array_equal(parts, whole)
    assert np.array_equal(op.sampler(max_growth=3).sample(8, 5).to_dense(), whole)      # another sampler of the same operator


# ---------------------------------------------------------------------------------------------------------------- 3. block contract
@pytest.mark.parametrize("shape", [(8, 8), (13, 5), (19, 5)])          # N = 64, 65, 95: N % 32 in {0, 1, 31}
@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
def test_block_contract(ctx, shape, layout):
    """Y a view inside a wider parent with guard columns: padding rows stay +0.0, nothing outside Y's window changes; an overwriting
    draw is the draw of a plain block bit for bit, an accumulating one adds it to what was there."""
    k, guard = 7, 2
    N = shape[0] * shape[1]
    op = hf.GridKernelCovarianceOperator(shape, (0.05, 0.08), family="matern52", sigma=1.1, ell=0.2, nugget=0.1, ctx=ctx)
    s = op.sampler(max_growth=3)
    if layout == "wrapped":
        a = ba.Arena.wrapped(ctx, N, k + 2 * guard, ld=ba.round_up(N, 32) + 32)
        y = a.window(guard, k)
    else:
        a = ba.Arena.in_parent(ctx, N, 2 * k + 2 * guard)
        a.window(guard, k)                                                  # a neighbour that is handed out and must not change
        y = a.window(guard + k, k)
    Y0 = np.random.default_rng(N).standard_normal((N, k))
    L.call("hfmi_block_upload", y.mv.handle, L.ptr(L.as_f64(Y0)), L.LAYOUT_DENSE)
    D = s.sample(k, 9, first=2).to_dense()
    for accumulate in (True, False, True):
        a.snapshot()
        before = y.mv.to_dense()
        s.sample(k, 9, first=2, out=y.mv, accumulate=accumulate)
        a.check(written=[y], what="hfmi_grid_sampler_draw accumulate=%d [%s]" % (accumulate, layout))
        assert np.array_equal(y.mv.to_dense(), before + D if accumulate else D), accumulate


# ---------------------------------------------------------------------------------------------------------------- 4. statistics
def test_statistics_against_the_dense_covariance(ctx):
    """13 x 5, matern12, ell 0.4, growth 0 (definite), 8192 draws at a fixed seed: every entry of the empirical covariance within
    6 sqrt((C_ii C_jj + C_ij^2) / S) of kernel_cov_host, the real and the imaginary parts uncorrelated to the same bound.  This is the
    check that does not share the twin's assumptions: a wrong square root, a wrong order of Lambda or a reused counter fail here."""
    shape, spacing, family, ell, growth = tw.TABLE[0]
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.0, ell=ell, ctx=ctx)
    s = op.sampler(max_growth=0)
    assert s.growth == growth == 0 and s.n_clipped == 0 and s.lambda_min > 0.0
    S = tw.STAT_DRAWS
    X = s.sample(S, tw.STAT_SEED).to_dense()
    Cm = op.to_dense()
    tol = tw.cov_tolerance(Cm, S)
    emp = X @ X.T / S
    cross = X[:, 0::2] @ X[:, 1::2].T / (S // 2)
    print("grid sampler statistics: worst |emp - C| / tol = %.3f, worst |Re Im^T| / tol = %.3f, mean %.2e" % (
        np.abs((emp - Cm) / tol).max(), np.abs(cross / tol).max(), np.abs(X.mean(axis=1)).max()))
    assert np.all(np.abs(emp - Cm) <= tol)
    assert np.all(np.abs(cross) <= tol)
    assert np.abs(X.mean(axis=1)).max() <= 6.0 * np.sqrt(np.diag(Cm).max() / S)


# ---------------------------------------------------------------------------------------------------------------- 5. info and errors
@pytest.mark.parametrize("shape,spacing,family,ell,growth", tw.TABLE, ids=["%s-%s-%g" % ("x".join(map(str, r[0])), r[2], r[3]) for r in tw.TABLE])
def test_growth_and_sign_pattern_of_the_table(ctx, shape, spacing, family, ell, growth):
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.0, ell=ell, ctx=ctx)
    s = op.sampler(max_growth=3)
    rec = tw.info(shape, spacing, family, 1.0, ell, 0.0, max_growth=3)
    assert s.growth == growth == rec["growth"] and s.embedding == tuple(rec["embedding"])
    assert s.n_clipped == 0 and s.cov_error_bound == 0.0
    assert abs(s.lambda_max - rec["lambda_max"]) <= 64 * EPS * np.log2(np.prod(s.embedding)) * rec["lambda_max"]
    for g in range(4):
        sg = sampler_at(op, g)
        lam = tw.spectrum(shape, spacing, family, 1.0, ell, 0.0, g)
        ratio, floor = sg.lambda_min / sg.lambda_max, tw.floor(lam.size, 1.0)
        print("grid sampler %s %s ell=%g g=%d: lambda_min / lambda_max = %.3e (numpy %.3e), clipped %d" % (
            shape, family, ell, g, ratio, lam.min() / lam.max(), sg.n_clipped))
        if g < growth:
            assert ratio < -floor and sg.n_clipped > 0 and sg.cov_error_bound > 0.0
            assert abs(ratio - lam.min() / lam.max()) <= 1e-6 * abs(ratio)
        else:
            assert ratio >= -floor and sg.n_clipped == 0 and sg.cov_error_bound == 0.0


def test_indefinite_embeddings_raise_or_clip(ctx):
    shape, spacing, family, ell = (8, 8), (0.125, 0.125), "matern52", 1.0
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.0, ell=ell, ctx=ctx)
    rec = tw.info(shape, spacing, family, 1.0, ell, 0.0, max_growth=1, clip=True)
    before = own_counts()
    with pytest.raises(hf.HfmiError) as e:
        op.sampler(max_growth=1, on_indefinite="raise")
    assert own_counts() == before                                           # a refused create frees all it took
    assert e.value.code == -1
    m = re.search(r"lambda_min / lambda_max = (-[0-9.]+e[-+][0-9]+)", str(e.value))
    assert m, str(e.value)
    assert abs(float(m.group(1)) - rec["ratios"][1]) <= 2e-3 * abs(rec["ratios"][1]) and "growth 1" in str(e.value)
    s = op.sampler(max_growth=1, on_indefinite="clip")
    assert s.growth == 1 and s.n_clipped > 0 and s.embedding == (32, 32)
    assert abs(s.cov_error_bound - rec["cov_error_bound"]) <= 1e-10 * rec["cov_error_bound"]
    assert np.all(np.isfinite(s.sample(3, 1).to_dense()))
    # the second clipped case of the twin's check
    op2 = hf.GridKernelCovarianceOperator((13, 5), (0.1, 0.25), family="sqexp", sigma=1.0, ell=1.0, ctx=ctx)
    rec2 = tw.info((13, 5), (0.1, 0.25), "sqexp", 1.0, 1.0, 0.0, max_growth=0, clip=True)
    s2 = op2.sampler(max_growth=0, on_indefinite="clip")
    assert s2.n_clipped > 0 and abs(s2.cov_error_bound - rec2["cov_error_bound"]) <= 1e-10 * rec2["cov_error_bound"]


def test_refusals_create_and_write_nothing(ctx):
    lib = L.load()
    grid = hf.GridKernelCovarianceOperator((13, 5), (0.1, 0.25), family="matern12", sigma=1.0, ell=0.4, ctx=ctx)
    free = grid.matrix_free()
    Y0 = np.random.default_rng(2).standard_normal((65, 4))
    Y = hf.MultiVector.from_dense(Y0, ctx=ctx)
    short = hf.MultiVector.from_dense(Y0[:64], ctx=ctx)
    assert np.array_equal(Y.to_dense(), Y0)                                 # and whatever staging a download takes exists from here on
    ctx.synchronize()
    before = own_counts()
    out = C.c_void_p()
    for what, args in (("not a grid operator", (free._op, 3, 0)), ("max_growth = 4", (grid._op, 4, 0)), ("max_growth = -1", (grid._op, -1, 1)),
                       ("null operator", (None, 3, 0))):
        assert lib.hfmi_grid_sampler_create(args[0], args[1], args[2], C.byref(out)) == -1 and not out.value, what
        assert lib.hfmi_last_error().decode(), what
    assert own_counts() == before
    with pytest.raises(ValueError):
        hf.GridFieldSampler(free)
    with pytest.raises(ValueError):
        grid.sampler(on_indefinite="ignore")
    assert lib.hfmi_grid_sampler_create(grid._op, 3, 0, C.byref(out)) == 0 and out.value
    for what, rc in (("odd first", lib.hfmi_grid_sampler_draw(out, Y.handle, C.c_uint64(1), 3, 0)),
                     ("negative first", lib.hfmi_grid_sampler_draw(out, Y.handle, C.c_uint64(1), -2, 0)),
                     ("past the stream", lib.hfmi_grid_sampler_draw(out, Y.handle, C.c_uint64(1), 1 << 33, 0)),
                     ("another length", lib.hfmi_grid_sampler_draw(out, short.handle, C.c_uint64(1), 0, 0)),
                     ("null block", lib.hfmi_grid_sampler_draw(out, None, C.c_uint64(1), 0, 0))):
        assert rc == -1 and lib.hfmi_last_error().decode(), what
    assert np.array_equal(Y.to_dense(), Y0) and np.array_equal(short.to_dense(), Y0[:64])
    assert lib.hfmi_grid_sampler_draw(out, Y.handle, C.c_uint64(1), 2, 0) == 0
    assert not np.array_equal(Y.to_dense(), Y0)
    assert lib.hfmi_grid_sampler_destroy(out) == 0
    assert own_counts() == before                                           # what the sampler took is back
    assert lib.hfmi_grid_sampler_info(None, None, None, None, None, None, None) == -1


def test_the_sampler_outlives_its_operator(ctx):
    op = hf.GridKernelCovarianceOperator((13, 5), (0.1, 0.25), family="matern32", sigma=1.0, ell=0.4, nodes=ft.case_nodes((13, 5), True, 3), ctx=ctx)
    s = op.sampler()
    a = s.sample(4, 3).to_dense()
    del op
    assert np.array_equal(s.sample(4, 3).to_dense(), a)


# ---------------------------------------------------------------------------------------------------------------- 6. consumer
class _Prior:
    pass


def test_projection_error_test_runs_on_sample_block(ctx):
    """KLEProjector's projection-error test with the draws of ``sample_block``: the sampler passes for the prior in
    ``_prior_sample_block``.  The mean relative error is non-increasing in the rank and below 1.5 sqrt(sum_{i > r} d_i / sum d_i) at
    r = 20 (d: eigh of the dense C); the twin's draws give 0.412 against sqrt(.) = 0.395 (tests/test_grid_sampler_twin_cpu.py)."""
    shape, spacing, family, ell, _ = tw.TABLE[0]
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.0, ell=ell, ctx=ctx)
    N = op.shape[0]
    s = op.sampler(max_growth=0, seed=tw.KLE_SEED)
    prior = _Prior()
    prior.M, prior.C, prior.sample_block = sp.identity(N, format="csr"), op, s.sample_block
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = 20, 10, False, False
    params["error_test_samples"] = tw.KLE_DRAWS
    hf.parRandom.reseed(7)
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    kle.construct_input_subspace("mass")
    avg, std = kle.test_errors(ranks=list(tw.KLE_RANKS))
    d = np.linalg.eigvalsh(op.to_dense())[::-1]
    expect = np.sqrt(d[20:].sum() / d.sum())
    print("grid sampler consumer: projection errors %s, sqrt(tail / trace) at 20 = %.4f" % (np.round(avg, 4), expect))
    assert len(avg) == len(tw.KLE_RANKS) and np.all(np.isfinite(avg)) and np.all(np.isfinite(std))
    assert all(b <= a for a, b in zip(avg, avg[1:]))
    assert avg[-1] <= 1.5 * expect
    assert s._next == tw.KLE_DRAWS
    block = s.sample_block(3)                                               # the counter moves on, by an even number
    assert block.shape == (3, N) and s._next == tw.KLE_DRAWS + 4
    assert np.array_equal(block.T, s.sample(3, tw.KLE_SEED, first=tw.KLE_DRAWS).to_dense())
