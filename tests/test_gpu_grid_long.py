"""GPU suite of the long route of the grid kernel covariance (hfmi_op_kernel_cov_grid_long, hfmi_grid_sampler_create_long,
``GridKernelCovarianceOperator(..., long_axes=True)``): split-line passes (tests/helpers/fftcov_long_twin.py states the rules).

* the apply against the dense host covariance under the bound of test_apply_against_host, with splits forced by the tuning key
  "fftcov_max_line" at small sizes and with natural long lines;
* bit-identity with the old route where no axis is split: applies, draws and factors;
* the sampler on the grids that need more than the old route's embedding (65^2 and 129^2 BiLaplacian, 1-D 1025 Matern-5/2), its
  draws against the twin, its factor against the dense covariance, chunked calls, and ``GridKernelPrior`` on it;
* the refusals of every new entry point."""
import ctypes as C
import gc
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_long_twin as lt                     # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import grid_factor_twin as gf                     # noqa: E402
import grid_metric_twin as gm                     # noqa: E402
import grid_sampler_twin as gs                    # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SIGMA = 1.3
METRIC = np.array([[1.25, -0.75], [-0.75, 1.25]])


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


class max_line:
    """the tuning key "fftcov_max_line" for the operators created inside the block, 4096 again after it"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        L.call("hfmi_tuning_set", b"fftcov_max_line", self.v)

    def __exit__(self, *exc):
        L.call("hfmi_tuning_set", b"fftcov_max_line", lt.MAX_LINE)


class pairs_knob:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        L.call("hfmi_tuning_set", b"fftcov_pairs", self.v)

    def __exit__(self, *exc):
        L.call("hfmi_tuning_set", b"fftcov_pairs", 0)


def own_counts():
    live, acquired, pooled = (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int64(0)
    L.call("hfmi_test_own_counts", None, live, acquired, C.byref(pooled))
    return list(live)


def within_bound(what, Y, Y_ref, bound):
    ratio = np.linalg.norm(Y - Y_ref, axis=0) / np.maximum(bound, 1e-300)
    print("grid long %s: N=%d k=%d worst err/bound = %.3g" % (what, Y.shape[0], Y.shape[1], ratio.max()))
    assert np.all(np.isfinite(Y)) and ratio.max() <= 1.0, float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------- 1. apply against the host
# (id, shape, max_line, family, metric, nodes kind, nvec, accumulate, fftcov_pairs)
APPLY_CASES = [
    ("9-ml8", (9,), 8, "sqexp", None, "all", 3, False, 0),
    ("9-ml16-subset", (9,), 16, "matern12", None, "subset", 2, True, 0),
    ("13x5-ml8", (13, 5), 8, "matern32", None, "all", 5, True, 0),
    ("13x5-ml16-subset", (13, 5), 16, "matern52", None, "subset", 3, False, 1),
    ("19x5-ml8-subset", (19, 5), 8, "matern52", None, "subset", 1, False, 0),
    ("19x5-ml16", (19, 5), 16, "sqexp", None, "all", 4, False, 1),
    ("9x8x5-ml8", (9, 8, 5), 8, "matern32", None, "all", 3, False, 0),
    ("9x8x5-ml16-subset", (9, 8, 5), 16, "matern12", None, "subset", 5, True, 0),
    ("5x3x6-ml4", (5, 3, 6), 4, "matern32", None, "all", 3, False, 1),
    ("9x8-ml8-matern1-metric", (9, 8), 8, "matern1", METRIC, "all", 3, False, 0),
    ("9x8-ml8-matern1-metric-subset", (9, 8), 8, "matern1", METRIC, "subset", 2, True, 0),
    ("2049", (2049,), 4096, "matern32", None, "all", 3, False, 0),
    ("4097", (4097,), 4096, "matern52", None, "all", 2, True, 0),
    ("2049x3", (2049, 3), 4096, "matern12", None, "all", 3, False, 0),
    ("3x2049-subset", (3, 2049), 4096, "sqexp", None, "subset", 1, False, 0),
    ("65-ml16", (65,), 16, "matern32", None, "all", 3, False, 0),          # a strided sub-axis of 16 entries
]


@pytest.mark.parametrize("cid,shape,ml,family,G,kind,nvec,accumulate,pairs", APPLY_CASES, ids=[c[0] for c in APPLY_CASES])
def test_long_apply_against_host(ctx, cid, shape, ml, family, G, kind, nvec, accumulate, pairs):
    """Per column ||Y_j - Yref_j||_2 <= 32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W_j||_2 + 8 N eps || |C| |W_j| ||_2 (the bound of
    test_apply_against_host; an accumulating case is the sum of both applies' bounds).  Up to 4096 points Yref is the whole dense
    product; beyond, 514 seeded rows of it, and the whole columns are held to the numpy split twin within twice the FFT term."""
    spacing = ft.SPACINGS[:len(shape)]
    ell, nugget = 0.05, 0.1
    nodes = ft.nodes_of(shape, kind)
    assert lt.feasible(shape, 0, ml)
    with max_line(ml):
        op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=SIGMA, ell=ell, nugget=nugget, nodes=nodes, ctx=ctx,
                                             metric=G, long_axes=True)
    assert op.long_axes and any(L1 > 1 for L1, _ in lt.plan(lt.APPLY, shape, 0, ml)["split"])
    pts = ft.points(shape, spacing, nodes)
    N = pts.shape[0]
    rng = np.random.default_rng(2000 + N + nvec)
    rows = ft.reference_rows(N)
    sel = slice(None) if rows is None else rows
    Ws = [rng.standard_normal((N, nvec)) for _ in range(2 if accumulate else 1)]
    Yd = hf.MultiVector(N, nvec, ctx=ctx)
    ref, bound, twin, twin_bound = 0.0, 0.0, 0.0, 0.0
    with pairs_knob(pairs):
        for i, W in enumerate(Ws):
            op.matMvMult(hf.MultiVector.from_dense(W, ctx=ctx), Yd, accumulate=i > 0)
            Cm = hf.kernel_cov_host(pts, family, SIGMA, ell, nugget, rows=rows, metric=G)
            ref = ref + Cm @ W
            bound = bound + gm.column_bounds(shape, spacing, family, SIGMA, ell, nugget, W, np.abs(Cm) @ np.abs(W), G)
            if rows is not None:
                twin = twin + lt.apply(shape, spacing, family, SIGMA, ell, nugget, W, nodes, G, ml)
                twin_bound = twin_bound + 2.0 * gm.column_bounds(shape, spacing, family, SIGMA, ell, nugget, W, np.zeros((1, nvec)), G)
    Y = Yd.to_dense()
    within_bound(cid, Y[sel], ref, bound)
    if rows is not None:
        within_bound(cid + " (whole columns against the split twin)", Y, twin, twin_bound)


# ---------------------------------------------------------------------------------------------------------------- 2. bit-identity, no split
@pytest.mark.parametrize("shape,spacing,family,kind", [((5, 4), (0.2, 0.25), "matern32", "all"), ((13, 5), (0.1, 0.25), "matern12", "subset"),
                                                       ((4, 3, 3), (0.4, 0.3, 0.3), "matern52", "all")])
def test_no_split_is_bit_identical_to_the_old_route(ctx, shape, spacing, family, kind):
    """default max_line: nothing splits, so the long route runs the old route's passes: applies, draws (3 growths' worth of creation
    rule, clip allowed) and both factors give the same bits"""
    nodes = ft.nodes_of(shape, kind)
    old = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=SIGMA, ell=0.3, nugget=0.01, nodes=nodes, ctx=ctx)
    new = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=SIGMA, ell=0.3, nugget=0.01, nodes=nodes, ctx=ctx, long_axes=True)
    N = old.shape[0]
    W = hf.MultiVector.from_dense(np.random.default_rng(N).standard_normal((N, 5)), ctx=ctx)
    Ya, Yb = hf.MultiVector(N, 5, ctx=ctx), hf.MultiVector(N, 5, ctx=ctx)
    old.matMvMult(W, Ya)
    new.matMvMult(W, Yb)
    assert np.array_equal(Ya.to_dense(), Yb.to_dense()) and np.abs(Ya.to_dense()).max() > 0
    sa, sb = old.sampler(max_growth=3, on_indefinite="clip"), new.sampler(max_growth=3, on_indefinite="clip")
    assert (sa.growth, sa.embedding, sa.n_clipped) == (sb.growth, sb.embedding, sb.n_clipped)
    assert sa.lambda_min == sb.lambda_min and sa.lambda_max == sb.lambda_max
    assert np.array_equal(sa.sample(5, 17).to_dense(), sb.sample(5, 17).to_dense())
    Fa, Fb = sa.factor(), sb.factor()
    Ptot = Fa.shape[1]
    Xi = hf.MultiVector.from_dense(np.random.default_rng(Ptot).standard_normal((Ptot, 3)), ctx=ctx)
    Za, Zb = hf.MultiVector(N, 3, ctx=ctx), hf.MultiVector(N, 3, ctx=ctx)
    Fa.matMvMult(Xi, Za)
    Fb.matMvMult(Xi, Zb)
    assert np.array_equal(Za.to_dense(), Zb.to_dense())
    Ta, Tb = hf.MultiVector(Ptot, 5, ctx=ctx), hf.MultiVector(Ptot, 5, ctx=ctx)
    Fa.matMvTranspmult(W, Ta)
    Fb.matMvTranspmult(W, Tb)
    assert np.array_equal(Ta.to_dense(), Tb.to_dense())


# ---------------------------------------------------------------------------------------------------------------- 3. sampler and factor
def root_norm_bound(P, sigma, nugget, lambda_max):
    """||sqrt(max(Lambda, 0))||_2 from above without the spectrum: sum max(lambda, 0) = P (sigma^2 + nugget) + sum |lambda^-|, and a
    definite embedding has every lambda^- within the floor 16 eps log2(P) lambda_max"""
    return np.sqrt(P * (sigma ** 2 + nugget) + P * gs.floor(P, lambda_max))


def check_factor_rows(ctx, op, s, G, family, sigma, ell, nugget, k=4):
    """S (S^T e_i) against C e_i at k seeded nodes: per column within the composition bound of test_gpu_grid_factor.py,
    bound_S(S^T e_i) + ||root||_inf bound_St(e_i) with ||S^T e_i||_2 = sqrt(C_ii), plus the twin's tolerance; cov_error_bound = 0"""
    S = s.factor()
    N, Ptot = S.shape
    idx = np.sort(np.random.default_rng(N).choice(N, k, replace=False))
    X = np.zeros((N, k))
    X[idx, np.arange(k)] = 1.0
    V, Y = hf.MultiVector(Ptot, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    S.transpose().matMvMult(hf.MultiVector.from_dense(X, ctx=ctx), V)
    S.matMvMult(V, Y)
    ref = hf.kernel_cov_host(op.points, family, sigma, ell, nugget, rows=idx, metric=G).T
    rn = root_norm_bound(Ptot, sigma, nugget, s.lambda_max)
    per = 32.0 * max(1.0, np.log2(Ptot)) * EPS * rn
    bound = per * np.sqrt(sigma ** 2 + nugget) + np.sqrt(s.lambda_max) * per + gf.twin_tolerance(Ptot, sigma, nugget)
    err = np.abs(Y.to_dense() - ref).max(axis=0)
    print("grid long factor P=%s: worst |S S^T e_i - C e_i| / bound = %.3g" % ("x".join(map(str, s.embedding)), (err / bound).max()))
    assert s.cov_error_bound == 0.0 and np.all(err <= bound)


@pytest.mark.parametrize("n,growth,P", [(65, 4, 4096), (129, 4, 8192)])
def test_bilaplacian_grids_take_growth_4(ctx, n, growth, P):
    """the reference's prior (bilaplacian_kernel_2d(0.1, 0.1), unit square, spacing 1 / (n - 1)): growth 4, nothing clipped; the info
    is the twin's: lambda_min and lambda_max within 64 eps log2(P) lambda_max of numpy's transform of the twin's column, which
    tests/golden/grid_long_growth.json records (tests/test_fftcov_long_cpu.py::test_growth_table computes them and holds them to the
    record; half a minute of host time, so not here); S S^T = C on seeded rows of both, the 129^2 factor through split passes on
    both axes.  (The old route's growth 3 is indefinite on both: test_growth_table.)"""
    kw = hf.bilaplacian_kernel_2d(0.1, 0.1)
    op = hf.GridKernelCovarianceOperator((n, n), 1.0 / (n - 1), ctx=ctx, long_axes=True, **kw)
    s = op.sampler(max_growth=6)
    print("bilaplacian %d^2: growth %d P %s lambda_min %.17g lambda_max %.17g ratio %.3g" % (n, s.growth, s.embedding, s.lambda_min, s.lambda_max,
                                                                                           s.lambda_min / s.lambda_max))
    assert (s.growth, s.embedding, s.n_clipped, s.cov_error_bound) == (growth, (P, P), 0, 0.0)
    assert s.lambda_min >= -gs.floor(P * P, s.lambda_max)
    with open(os.path.join(ROOT, "tests", "golden", "grid_long_growth.json")) as f:
        twin = json.load(f)["bilaplacian_%dx%d" % (n, n)]
    assert (twin["growth"], twin["embedding"]) == (growth, [P, P])
    tol = 64.0 * EPS * np.log2(P * P) * twin["lambda_max"]
    assert abs(s.lambda_min - twin["lambda_min"]) <= tol and abs(s.lambda_max - twin["lambda_max"]) <= tol
    assert tol < 0.01 * twin["lambda_min"]            # the comparison resolves lambda_min
    check_factor_rows(ctx, op, s, kw["metric"], kw["family"], kw["sigma"], kw["ell"], 0.0, k=4 if n == 65 else 2)


def test_one_dimensional_matern52_takes_growth_3(ctx):
    """1025 nodes, spacing 1 / 1024, matern52, ell = 1: growth 3, P = 32768 (over the old route's 4096); info equals the twin's (the
    extremes within 64 eps log2(P) lambda_max of numpy's); chunked calls and the pairs per chunk change no bit; S S^T = C on seeded
    rows.  Its draws against the twin's: this spectrum has most eigenvalues within rounding of zero, where the square root turns a
    rounding difference of the two spectra into more than rounding (grid_factor_twin.py says the same of its cases), so the twin's
    parity bound, which assumes equal amplitudes, gets the term that pays for it:  with |lambda'_e - lambda_e| <= delta =
    64 eps log2(P) lambda_max (what the extremes are held to) and |sqrt(max(a, 0)) - sqrt(max(b, 0))| <= sqrt(|a - b|), a draw
    z_j = sum_e sqrt(max(lambda_e, 0) / P) xi_e w^(j e) moves by at most sqrt(delta / P) sum_e |xi_e|.  The parity of split draws
    without that term is test_split_draws_against_the_twin's, on spectra bounded away from zero."""
    shape, spacing, family = (1025,), (1.0 / 1024,), "matern52"
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=SIGMA, ell=1.0, ctx=ctx, long_axes=True)
    s = op.sampler(max_growth=6)
    g, P, ratio, definite = lt.sampler_growth(shape, spacing, family, SIGMA, 1.0, 0.0, max_growth=6)
    lam = gs.spectrum(shape, spacing, family, SIGMA, 1.0, 0.0, g)
    assert (s.growth, list(s.embedding), s.n_clipped) == (g, P, 0) == (3, [32768], 0) and definite
    tol = 64.0 * EPS * np.log2(lam.size) * lam.max()
    assert abs(s.lambda_min - lam.min()) <= tol and abs(s.lambda_max - lam.max()) <= tol
    D = s.sample(6, 99).to_dense()
    assert np.all(np.isfinite(D)) and np.abs(D).max() > 0
    ref = gs.draws(shape, spacing, family, SIGMA, 1.0, 0.0, g, 6, 99, lam=lam)
    xi_sum = max(np.abs(gs.noise(lam.size, pair, 99)).sum() for pair in range(3))
    bound = gs.parity_bound(lam.size, SIGMA, 0.0) + np.sqrt(tol / lam.size) * xi_sum
    err = np.abs(D - ref).max()
    print("1-D growth-3 draws: worst |device - twin| = %.3g, bound %.3g (parity alone %.3g)" % (err, bound, gs.parity_bound(lam.size, SIGMA, 0.0)))
    assert err <= bound
    parts = np.concatenate([s.sample(2, 99, first=0).to_dense(), s.sample(4, 99, first=2).to_dense()], axis=1)
    assert np.array_equal(parts, D)
    with pairs_knob(1):
        assert np.array_equal(s.sample(6, 99).to_dense(), D)
    check_factor_rows(ctx, op, s, None, family, SIGMA, 1.0, 0.0)


@pytest.mark.parametrize("shape,ml,growth,kind", [((9, 8), 8, 1, "all"), ((13, 5), 16, 2, "subset"), ((9,), 16, 2, "all"), ((5, 3, 6), 8, 1, "all"),
                                                  ((2049,), 4096, 0, "all"),
                                                  # the generated pass on sub-axes of 4 and 8 entries, contiguous and strided
                                                  ((3,), 4, 0, "all"), ((5,), 8, 0, "all"), ((3, 3), 4, 0, "all")])
def test_split_draws_against_the_twin(ctx, shape, ml, growth, kind):
    """forced splits (and one natural long line), the growth forced by "fftcov_min_growth": the generated pass on a split low sub-axis
    keeps storage entries 2 q, 2 q + 1 together, so the draws are the twin's (noise defined on storage entries) within its parity bound;
    chunks keep the bits; S S^T = C on seeded rows.  Matern-1/2: a spectrum bounded away from zero, where the square root keeps rounding at rounding level."""
    spacing, ell = ((0.2, 0.25, 0.3)[:len(shape)], 0.4) if shape != (2049,) else ((1.0 / 2048,), 0.005)
    nodes = ft.nodes_of(shape, kind)
    with max_line(ml):
        op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern12", sigma=SIGMA, ell=ell, nodes=nodes, ctx=ctx, long_axes=True)
    L.call("hfmi_tuning_set", b"fftcov_min_growth", growth)
    try:
        s = op.sampler(max_growth=growth, on_indefinite="clip")
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
    assert s.growth == growth and max(lt.plan(lt.DRAW, shape, growth, ml)["split"])[0] > 1
    lam = gs.spectrum(shape, spacing, "matern12", SIGMA, ell, 0.0, growth)
    D = s.sample(5, 7).to_dense()
    ref = gs.draws(shape, spacing, "matern12", SIGMA, ell, 0.0, growth, 5, 7, nodes=nodes, lam=lam)
    err = np.abs(D - ref).max()
    print("split draws %s ml=%d g=%d: worst |device - twin| = %.3g" % (shape, ml, growth, err))
    assert err <= gs.parity_bound(lam.size, SIGMA, 0.0)
    parts = np.concatenate([s.sample(2, 7, first=0).to_dense(), s.sample(3, 7, first=2).to_dense()], axis=1)
    assert np.array_equal(parts, D)
    check_factor_rows(ctx, op, s, None, "matern12", SIGMA, ell, 0.0, k=3)       # the factor's split passes


def test_prior_on_the_bilaplacian_grid(ctx):
    """GridKernelPrior(op, max_growth=4) on 65^2: unclipped; sample(noise, m) and sample_block are finite"""
    kw = hf.bilaplacian_kernel_2d(0.1, 0.1)
    op = hf.GridKernelCovarianceOperator((65, 65), 1.0 / 64, ctx=ctx, long_axes=True, **kw)
    prior = hf.GridKernelPrior(op, max_growth=4)
    assert prior.growth == 4 and prior.n_clipped == 0 and prior.cov_error_bound == 0.0
    noise, m = hf.HostVector(), hf.HostVector()
    prior.init_vector(noise, "noise")
    prior.init_vector(m, 0)
    assert noise.size() == 4096 * 4096 and m.size() == 65 * 65
    hf.parRandom.reseed(3)
    hf.parRandom.normal(1.0, noise)
    prior.sample(noise, m)
    v = m.get_local()
    blk = prior.sample_block(3)
    assert np.all(np.isfinite(v)) and np.abs(v).max() > 0 and blk.shape == (3, 65 * 65) and np.all(np.isfinite(blk))


def test_profiler_times_every_pass_at_level_3(ctx):
    """tuning key "prof_level" 3: a profiling region records each pass of an apply as a group of its own (kind fftcov_pass, m = L,
    k = 4 flags + part, N = index in the plan) with the bytes the pass moves; at the default level it records none"""
    shape, ml = (13, 5), 8
    with max_line(ml):
        op = hf.GridKernelCovarianceOperator(shape, (0.1, 0.25), ell=0.4, ctx=ctx, long_axes=True)
    p = lt.plan(lt.APPLY, shape, 0, ml, nvec=4)
    W = hf.MultiVector.from_dense(np.random.default_rng(1).standard_normal((65, 4)), ctx=ctx)
    Y = hf.MultiVector(65, 4, ctx=ctx)
    ctx.profile_begin()
    op.matMvMult(W, Y)
    assert [r for r in ctx.profile_end() if r["kernel"] == "fftcov_pass"] == []
    L.call("hfmi_tuning_set", b"prof_level", 3)
    try:
        ctx.profile_begin()
        op.matMvMult(W, Y)
        recs = ctx.profile_end()
    finally:
        L.call("hfmi_tuning_set", b"prof_level", 2)
    recs = sorted((r for r in recs if r["kernel"] == "fftcov_pass"), key=lambda r: r["N"])
    assert len(recs) == len(p["passes"]) == 7
    for i, (r, q) in enumerate(zip(recs, p["passes"])):
        pm = q["pm"] if q["part"] == lt.HI else 1           # nload, nstore count axis positions: a high sub-line holds every pm-th
        held = min(q["L"], -(-q["nload"] // pm)) + min(q["L"], -(-q["nstore"] // pm))
        moved = 2 * q["nlines"] * (16 * held + (8 * q["L"] if q["flags"] & 2 else 0))
        assert (r["N"], r["m"], r["k"], r["launches"]) == (i, q["L"], 4 * q["flags"] + q["part"], 1) and r["ms"] > 0 and r["bytes_per_launch"] == moved


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_create_nothing(ctx):
    lib = L.load()
    spec = L.KernelSpec(L.KERNEL_FAMILIES["matern32"], 1, 1.0, 0.3, 0.0)
    spec2 = L.KernelSpec(L.KERNEL_FAMILIES["matern32"], 2, 1.0, 0.3, 0.0)
    h = (C.c_double * 3)(0.1, 0.1, 0.1)
    ctx.synchronize()
    gc.collect()                       # what earlier tests left to the collector goes before the count
    before = own_counts()
    out = C.c_void_p()

    def create(d, n, s=spec, nodes=None, N=None):
        arr = (C.c_int64 * max(1, len(n)))(*n)
        N = int(np.prod(n)) if N is None else N
        return lib.hfmi_op_kernel_cov_grid_long(ctx.handle, d, arr, h, nodes, C.c_int64(N), C.byref(s) if s is not None else None, C.byref(out))

    cases = [("axis past 2^23", lambda: create(1, [(1 << 23) + 1])), ("empty axis", lambda: create(1, [0])), ("d = 4", lambda: create(4, [2, 2, 2, 2])),
             ("null spec", lambda: create(1, [9], None)), ("spec of another d", lambda: create(1, [9], spec2)),
             ("N past the nodes", lambda: create(1, [9], N=10))]
    for what, call in cases:
        assert call() == -1 and not out.value, what
        assert lib.hfmi_last_error().decode(), what
    with max_line(4):
        assert create(1, [9]) == -1 and not out.value                      # P = 32 > 4^2
    assert own_counts() == before
    with pytest.raises(ValueError):
        hf.GridKernelCovarianceOperator(((1 << 23) + 1,), 0.1, ctx=ctx, long_axes=True)
    with pytest.raises(ValueError):
        hf.GridKernelCovarianceOperator((2049,), 0.1, ctx=ctx)             # the old route keeps its limit
    old = hf.GridKernelCovarianceOperator((13, 5), (0.1, 0.25), ell=0.4, ctx=ctx)
    new = hf.GridKernelCovarianceOperator((13, 5), (0.1, 0.25), ell=0.4, ctx=ctx, long_axes=True)
    free = old.matrix_free()
    gc.collect()                       # what earlier tests left to the collector goes before the count
    before = own_counts()
    for what, args in (("old-route operator", (old._op, 3, 0)), ("not a grid operator", (free._op, 3, 0)), ("max_growth = 7", (new._op, 7, 0)),
                       ("max_growth = -1", (new._op, -1, 1)), ("null operator", (None, 3, 0))):
        assert lib.hfmi_grid_sampler_create_long(args[0], args[1], args[2], C.byref(out)) == -1 and not out.value, what
        assert lib.hfmi_last_error().decode(), what
    assert own_counts() == before
    with pytest.raises(hf.HfmiError):
        old.sampler(max_growth=4)                                          # the old route answers as ever
    assert lib.hfmi_grid_sampler_create_long(new._op, 6, 0, C.byref(out)) == 0 and out.value
    assert lib.hfmi_grid_sampler_destroy(out) == 0
    assert own_counts() == before
