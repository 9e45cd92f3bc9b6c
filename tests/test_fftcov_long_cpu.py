"""The long route of the grid kernel covariance without a device: ``hfmi_fftcov_long_plan_predict`` against the Python statement of
the split-line rules (tests/helpers/fftcov_long_twin.py) word for word, and against the old planners where no axis is split; the line
map of every split pass enumerated; the refusals; the numpy split transform against ``numpy.fft.fftn``; its apply against the dense
host covariance under the bound of test_apply_against_host; the growth the long-route sampler takes on the grids that need it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_long_twin as lt                     # noqa: E402
import fftcov_plan_twin as pt                     # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import grid_metric_twin as gm                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

# the shapes of tests/test_fftcov_plan_cpu.py
AXIS = list(range(1, 71)) + [127, 128, 129, 1024, 1025, 2048]
CORNERS = [1, 2, 3, 5, 16, 17, 33, 64, 70, 127, 128, 129, 1024, 1025, 2048]
BUDGETS = [0, 1, 1 << 20, 1 << 28, 1 << 34]
FORCED = [(9,), (9, 8), (9, 8, 5)]
NATURAL = [(2049,), (4097,), (1025,), (2049, 3), (3, 2049), (2, 3, 2049)]


def old_shapes():
    out = [(n,) for n in AXIS]
    out += [(a, b) for a in AXIS for b in AXIS]
    out += [(a, b, c) for a in CORNERS for b in CORNERS for c in CORNERS]
    for n in AXIS:
        out += [(n, 3, 5), (3, n, 5), (3, 5, n)]
    return out


def old_predict(kind, shape, growth, nvec, budget):
    import ctypes as C
    words = (C.c_int64 * pt.PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    if kind == lt.APPLY:
        L.call("hfmi_fftcov_plan_predict", len(shape), C.cast(n, C.c_void_p), int(nvec), int(budget), words)
    elif kind == lt.DRAW:
        L.call("hfmi_fftcov_sample_plan_predict", len(shape), C.cast(n, C.c_void_p), int(growth), int(nvec), int(budget), words)
    else:
        L.call("hfmi_fftcov_factor_plan_predict", len(shape), C.cast(n, C.c_void_p), int(growth), int(kind == lt.FACTOR_T), int(nvec),
               int(budget), words)
    return list(words)


def check_long(kind, shape, growth, max_line, nvec, budget):
    """the library's words equal the twin's, and the plan keeps the kernel's limits"""
    w = lt.predict(L, kind, shape, growth, max_line, nvec, budget)
    p = lt.plan(kind, shape, growth, max_line, nvec, budget)
    assert w == lt.plan_words(p), (kind, shape, growth, max_line)
    nsplit = sum(L1 > 1 for L1, _ in p["split"])
    assert len(p["passes"]) == ((2 * (len(shape) + nsplit) - 1) if kind in (lt.APPLY, lt.FACTOR, lt.FACTOR_T) else len(shape) + nsplit)
    assert len(p["passes"]) <= lt.MAX_PASSES
    for q in p["passes"]:
        assert q["L"] <= max_line
        assert q["lds_total"] <= pt.LDS_BYTES and q["lpw"] <= pt.MAX_LINES and 64 <= q["threads"] <= 512, (shape, q)
        assert (q["grid_x"] - 1) * q["lpw"] < q["nlines"] <= q["grid_x"] * q["lpw"]
    return p


def test_long_plan_is_the_old_plan_where_nothing_splits():
    """every shape of the old plan tests: the long apply's words are the twin's, and its head (words 0-11) and passes (16 words each)
    are the old planner's; the draw and the factors likewise at growth 0..3 on a subset"""
    count = 0
    for i, shape in enumerate(old_shapes()):
        nvec, budget = (1, 2, 5, 17, 74, 290)[i % 6], BUDGETS[i % len(BUDGETS)]
        kinds = [lt.APPLY] + ([lt.DRAW, lt.FACTOR, lt.FACTOR_T] if i % 7 == 0 else [])
        for kind in kinds:
            for growth in ([0] if kind == lt.APPLY else [0, 1, 2, 3]):
                _, P = lt.embedding(shape, growth)
                if max(P) > 4096:
                    continue
                p = check_long(kind, shape, growth, lt.MAX_LINE, nvec, budget)
                assert all(q["part"] == lt.WHOLE for q in p["passes"])
                w, o = lt.plan_words(p), old_predict(kind, shape, growth, nvec, budget)
                assert w[:12] == o[:12], shape
                for j in range(len(p["passes"])):
                    a, b = lt.HEAD_WORDS + j * lt.PASS_WORDS, pt.HEAD_WORDS + j * pt.PASS_WORDS
                    assert w[a:a + pt.PASS_WORDS] == o[b:b + pt.PASS_WORDS], (kind, shape, growth, j)
                count += 1
    assert count > 10000


@pytest.mark.parametrize("shape", NATURAL)
def test_natural_long_lines(shape):
    growths = [0, 1, 2, 3]
    for kind in (lt.APPLY, lt.DRAW, lt.FACTOR, lt.FACTOR_T):
        for growth in ([0] if kind == lt.APPLY else growths):
            p = check_long(kind, shape, growth, lt.MAX_LINE, 5, 0)
            if max(p["P"]) > lt.MAX_LINE:
                assert any(q["part"] != lt.WHOLE for q in p["passes"])


@pytest.mark.parametrize("max_line", [4, 8, 16, 64])
@pytest.mark.parametrize("shape", FORCED)
def test_forced_splits(shape, max_line):
    """sub-lines of 2, 4, 8, 16 (odd and even log2); shapes whose embedding passes max_line^2 are refused as the twin says"""
    seen = 0
    for kind in (lt.APPLY, lt.DRAW, lt.FACTOR, lt.FACTOR_T):
        for growth in ([0] if kind == lt.APPLY else [0, 1, 2]):
            if lt.feasible(shape, growth, max_line):
                check_long(kind, shape, growth, max_line, 3, 0)
                seen += 1
            else:
                with pytest.raises(hf.HfmiError):
                    lt.predict(L, kind, shape, growth, max_line, 3, 0)
    assert seen > 0 or max_line == 4        # (9, ...) has P_0 = 32 > 4^2: test_forced_splits_at_max_line_4 has feasible shapes


@pytest.mark.parametrize("shape", [(5, 3, 6), (3, 4, 6), (5,), (8, 2), (2, 5, 1)])
def test_forced_splits_at_max_line_4(shape):
    """max_line = 4 on shapes it can serve (P_c <= 16: sub-lines of 2 and 4), every kind, word for word"""
    for kind in (lt.APPLY, lt.DRAW, lt.FACTOR, lt.FACTOR_T):
        for growth in ([0] if kind == lt.APPLY else [0, 1, 2]):
            if lt.feasible(shape, growth, 4):
                p = check_long(kind, shape, growth, 4, 3, 0)
                if growth == 0 and max(p["P"]) > 4:
                    assert any(q["part"] != lt.WHOLE for q in p["passes"])
            else:
                with pytest.raises(hf.HfmiError):
                    lt.predict(L, kind, shape, growth, 4, 3, 0)
    assert lt.feasible(shape, 0, 4)


def test_refusals():
    ok = dict(kind=lt.APPLY, shape=(9, 8), growth=0, max_line=8, nvec=2, budget=0)
    lt.predict(L, **ok)
    bad = [dict(shape=((1 << 23) + 1,)), dict(shape=(9,), max_line=4), dict(shape=(3, 4097), max_line=64), dict(kind=lt.DRAW, growth=7),
           dict(kind=lt.APPLY, growth=1), dict(max_line=12), dict(max_line=2), dict(max_line=8192), dict(max_line=0), dict(kind=4),
           dict(kind=-1), dict(shape=(0, 3)), dict(shape=()), dict(shape=(1, 2, 3, 4)), dict(nvec=-1)]
    for change in bad:
        with pytest.raises(hf.HfmiError):
            lt.predict(L, **dict(ok, **change))
    assert lt.feasible(((1 << 23),), 0, 4096) and not lt.feasible(((1 << 23),), 1, 4096)
    assert lt.feasible(((1 << 17),), 6, 4096) and not lt.feasible(((1 << 17) + 1,), 6, 4096)
    # the tuning key: a power of two in 4 .. 4096
    for v in (3, 2, 8192, 0, -4, 12):
        with pytest.raises(hf.HfmiError):
            L.call("hfmi_tuning_set", b"fftcov_max_line", v)
    for v in (4, 4096):
        L.call("hfmi_tuning_set", b"fftcov_max_line", v)
    # the Python rules that need no device
    from hippyflow_amd.operators import _check_grid
    with pytest.raises(ValueError):
        _check_grid((2049,), 0.1, None, None, "matern32", 0.1, 0.0)
    _check_grid((2049,), 0.1, None, None, "matern32", 0.1, 0.0, L.GRID_COV_LONG_MAX_NODES)
    with pytest.raises(ValueError):
        _check_grid(((1 << 23) + 1,), 0.1, None, None, "matern32", 0.1, 0.0, L.GRID_COV_LONG_MAX_NODES)


@pytest.mark.parametrize("shape,max_line", [((9,), 8), ((9,), 16), ((9, 8), 8), ((9, 8, 5), 8), ((9, 8, 5), 16), ((13, 5), 8),
                                            ((19, 5), 8), ((2049,), 4096), ((3, 2049), 4096), ((5, 3, 6), 4), ((3, 4, 6), 4)])
def test_every_entry_of_a_pass_is_taken_once(shape, max_line):
    """each pass of the apply, the draw (growth 1) and the spectrum: the (line, position) pairs of the line map address distinct entries
    inside the padded array, exactly the entries the pass must take (all positions of the axes below, the data positions of the axes
    above, and along the axis itself every position -- on a high pass, of the low sub-lines n2 < esub); and 'p pm + sub sm' is the axis
    position of the entry (its low coordinate on a low pass)"""
    for kind in (lt.APPLY, lt.DRAW, lt.SPECTRUM):
        growth = 0 if kind == lt.APPLY else 1
        if not lt.feasible(shape, growth, max_line):
            continue
        p = lt.plan(kind, shape, growth, max_line)
        P, n = p["P"], p["n"]
        for q in p["passes"]:
            base, pos = lt.line_entries(q)
            ent = base[:, None] + np.arange(q["L"])[None, :] * q["stride"]
            assert ent.min() >= 0 and ent.max() < p["Ptot"]
            a = q["axis"]
            S = int(np.prod(P[:a]))
            coord = (ent // S) % P[a]
            if q["part"] == lt.LO:
                assert np.array_equal(coord % q["L2"], pos)
            else:
                assert np.array_equal(coord, pos)
            rng = []
            for b in range(3):
                if b < a:
                    rng.append(np.arange(P[b]))
                elif b > a:
                    rng.append(np.arange(P[b] if kind == lt.SPECTRUM else n[b]))
                else:
                    s_ = np.arange(P[a])
                    rng.append(s_[s_ % q["L2"] < q["esub"]] if q["part"] == lt.HI else s_)
            i0, i1, i2 = np.meshgrid(*rng, indexing="ij")
            want = np.sort((i0 + P[0] * (i1 + P[1] * i2)).ravel())
            assert np.array_equal(np.sort(ent.ravel()), want), (kind, shape, a, q["part"])
    for kind in (lt.FACTOR, lt.FACTOR_T):        # the factor's passes: distinct entries inside the padded array
        if lt.feasible(shape, 1, max_line):
            p = lt.plan(kind, shape, 1, max_line)
            for q in p["passes"]:
                base, pos = lt.line_entries(q)
                ent = base[:, None] + np.arange(q["L"])[None, :] * q["stride"]
                assert ent.min() >= 0 and ent.max() < p["Ptot"] and np.unique(ent).size == ent.size


# ---------------------------------------------------------------------------------------------------------------- the split transform
@pytest.mark.parametrize("shape,split", [((32,), [(4, 8)]), ((32,), [(8, 4)]), ((32,), [(2, 16)]), ((64,), [(8, 8)]), ((8, 16), [(2, 4), (4, 4)]),
                                         ((8, 4, 32), [(1, 8), (2, 2), (4, 8)]), ((4096 * 2,), [(2, 4096)])])
def test_split_transform_is_fftn_in_storage_order(shape, split):
    rng = np.random.default_rng(len(shape) + shape[0])
    P = list(shape)
    x = rng.standard_normal(P[::-1]) + 1j * rng.standard_normal(P[::-1])
    got = lt.storage_fftn(x, split)
    ref = np.fft.fftn(x)[lt.storage_permutation(P)]
    assert np.abs(got - ref).max() <= 64 * lt.EPS * np.log2(x.size) * np.abs(ref).max()
    back = lt.storage_ifftn(got, split) / x.size
    assert np.abs(back - x).max() <= 64 * lt.EPS * np.log2(x.size) * np.abs(x).max()


APPLY_CASES = [((9,), 8, "sqexp", None, 3), ((9,), 16, "matern12", None, 2), ((13, 5), 8, "matern32", None, 5), ((19, 5), 8, "matern52", None, 1),
               ((9, 8, 5), 8, "matern32", None, 3), ((9, 8, 5), 16, "sqexp", None, 4), ((9, 8), 8, "matern1", np.array([[1.25, -0.75], [-0.75, 1.25]]), 3)]


@pytest.mark.parametrize("shape,max_line,family,G,nvec", APPLY_CASES)
def test_twin_apply_meets_the_bound(shape, max_line, family, G, nvec):
    """the numpy split apply against the dense host covariance under 32 max(1, log2 P) eps sqrt(P) ||c|| ||W_j|| + 8 N eps || |C| |W_j| ||,
    with and without a node map; no extra twiddle term (tests/helpers/fftcov_long_twin.py says why)"""
    spacing = ft.SPACINGS[:len(shape)]
    sigma, ell, nugget = 1.3, 0.05, 0.1
    for kind in ("all", "subset"):
        nodes = ft.nodes_of(shape, kind)
        pts = ft.points(shape, spacing, nodes)
        W = np.random.default_rng(7 + pts.shape[0]).standard_normal((pts.shape[0], nvec))
        Y = lt.apply(shape, spacing, family, sigma, ell, nugget, W, nodes, G, max_line)
        Cm = hf.kernel_cov_host(pts, family, sigma, ell, nugget, metric=G)
        bound = gm.column_bounds(shape, spacing, family, sigma, ell, nugget, W, np.abs(Cm) @ np.abs(W), G)
        ratio = np.linalg.norm(Y - Cm @ W, axis=0) / bound
        print("long twin %s %s max_line=%d: worst err/bound = %.3g" % (shape, kind, max_line, ratio.max()))
        assert ratio.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the sampler's growth
def test_first_column_is_the_metric_twins():
    """the one-evaluation column of the long twin has the bits of grid_metric_twin.first_column: with and without a metric, every
    family of the table, 1 to 3 dimensions, an axis of one node, grown embeddings"""
    cases = [((65, 65), (1 / 64, 1 / 64), "matern1", hf.bilaplacian_kernel_2d(0.1, 0.1)["metric"], 1), ((6, 5), (0.2, 0.25), "matern32", gm.rotated_metric(), 0),
             ((4, 3, 3), (0.2, 0.25, 0.3), "matern52", gm.FULL_3D, 1), ((9, 1), (0.1, 0.3), "sqexp", None, 2), ((1025,), (1 / 1024,), "matern52", None, 3),
             ((1, 7), (0.1, 0.3), "matern1", np.array([[1.25, -0.75], [-0.75, 1.25]]), 0)]
    for shape, spacing, family, G, growth in cases:
        want = gm.first_column(shape, spacing, family, 1.3, 0.3, 0.1, G, growth)
        got = lt.first_column(shape, spacing, family, 1.3, 0.3, 0.1, G, growth)
        assert got.shape == want.shape and np.array_equal(got, want), (shape, family)


def old_route_could(shape, g):
    return g <= 3 and max(lt.embedding(shape, g)[1]) <= 4096


def test_growth_table():
    """the growth a long-route sampler takes (floor 16 eps log2(P) lambda_max), every growth below it indefinite, and what the old
    route could do on the same grid (growth <= 3, every P_c <= 4096):
    65 x 65 BiLaplacian (defaults 0.1, 0.1, spacing 1/64): growth 4, P_c = 4096, definite, lambda_min / lambda_max = +8.6e-10; the old
    route ends at growth 3, indefinite (-1.9e-8).
    129 x 129 (spacing 1/128): growth 4, P_c = 8192, definite, +5.4e-11; the old route ends at growth 3, P_c = 4096, indefinite (-2.4e-8),
    and growth 4 is past its line.
    1-D 1025 nodes, matern52, ell = 1, spacing 1/1024: growth 3, P = 32768; the old route has growth 0 alone, indefinite (-3.1e-3)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "grid_long_growth.json")) as f:
        golden = json.load(f)
    kw = hf.bilaplacian_kernel_2d(0.1, 0.1)
    for n, Pc, want, old in ((65, 4096, 8.6e-10, -1.9e-8), (129, 8192, 5.4e-11, -2.4e-8)):
        shape, trace = (n, n), []
        g, P, ratio, definite = lt.sampler_growth(shape, (1 / (n - 1),) * 2, kw["family"], kw["sigma"], kw["ell"], 0.0, kw["metric"], max_growth=6,
                                                  trace=trace)
        print("%d^2: growth %d P %s ratio %.3g; growth 3: %.3g" % (n, g, P, ratio, trace[3][2] / trace[3][3]))
        assert (g, P, definite) == (4, [Pc, Pc], True) and ratio > 0 and abs(ratio - want) <= 0.02 * want
        assert [t[0] for t in trace] == [0, 1, 2, 3, 4] and not any(t[4] for t in trace[:4])
        # the record the GPU suite holds the device's info to (tests/golden/grid_long_growth.json): these extremes, within rounding
        rec = golden["bilaplacian_%dx%d" % (n, n)]
        lo4, hi4 = trace[4][2], trace[4][3]
        assert (rec["growth"], rec["embedding"]) == (g, P)
        assert max(abs(lo4 - rec["lambda_min"]), abs(hi4 - rec["lambda_max"])) <= 16 * lt.EPS * np.log2(Pc * Pc) * hi4 < 0.01 * lo4
        # the old route on this grid: growth 3 is its last, on 8 n' <= 4096 per axis, and indefinite far below the floor
        assert old_route_could(shape, 3) and not old_route_could(shape, 4)
        g3, P3, lo3, hi3, def3 = trace[3]
        assert P3 == [Pc // 2, Pc // 2] and not def3 and lo3 < -1e4 * lt.floor(P3[0] * P3[1], hi3) and abs(lo3 / hi3 - old) <= 0.05 * abs(old)
    assert lt.feasible((129, 129), 4, 4096) and max(lt.embedding((129, 129), 4)[1]) > 4096
    g, P, ratio, definite = lt.sampler_growth((1025,), (1 / 1024,), "matern52", 1.0, 1.0, 0.0, max_growth=6)
    assert (g, P, definite) == (3, [32768], True)
    g, P, ratio, definite = lt.sampler_growth((1025,), (1 / 1024,), "matern52", 1.0, 1.0, 0.0, max_growth=3, long_route=False)
    assert (g, P, definite) == (0, [4096], False) and ratio < -1e-3


def test_bindings():
    for name in ("hfmi_op_kernel_cov_grid_long", "hfmi_grid_sampler_create_long", "hfmi_fftcov_long_plan_predict"):
        assert name in L.SIGNATURES
    assert L.FFTCOV_LONG_PLAN_WORDS == lt.PLAN_WORDS and L.GRID_COV_LONG_MAX_NODES == lt.LONG_MAXN
