"""``hfmi_fftcov_plan_predict`` -- the planner the FFT apply of ``hfmi_op_kernel_cov_grid`` itself asks -- against a Python statement of
the plan (tests/helpers/fftcov_plan_twin.py), and against what the kernel needs: embedding lengths, LDS within a workgroup's 160 KiB,
every line of every pass covered exactly once, pairs per chunk within the budget.  No device.  The argument rules of the Python class
that need no device are here too."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_plan_twin as tw                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

AXIS = list(range(1, 71)) + [127, 128, 129, 1024, 1025, 2048]
CORNERS = [1, 2, 3, 5, 16, 17, 33, 64, 70, 127, 128, 129, 1024, 1025, 2048]
BUDGETS = [0, 1, 1 << 20, 1 << 28, 1 << 34]


def shapes():
    out = [(n,) for n in AXIS]
    out += [(a, b) for a in AXIS for b in AXIS]
    out += [(a, b, c) for a in CORNERS for b in CORNERS for c in CORNERS]
    for n in AXIS:                                      # every length on every axis of a 3-D grid
        out += [(n, 3, 5), (3, n, 5), (3, 5, n)]
    return out


def check_plan(shape, nvec, budget, words):
    p = tw.plan(shape, nvec, budget)
    assert words == tw.plan_words(p), (shape, nvec, budget)
    n = list(shape) + [1] * (3 - len(shape))
    for c in range(3):
        P = p["P"][c]
        assert P & (P - 1) == 0 and P >= 2 * n[c] - 1 and (P == 1 or P // 2 < 2 * n[c] - 1), (shape, c)
        assert (P == 1) == (n[c] == 1)
    assert len(p["passes"]) == 2 * len(shape) - 1
    for q in p["passes"]:
        assert q["lds_total"] <= tw.LDS_BYTES and q["lpw"] <= tw.MAX_LINES and 64 <= q["threads"] <= 512 and q["threads"] % 64 == 0, (shape, q)
        assert q["lpw"] & (q["lpw"] - 1) == 0 and q["ls"] >= q["L"]
        # the launch grid takes every line once: grid_x workgroups of lpw consecutive lines, the last one ragged
        assert (q["grid_x"] - 1) * q["lpw"] < q["nlines"] <= q["grid_x"] * q["lpw"], (shape, q)
        assert 1 <= q["nload"] <= q["L"] and 1 <= q["nstore"] <= q["L"]
    assert p["chunk_pairs"] >= 1 and p["chunk_pairs"] * p["nchunks"] >= p["pairs"] > (p["nchunks"] - 1) * p["chunk_pairs"]
    b = budget if budget > 0 else tw.DEFAULT_BUDGET
    assert p["chunk_pairs"] == 1 or p["chunk_pairs"] * p["pair_bytes"] <= b, (shape, budget)
    return p


def test_predict_matches_the_twin_everywhere():
    count = 0
    for i, shape in enumerate(shapes()):
        nvec = (1, 2, 5, 17, 74, 290)[i % 6]
        check_plan(shape, nvec, BUDGETS[i % len(BUDGETS)], tw.predict(L, shape, nvec, BUDGETS[i % len(BUDGETS)]))
        count += 1
    assert count > 9000


@pytest.mark.parametrize("shape", [(1,), (2,), (17,), (2048,), (5, 3), (1, 9), (32, 33), (300, 200), (70, 1), (7, 5, 3), (9, 8, 5),
                                   (33, 2, 17), (1, 1, 4), (129, 3, 2)])
def test_every_line_is_taken_once(shape):
    """the line map of every pass enumerated: distinct lines, exactly the ones the pass must transform, all inside the padded array"""
    p = check_plan(shape, 5, 0, tw.predict(L, shape, 5, 0))
    for q in p["passes"]:
        bases = np.sort(tw.line_bases(q))
        assert np.array_equal(bases, tw.expected_bases(p, shape, q)), (shape, q["axis"])
        assert bases[-1] + (q["L"] - 1) * q["stride"] < p["Ptot"]


def test_pairs_knob_and_budget():
    shape, nvec = (64, 40), 17
    P = tw.embed_len(64) * tw.embed_len(40)
    assert tw.predict(L, shape, nvec, 16 * P * 4)[6] == 4 and tw.predict(L, shape, nvec, 16 * P * 4)[7] == 3
    assert tw.predict(L, shape, nvec, 1)[6] == 1                      # a budget below one pair still takes one
    assert tw.predict(L, shape, nvec, 0)[6] == 9                      # the default budget holds all nine pairs
    for forced in (1, 3):
        L.call("hfmi_tuning_set", b"fftcov_pairs", forced)
        try:
            w = tw.predict(L, shape, nvec, 0)
            assert w == tw.plan_words(tw.plan(shape, nvec, 0, forced)) and w[6] == forced
        finally:
            L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    with pytest.raises(hf.HfmiError):
        L.call("hfmi_tuning_set", b"fftcov_pairs", 4097)
    with pytest.raises(hf.HfmiError):
        L.call("hfmi_tuning_set", b"fftcov_pairs", -1)
    for bad in ((0,), (2049,), (3, 0), (1, 2, 3, 4), ()):
        with pytest.raises((hf.HfmiError, ValueError)):
            if not 1 <= len(bad) <= 3:
                raise ValueError(bad)
            tw.predict(L, bad, 2, 0)


def test_python_argument_rules_need_no_device():
    """every host-checkable rule raises ValueError before a context is asked for (there is none here)"""
    from hippyflow_amd.operators import _check_grid
    ok = dict(shape=(5, 4), spacing=(0.1, 0.2), nodes=None, origin=None, family="matern32", ell=0.1, nugget=0.0)
    _check_grid(**ok)
    bad = [dict(shape=()), dict(shape=(2, 2, 2, 2)), dict(shape=(0, 3)), dict(shape=(2049,)), dict(spacing=(0.1,)), dict(spacing=(0.1, 0.0)),
           dict(spacing=(0.1, -1.0)), dict(spacing=(0.1, np.inf)), dict(spacing=(np.nan, 0.1)), dict(nodes=[]), dict(nodes=[0, 20]),
           dict(nodes=[-1, 2]), dict(nodes=[3, 3]), dict(nodes=[[1, 2]]), dict(origin=(0.0,)), dict(family="matern72"), dict(ell=0.0),
           dict(ell=-1.0), dict(nugget=-1e-3), dict(ell=np.nan)]
    for change in bad:
        with pytest.raises(ValueError):
            _check_grid(**dict(ok, **change))
    if hf.device_count() < 1:
        for change in bad:
            kw = dict(ok, **change)
            with pytest.raises(ValueError):
                hf.GridKernelCovarianceOperator(kw.pop("shape"), kw.pop("spacing"), **kw)
    n, h, nodes, o = _check_grid((5, 4), 0.25, [7, 0, 19], None, "sqexp", 1.0, 0.0)
    assert list(n) == [5, 4] and list(h) == [0.25, 0.25] and list(nodes) == [7, 0, 19] and list(o) == [0.0, 0.0]
    pts = hf.grid_node_points((5, 4), (0.25, 0.5), nodes=[7, 0, 19], origin=(1.0, 2.0))
    assert np.array_equal(pts, [[1.5, 2.5], [1.0, 2.0], [2.0, 3.5]])


def test_bindings_and_build_list():
    assert "hfmi_op_kernel_cov_grid" in L.SIGNATURES and "hfmi_fftcov_plan_predict" in L.SIGNATURES
    assert "hfmi_fftcov.hip" in __import__("hippyflow_amd._build", fromlist=["SOURCES"]).SOURCES
    assert L.FFTCOV_PLAN_WORDS == tw.PLAN_WORDS
