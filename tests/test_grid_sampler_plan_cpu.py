"""``hfmi_fftcov_sample_plan_predict`` -- the planner a draw of the grid sampler (``hfmi_grid_sampler_draw``) itself asks -- against a
Python statement of the plan (tests/helpers/grid_sampler_plan_twin.py) and against what the kernels need: the grown embedding, d passes
of which the first generates its load, LDS within a workgroup's 160 KiB, every line of every pass covered exactly once, and the
pairing of adjacent storage entries that the noise's element map relies on.  No device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_plan_twin as atw                    # noqa: E402
import grid_sampler_plan_twin as tw               # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

AXIS = [1, 2, 3, 4, 5, 8, 9, 13, 16, 17, 33, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
BUDGETS = [0, 1, 1 << 20, 1 << 28, 1 << 34]


def shapes():
    out = [(n,) for n in AXIS]
    out += [(a, b) for a in AXIS for b in AXIS]
    out += [(a, b, c) for a in AXIS[::2] for b in AXIS[1::3] for c in AXIS[::3]]
    return out


def check_plan(shape, growth, nsamples, budget, words):
    p = tw.plan(shape, growth, nsamples, budget)
    assert words == tw.plan_words(p), (shape, growth, nsamples, budget)
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    for c in range(3):
        assert p["P"][c] == (atw.embed_len(n[c]) << growth if n[c] > 1 else 1) and p["P"][c] <= tw.MAXP
    assert words[13] == growth and len(p["passes"]) == d
    for i, q in enumerate(p["passes"]):
        assert q["axis"] == d - 1 - i
        assert q["flags"] == (tw.GEN if i == 0 else 0) | atw.INV | (atw.GATHER if q["axis"] == 0 else 0)
        assert q["nload"] == q["L"] and q["nstore"] == n[q["axis"]]
        assert q["lds_total"] <= atw.LDS_BYTES and q["lpw"] <= atw.MAX_LINES and 64 <= q["threads"] <= 512 and q["threads"] % 64 == 0
        assert (q["grid_x"] - 1) * q["lpw"] < q["nlines"] <= q["grid_x"] * q["lpw"]
    # the noise pass: all lines of the padded array, and two adjacent storage entries for every thread
    q = p["passes"][0]
    assert q["nlines"] == q["stride"] and q["nlines"] * q["L"] == p["Ptot"]
    if q["stride"] > 1:
        assert q["lpw"] >= 2 and q["nlines"] % 2 == 0 and q["stride"] % 2 == 0
    else:
        assert q["L"] >= 2 or p["Ptot"] == 1
    return p


def test_predict_matches_the_twin():
    count = refused = 0
    for i, shape in enumerate(shapes()):
        for g in range(4):
            nsamples, budget = (1, 2, 7, 64, 290)[(i + g) % 5], BUDGETS[(i + g) % len(BUDGETS)]
            if tw.feasible(shape, g):
                check_plan(shape, g, nsamples, budget, tw.predict(L, shape, g, nsamples, budget))
                count += 1
            else:
                with pytest.raises(hf.HfmiError):
                    tw.predict(L, shape, g, nsamples, budget)
                refused += 1
    assert count > 2000 and refused > 500


@pytest.mark.parametrize("shape,growth", [((1,), 3), ((2,), 0), ((33,), 2), ((2048,), 0), ((1025,), 0), ((513,), 1), ((129,), 3), ((13, 5), 0),
                                          ((13, 5), 3), ((1, 9), 2), ((70, 1), 1), ((2048, 3), 0), ((3, 2048), 0), ((7, 6, 5), 1), ((1, 1, 4), 3),
                                          ((129, 3, 2), 2), ((1, 1, 1), 3)])
def test_every_line_is_taken_once(shape, growth):
    """the line map of every pass enumerated: the noise pass takes every line of the padded array, the others the apply's inverse lines"""
    p = check_plan(shape, growth, 5, 0, tw.predict(L, shape, growth, 5, 0))
    for q in p["passes"]:
        bases = np.sort(atw.line_bases(q))
        assert np.array_equal(bases, atw.expected_bases(p, shape, q)), (shape, q["axis"])
        assert bases[-1] + (q["L"] - 1) * q["stride"] < p["Ptot"]


def test_largest_embedding_and_refusals():
    w = tw.predict(L, (2048, 2048), 0, 2)
    assert w[1:4] == [4096, 4096, 1]
    assert tw.predict(L, (1024, 1, 512), 1, 2)[1:4] == [4096, 1, 2048]
    assert tw.predict(L, (129,), 3, 2)[1:4] == [4096, 1, 1]
    assert tw.predict(L, (1, 1), 3, 2)[1:4] == [1, 1, 1]                # axes of one node never grow
    for shape, g in (((2048,), 1), ((1025, 3), 1), ((3, 513), 2), ((257, 2, 2), 3), ((129, 2, 2), 4), ((5,), -1), ((5,), 4), ((0,), 0), ((2049,), 0)):
        with pytest.raises(hf.HfmiError):
            tw.predict(L, shape, g, 2)
    with pytest.raises(hf.HfmiError):
        tw.predict(L, (5, 4), 0, -1)


def test_pairs_knob_and_budget():
    shape, g, ns = (64, 40), 1, 17
    P = 256 * 256
    assert tw.predict(L, shape, g, ns, 16 * P * 4)[6:8] == [4, 3]
    assert tw.predict(L, shape, g, ns, 1)[6] == 1
    assert tw.predict(L, shape, g, ns, 0)[6] == 9
    for forced in (1, 3):
        L.call("hfmi_tuning_set", b"fftcov_pairs", forced)
        try:
            w = tw.predict(L, shape, g, ns, 0)
            assert w == tw.plan_words(tw.plan(shape, g, ns, 0, forced)) and w[6] == forced
        finally:
            L.call("hfmi_tuning_set", b"fftcov_pairs", 0)


def test_the_apply_plan_is_what_it_was():
    """growth 0 shares the embedding with the apply; the apply's own record does not know the draw"""
    for shape in ((33,), (13, 5), (7, 6, 5)):
        a, s = atw.predict(L, shape, 4, 0), tw.predict(L, shape, 0, 4, 0)
        assert a[:8] == s[:8] and a[9:13] == s[9:13] and a[13] == 0
        assert a == atw.plan_words(atw.plan(shape, 4, 0))


def test_bindings():
    for name in ("hfmi_grid_sampler_create", "hfmi_grid_sampler_info", "hfmi_grid_sampler_draw", "hfmi_grid_sampler_destroy",
                 "hfmi_fftcov_sample_plan_predict"):
        assert name in L.SIGNATURES
    assert hf.GridFieldSampler is not None and hasattr(hf.GridKernelCovarianceOperator, "sampler")
