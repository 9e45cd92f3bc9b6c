"""``hfmi_fftcov_factor_plan_predict`` -- the planner an apply of the factor S / S^T of a grid sampler's embedding
(``hfmi_op_grid_factor``) itself asks -- against a Python statement of the pass list (tests/helpers/grid_factor_twin.py) and against
what the kernels need: 2 d - 1 passes, the full-extent half over every line of the padded array, the other half over the apply's
lines, LDS within a workgroup's 160 KiB, every line of every pass taken exactly once and inside the work buffer.  No device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_plan_twin as atw                    # noqa: E402
import grid_sampler_plan_twin as stw              # noqa: E402
import grid_factor_twin as tw                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402

AXIS = [1, 2, 3, 4, 5, 8, 9, 13, 16, 17, 33, 64, 65, 127, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
BUDGETS = [0, 1, 1 << 20, 1 << 28, 1 << 34]


def shapes():
    out = [(n,) for n in AXIS]
    out += [(a, b) for a in AXIS[::2] for b in AXIS]
    out += [(a, b, c) for a in AXIS[::2] for b in AXIS[1::3] for c in AXIS[::3]]
    return out


def check_plan(shape, growth, transpose, nvec, budget, words):
    p = tw.plan(shape, growth, transpose, nvec, budget)
    assert words == tw.plan_words(p), (shape, growth, transpose, nvec, budget)
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    P = p["P"]
    assert words[13] == growth and words[14] == transpose and len(p["passes"]) == 2 * d - 1
    assert p["pairs"] == (nvec + 1) // 2
    axes = list(range(d - 1)) + [d - 1] + list(range(d - 2, -1, -1))
    for i, q in enumerate(p["passes"]):
        a = q["axis"]
        assert a == axes[i]
        fwd, inv = i <= d - 1, i >= d - 1
        assert bool(q["flags"] & atw.FWD) == fwd and bool(q["flags"] & atw.INV) == inv and bool(q["flags"] & atw.MUL) == (i == d - 1)
        assert bool(q["flags"] & atw.SCATTER) == (i == 0) and bool(q["flags"] & atw.GATHER) == (i == 2 * d - 2)
        assert bool(q["flags"] & tw.LOAD_FULL) == (i == 0 and not transpose) and bool(q["flags"] & tw.STORE_FULL) == (i == 2 * d - 2 and transpose == 1)
        # the side of the multiply that holds padded vectors moves P positions, the other the nodes'
        in_full, out_full = not transpose, bool(transpose)
        assert q["nload"] == (P[a] if (not fwd or in_full) else n[a])
        assert q["nstore"] == (P[a] if (not inv or out_full) else n[a])
        assert q["lds_total"] <= atw.LDS_BYTES and q["lpw"] <= atw.MAX_LINES and 64 <= q["threads"] <= 512 and q["threads"] % 64 == 0
        assert (q["grid_x"] - 1) * q["lpw"] < q["nlines"] <= q["grid_x"] * q["lpw"]
    return p


def test_predict_matches_the_twin():
    count = refused = 0
    for i, shape in enumerate(shapes()):
        for g in range(4):
            for transpose in (0, 1):
                nvec, budget = (1, 2, 7, 64, 291)[(i + g + transpose) % 5], BUDGETS[(i + g) % len(BUDGETS)]
                if tw.feasible(shape, g):
                    check_plan(shape, g, transpose, nvec, budget, tw.predict(L, shape, g, transpose, nvec, budget))
                    count += 1
                else:
                    with pytest.raises(hf.HfmiError):
                        tw.predict(L, shape, g, transpose, nvec, budget)
                    refused += 1
    assert count > 2000 and refused > 500


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("shape,growth", [((1,), 3), ((2,), 0), ((7,), 1), ((33,), 2), ((2048,), 0), ((513,), 1), ((6, 5), 0), ((17, 12), 2),
                                          ((1, 9), 2), ((70, 1), 1), ((300, 70), 1), ((2048, 3), 0), ((3, 2048), 0), ((4, 3, 3), 0),
                                          ((9, 8, 7), 1), ((1, 1, 4), 3), ((129, 3, 2), 2), ((1, 1, 1), 3)])
def test_every_line_is_taken_once(shape, growth, transpose):
    """the line map of every pass enumerated: the full-extent half takes every line of the padded array, the other half the apply's"""
    p = check_plan(shape, growth, transpose, 5, 0, tw.predict(L, shape, growth, transpose, 5, 0))
    d = len(shape)
    for i, q in enumerate(p["passes"]):
        full_above = (i < d - 1 and not transpose) or (i > d - 1 and transpose == 1)
        bases = np.sort(atw.line_bases(q))
        assert np.array_equal(bases, tw.expected_bases(p, shape, q, full_above)), (shape, q["axis"], i)
        assert bases[-1] + (q["L"] - 1) * q["stride"] < p["Ptot"]
        if q["flags"] & (tw.LOAD_FULL | tw.STORE_FULL) and d > 1:
            # the direct load / store: line o of the pass along axis 0 is entries o P_0 .. o P_0 + P_0 - 1 of the padded vector
            assert np.array_equal(atw.line_bases(q), np.arange(q["nlines"]) * p["P"][0]) and q["nlines"] * p["P"][0] == p["Ptot"]


def test_refusals_are_the_samplers():
    """HFMI_ERR_INVALID exactly where hfmi_fftcov_sample_plan_predict refuses, and for a transpose outside 0 / 1"""
    for shape, g, nvec in (((2048,), 1, 2), ((1025, 3), 1, 2), ((3, 513), 2, 2), ((257, 2, 2), 3, 2), ((129, 2, 2), 4, 2), ((5,), -1, 2), ((5,), 4, 2),
                           ((0,), 0, 2), ((2049,), 0, 2), ((5, 4), 0, -1), ((2048, 2048), 0, 2), ((129,), 3, 2), ((1, 1), 3, 0)):
        outcome = []
        for call in (lambda: stw.predict(L, shape, g, nvec), lambda: tw.predict(L, shape, g, 0, nvec), lambda: tw.predict(L, shape, g, 1, nvec)):
            try:
                call()
                outcome.append(True)
            except hf.HfmiError:
                outcome.append(False)
        assert outcome[0] == outcome[1] == outcome[2], (shape, g, nvec, outcome)
    for transpose in (-1, 2):
        with pytest.raises(hf.HfmiError):
            tw.predict(L, (5, 4), 0, transpose, 2)


def test_pairs_knob_and_budget():
    shape, g, nv = (64, 40), 1, 17
    P = 256 * 256
    for transpose in (0, 1):
        assert tw.predict(L, shape, g, transpose, nv, 16 * P * 4)[6:8] == [4, 3]
        assert tw.predict(L, shape, g, transpose, nv, 1)[6] == 1
        assert tw.predict(L, shape, g, transpose, nv, 0)[6] == 9
        for forced in (1, 3):
            L.call("hfmi_tuning_set", b"fftcov_pairs", forced)
            try:
                w = tw.predict(L, shape, g, transpose, nv, 0)
                assert w == tw.plan_words(tw.plan(shape, g, transpose, nv, 0, forced)) and w[6] == forced
            finally:
                L.call("hfmi_tuning_set", b"fftcov_pairs", 0)


def test_the_other_plans_are_what_they_were():
    """the embedding, chunking and inverse half are the draw's; the apply's and the draw's own records do not know the factor"""
    for shape, g in (((33,), 1), ((13, 5), 0), ((7, 6, 5), 2)):
        s, f = stw.predict(L, shape, g, 4, 0), tw.predict(L, shape, g, 0, 4, 0)
        assert s == stw.plan_words(stw.plan(shape, g, 4, 0)) and s[14] == 0
        assert s[:8] == f[:8] and s[9:14] == f[9:14]
        d = len(shape)
        for i in range(1, d):                               # S: the inverse passes after the fused one are the draw's
            a = atw.HEAD_WORDS + (d - 1 + i) * atw.PASS_WORDS
            b = atw.HEAD_WORDS + i * atw.PASS_WORDS
            assert f[a:a + atw.PASS_WORDS] == s[b:b + atw.PASS_WORDS]
    assert atw.predict(L, (13, 5), 4, 0) == atw.plan_words(atw.plan((13, 5), 4, 0))


def test_bindings():
    for name in ("hfmi_op_grid_factor", "hfmi_fftcov_factor_plan_predict"):
        assert name in L.SIGNATURES
    assert hf.GridCovarianceFactor is not None and hf.GridKernelPrior is not None and hasattr(hf.GridFieldSampler, "factor")
    header = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    assert "hfmi_op_grid_factor(hfmi_grid_sampler* s" in header and "hfmi_fftcov_factor_plan_predict(" in header
