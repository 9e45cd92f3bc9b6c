"""CPU suite: the route of the general fp64 MFMA product (``dgemm_route_make`` of hippyflow_amd/csrc/hfmi_dgemm.h, the function
``launch_dgemm`` calls) through ``hfmi_dgemm_route_predict`` -- no device involved -- against its plain-Python twin
(tests/helpers/dgemm_twin.py): on every case list of tests/test_gpu_dgemm_descriptor.py, on a seeded sweep around the edges of the
rule, on the two refusals and on the no-op.  The case lists are also shown to reach every kernel instance and load path, so that a
list that stops reaching one fails here and not silently on the GPU."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dgemm_twin as twin  # noqa: E402

from hippyflow_amd import _lib as L  # noqa: E402


def predict(d, pipelined=1):
    return L.Context.dgemm_route_predict(d, pipelined)


def check(d, pipelined=1):
    got, want = predict(d, pipelined), twin.route(d, pipelined)
    assert got == want, "%r (switch %d)\n library %r\n twin    %r" % (d, pipelined, got, want)
    return got


def test_route_of_every_gpu_case_equals_the_twin():
    cases = twin.all_default_cases()
    assert len(cases) > 500
    assert len({c["name"] for c in cases}) == len(cases), "case names must be unique"
    for c in cases:
        check(c, 1)
    for c in twin.gemm0_cases():
        r = check(c, 0)
        assert r["kernel"] == twin.K64 and r["vec"] == 0


def test_case_lists_reach_the_kernels_they_are_named_after():
    for ta, tb in twin.TT:
        for c in twin.p128_cases(ta, tb):
            assert twin.route(c)["kernel"] == twin.P128 and twin.route(c)["gx"] == 2 and twin.route(c)["gy"] == 96, c["name"]
            assert twin.route(c)["vec"] == (0 if any(w in c["name"] for w, _ in twin.UNALIGNED) else 1), c["name"]
        for c in twin.p64_cases(ta, tb):
            assert twin.route(c)["kernel"] == twin.P64 and twin.route(c)["gx"] == 4 and twin.route(c)["gy"] == 48, c["name"]
        for c in twin.k64_cases(ta, tb):
            assert twin.route(c)["kernel"] == twin.K64, c["name"]
        # every value of every axis occurs with every (ta, tb) on the 128-tile list
        cs = twin.p128_cases(ta, tb)
        assert {(c["K"], c["K2"]) for c in cs} == set(twin.KK) and {(c["alpha"], c["beta"]) for c in cs} == set(twin.AB)
        assert sum(c["lda"] % 2 for c in cs) == 1 and sum(c["ldb"] % 2 for c in cs) == 1
        assert sum(c["off_A"] for c in cs) == 1 and sum(c["off_B2"] for c in cs) == 1
    assert {(c["K"], c["K2"]) for t in twin.TT for c in twin.p64_cases(*t)} == set(twin.KK)
    kinds = {c["name"]: twin.route(c)["kernel"] for c in twin.batch_cases()}
    assert all(k == (twin.P128 if name.startswith("batch48") else twin.K64) for name, k in kinds.items()), kinds
    assert any(c["sA"] % 2 for c in twin.batch_cases()) and any(c["beta"] != 0 for c in twin.batch_cases())
    assert all(c["sC"] > c["ldc"] * c["N"] for c in twin.batch_cases())
    for n, kern in zip(twin.LOWER_SHAPES, (twin.P128, twin.P64)):
        for lo in twin.LOWER_VALUES:
            assert twin.route(twin.lower_case(n, lo))["kernel"] == kern
    for cut in twin.CUT_VALUES:
        assert all(twin.route(c)["kernel"] == twin.K64_CUT for c in twin.cut_cases(cut))
    assert all(twin.route(c)["kernel"] == twin.K64_CUT for c in twin.cw_cases() + twin.skip_up_cases())
    assert all(twin.route(c)["error"] == twin.ERR_K2_BATCH for c in twin.batch_refusals())
    assert all(twin.route(c)["error"] == twin.ERR_CUT for c in twin.cut_refusals())
    assert [twin.route(c)["kernel"] for c in twin.rounding_cases()] == [twin.K64, twin.P128, twin.P64]


def test_case_lists_together_reach_every_instance():
    """all four kernels; both load paths on the pipelined ones; all four (ta, tb) on the three uncut kernels, both legal ones on the
    cut kernel"""
    reached = {twin.instance(c) for c in twin.all_default_cases()} - {None}
    want = {(k, ta, tb, vec) for k in (twin.P128, twin.P64) for ta, tb in twin.TT for vec in (0, 1)}
    want |= {(twin.K64, ta, tb, 0) for ta, tb in twin.TT}
    want |= {(twin.K64_CUT, 0, tb, 0) for tb in (0, 1)}
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    # the exact leg reaches them on its own (the rounding cases add none), and the switch-off cases all four orientations of nothing
    # but the 64 x 64 kernel
    exact = {twin.instance(c) for c in twin.all_default_cases() if not c["name"].startswith("round-")} - {None}
    assert exact == want
    assert {twin.instance(c, 0)[0] for c in twin.gemm0_cases()} == {twin.K64}


def _factor3(rng, t):
    """t = a b c, a random factorisation"""
    divs = [x for x in range(1, t + 1) if t % x == 0]
    a = rng.choice(divs)
    divs = [x for x in range(1, t // a + 1) if (t // a) % x == 0]
    b = rng.choice(divs)
    return a, b, t // a // b


def _edge_desc(rng):
    """a descriptor next to an edge of the rule: 191 / 192 / 193 tiles of either size reached through M, N and batch, K + K2 of
    31 / 32 / 33, odd and even leading dimensions and strides, every alignment"""
    tiles = rng.choice((191, 192, 193))
    a, b, c = _factor3(rng, tiles)
    bm = rng.choice((128, 64))
    M = bm * a - rng.choice((0, 1, bm - 1))
    N = 128 * b - rng.choice((0, 1, 127))
    ksum = rng.choice((31, 32, 33, 64))
    K2 = rng.choice((0, 0, 1, 15, 16, 17, ksum))
    d = dict(M=M, N=N, K=ksum - K2, K2=K2, batch=c, ta=rng.randrange(2), tb=rng.randrange(2))
    for key in ("lda", "ldb", "sA", "sB"):
        d[key] = rng.choice((256, 258, 1000)) + (rng.random() < 0.15)
    for x in ("A", "B", "A2", "B2"):
        d["align_" + x] = 8 * (rng.random() < 0.15)
    d["cut"] = rng.choice((0, 0, 0, 0, 0, 1, 2, 4, 3, 7))
    d["has_skip"] = int(rng.random() < 0.1)
    return d


def test_route_sweep_around_the_edges_of_the_rule():
    rng = random.Random(20240607)
    seen, kernels = set(), {}
    for _ in range(6000):
        d = _edge_desc(rng)
        pipelined = 0 if rng.random() < 0.1 else 1
        r = check(d, pipelined)
        cut = d["cut"] != 0 or d["has_skip"]
        if r["error"] == twin.ERR_NONE:
            kernels[r["kernel"]] = kernels.get(r["kernel"], 0) + 1
            # what the rule promises, stated once more without the twin
            if cut:
                assert r["kernel"] == twin.K64_CUT            # however large the shape
            elif not pipelined:
                assert r["kernel"] == twin.K64
            if r["kernel"] in (twin.P128, twin.P64):
                assert d["K"] + d["K2"] >= 32 and r["gx"] * r["gy"] * r["gz"] >= 192
            seen.add((r["kernel"], r["vec"], d["K"] + d["K2"]))
    assert min(kernels.get(k, 0) for k in (twin.K64, twin.K64_CUT, twin.P128, twin.P64)) > 100, kernels
    for k in (twin.P128, twin.P64):
        assert {(k, 0, 32), (k, 1, 32), (k, 0, 33), (k, 1, 33)} <= seen
    assert (twin.K64, 0, 31) in seen


@pytest.mark.parametrize("tiles", [191, 192, 193])
@pytest.mark.parametrize("ksum", [31, 32, 33])
def test_route_edges_one_by_one(tiles, ksum):
    """the thresholds themselves, each through M, through N and through batch, and with the reduction split over two products"""
    for K2 in (0, 1, 16, ksum):
        for M, N, batch in ((128 * tiles, 128, 1), (128, 128 * tiles, 1), (128, 128, tiles), (100, 1, tiles), (64 * tiles, 100, 1)):
            d = dict(M=M, N=N, K=ksum - K2, K2=K2 if batch == 1 else 0, batch=batch, ta=0, tb=1, lda=M + 2, ldb=N + 2, sA=2 * M * 40, sB=2 * N * 40)
            if batch > 1:
                d["K"] = ksum
            r = check(d)
            t128, t64 = -(-M // 128) * -(-N // 128) * batch, -(-M // 64) * -(-N // 128) * batch
            assert tiles in (t128, t64)
            want = twin.K64 if ksum < 32 else twin.P128 if t128 >= 192 else twin.P64 if t64 >= 192 else twin.K64
            assert r["kernel"] == want, (d, r)
            assert check(d, 0)["kernel"] == twin.K64
            assert check(dict(d, cut=1, K2=0), 1)["kernel"] == twin.K64_CUT
            assert check(dict(d, has_skip=1, K2=0), 1)["kernel"] == twin.K64_CUT


def test_vec_needs_every_operand_even_and_aligned():
    base = dict(M=130, N=12161, K=40, K2=23, ta=0, tb=0, lda=130, ldb=64, sA=0, sB=0)
    assert check(base) == dict(kernel=twin.P128, vec=1, gx=2, gy=96, gz=1, error=0)
    for key in ("lda", "ldb", "sA", "sB"):
        assert check(dict(base, **{key: base[key] + 1}))["vec"] == 0
    for x in ("A", "B", "A2", "B2"):
        assert check(dict(base, **{"align_" + x: 8}))["vec"] == 0
        # without a second product its pointers do not count
        assert check(dict(base, K=63, K2=0, **{"align_" + x: 8}))["vec"] == (1 if x in ("A2", "B2") else 0)


def test_the_two_refusals_and_the_no_op():
    big = dict(M=1700, N=1700, K=32, lda=1700, ldb=1700)
    for batch in (2, 48):
        for K2 in (1, 32):
            r = check(dict(big, K2=K2, batch=batch, ta=0, tb=1))
            assert r == dict(kernel=twin.NONE, vec=0, gx=0, gy=0, gz=0, error=twin.ERR_K2_BATCH)
    for kw in (dict(cut=1), dict(cut=2), dict(cut=4), dict(cut=7), dict(has_skip=1)):
        for ta, tb, K2 in ((1, 0, 0), (1, 1, 0), (0, 0, 5), (0, 1, 5), (1, 0, 5)):
            r = check(dict(big, ta=ta, tb=tb, K2=K2, **kw))
            assert r["error"] == twin.ERR_CUT and r["kernel"] == twin.NONE
        for tb in (0, 1):
            assert check(dict(big, ta=0, tb=tb, **kw))["error"] == twin.ERR_NONE
    # M <= 0 or N <= 0: nothing to do, and nothing to refuse either
    for M, N in ((0, 5), (5, 0), (0, 0), (-1, 5), (5, -3)):
        for extra in (dict(), dict(K2=5, batch=3), dict(cut=1, ta=1)):
            r = check(dict(dict(big, M=M, N=N, ta=0, tb=0), **extra))
            assert r == dict(kernel=twin.NONE, vec=0, gx=0, gy=0, gz=0, error=twin.ERR_NONE)


def test_exact_amplitude_rule():
    for c in twin.all_default_cases():
        if c["name"].startswith("round-"):
            continue
        a = twin.exact_amplitude(c)
        assert a >= 1 << 16, (c["name"], a)         # operands that use the upper half of the mantissa in the products
        assert (c["K"] + c["K2"]) * a * a * max(abs(c["alpha"]), 1.0) + abs(c["beta"]) * twin.C0_AMP < 2.0 ** 52
