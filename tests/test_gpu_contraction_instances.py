"""GPU sweep over the compiled instances of the three tall-skinny contractions (k_tsgemm_tn, k_tsgemm_nn / k_tsgemm_nn_res,
k_tsgemm_ss / k_tsgemm_ssb) and the partial-sum kernels behind them.  The case lists come from tests/helpers/contraction_plan_twin.py
(tests/test_contraction_plan_cpu.py shows that they reach every instance); every case sets the knobs, clears the plan record, runs,
and asserts that the record equals the twin's prediction -- so a case fails if the intended instance did not run -- before it
compares values.

Exact leg: integer operands in [-a, a] with (reduction length) a^2 <= 2^51 (a = 2^19 up to 8192 terms): every product and every
partial sum in any order is an integer below 2^51, exactly representable in fp64, so the int64 numpy product is the reference
and the comparison is equality.  scale / beta are +-powers of two and C0 is a small integer, which keeps that exact.  Rounding
leg: one Gaussian case per family against a long-double product under the bounds of tests/test_gpu_kernels.py.  Guard leg: the
result is prefilled with NaN where beta == 0 and the columns behind the fast extent carry a sentinel that must come back bit
for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import contraction_plan_twin as twin  # noqa: E402

SENTINEL = np.array([0x7FF8C0DEFACE0001], dtype=np.uint64).view(np.float64)[0]     # a NaN with a payload: compared as bits


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


@pytest.fixture(scope="module")
def cus(ctx):
    return ctx.device_info()["compute_units"]


@pytest.fixture(autouse=True)
def default_knobs():
    yield
    for key, val in twin.DEFAULT_KNOBS.items():
        L.call("hfmi_tuning_set", key.encode(), val)


def set_knobs(kw):
    kn = twin.knobs(**kw)
    for key, val in kn.items():
        L.call("hfmi_tuning_set", key.encode(), val)
    return kn


def plan_clear(ctx):
    L.call("hfmi_plan_clear", ctx.handle)


def plan_read(ctx):
    words = (C.c_int * (256 * twin.PLAN_WORDS))()
    n, total = C.c_int(0), C.c_int(0)
    L.call("hfmi_plan_read", ctx.handle, 256, words, C.byref(n), C.byref(total))
    assert total.value == n.value, "more launches than the ring holds"
    flat = list(words)
    return [twin.decode(flat[i * twin.PLAN_WORDS:(i + 1) * twin.PLAN_WORDS]) for i in range(n.value)]


def ints(rng, shape, amp):
    return rng.integers(-amp, amp, size=shape, endpoint=True).astype(np.float64)


def assert_exact(got, want, what):
    """equality; the wrong entries are named as (row tile, column tile, row and column inside the 16 x 16 tile)"""
    bad = np.argwhere(~(got == want))
    if bad.size:
        rows = ["(row tile %d, col tile %d, lane %d,%d): got %r want %r" % (i // 16, j // 16, i % 16, j % 16, got[i, j], want[i, j])
                for i, j in bad[:10]]
        tiles = sorted({(int(i) // 16, int(j) // 16) for i, j in bad})
        pytest.fail("%s: %d wrong entries in tiles %s\n%s" % (what, len(bad), tiles[:20], "\n".join(rows)))


def run_tn(ctx, cus, c, rng, swap_check=False):
    """one call of the tn entry (tn or skinny route): record == twin, exact values, NaN prefill overwritten, guard untouched"""
    m, k, N, tr = c["m"], c["k"], c["N"], c["tr"]
    same = c.get("same", False)
    amp = twin.exact_amplitude(N)
    A = ints(rng, (N, m), amp)
    B = A if same else ints(rng, (N, k), amp)
    Am = hf.MultiVector.from_dense(A)
    Bm = Am if same else hf.MultiVector.from_dense(B)
    fast, slow = (m, k) if tr else (k, m)
    ld = twin.out_ld(c, fast)
    rs, cs = (1, ld) if tr else (ld, 1)
    host = np.full((slow, ld), SENTINEL)
    C0 = ints(rng, (slow, fast), 1 << 19) if c["beta"] != 0.0 else np.full((slow, fast), np.nan)
    host[:, :fast] = C0
    kn = set_knobs(c["knobs"])
    skinny = kn["ss"] and twin.ss_applicable(m, k, same)
    if skinny:
        want = twin.ss_plan(m, k, N, kn, cus, same, c["scale"], c["beta"], rs, cs, c["nsplit"])
    else:
        want = twin.tn_plan(m, k, N, kn, cus, c["scale"], c["beta"], rs, cs, c["nsplit"])
    plan_clear(ctx)
    L.call("hfmi_test_tsgemm_tn", Am.handle, Bm.handle, float(c["scale"]), float(c["beta"]), int(tr), int(ld), int(c["nsplit"]), L.ptr(host))
    got_plan = plan_read(ctx)
    assert got_plan == want, "%r\n ran      %r\n expected %r" % (c, got_plan, want)
    ref = (A.astype(np.int64).T @ B.astype(np.int64)).astype(np.float64)
    expect = c["scale"] * ref + (c["beta"] * C0.T if tr else c["beta"] * C0) if c["beta"] != 0.0 else c["scale"] * ref
    got = host[:, :fast].T if tr else host[:, :fast]
    assert_exact(got, expect, repr(c))
    guard = host[:, fast:]
    # a row-major result whose row stride is the partials' own is reduced as ONE array: its pad columns are written as zeros
    zero_pad = any(r["kind"] == "reduce" and r["route"] in (twin.VEC_LONG, twin.FLAT) for r in want)
    if zero_pad:
        assert not guard.any(), c
    else:
        assert (guard.view(np.uint64) == np.array([SENTINEL]).view(np.uint64)[0]).all(), "guard columns written: %r" % (c,)
    if swap_check:
        other = np.full((k, m + 3), SENTINEL)
        other[:, :m] = np.nan
        L.call("hfmi_test_tsgemm_tn", Bm.handle, Am.handle, 1.0, 0.0, 0, m + 3, int(c["nsplit"]), L.ptr(other))
        assert_exact(other[:, :m].T, ref, "transposed problem of %r" % (c,))
    return want


def tn_ids():
    return [(mode, nt) for nt in range(1, 17) for mode in ((4,) if nt > 11 else (8, 4, 44))]


# ------------------------------------------------------------------ tn
@pytest.mark.parametrize("mode,nt", tn_ids(), ids=["waves%d-nt%d" % p for p in tn_ids()])
def test_tn_every_instance_exact(ctx, cus, mode, nt):
    """every <MT, NT, TR, WAVES, R4> the dispatcher reaches at this panel width: the tile height limited by the table, the need
    and the knob in turn, a ragged last row block, both output orders, both boundaries of every remainder class, scale / beta"""
    rng = np.random.default_rng(1000 * mode + nt)
    cases = twin.tn_cases(nt_filter=nt, mode_filter=mode)
    assert cases
    for c in cases:
        want = run_tn(ctx, cus, c, rng)[0]
        got = (twin.tn_mode(want["NT"], twin.knobs(**c["knobs"])), want["MT"], want["NT"], want["TR"], want["R4"])
        assert got == c["want"]


@pytest.mark.parametrize("i", range(len(twin.tn_split_cases())))
def test_tn_forced_splits_and_every_reduce_route_exact(ctx, cus, i):
    """forced splits over the <4> / <16> threshold of the partial-sum kernels, and launch_reduce_partials' routes at m k >= 65536:
    one long row, row by row, flat, scalar for an odd fast extent (a single odd row must not lose its last element)"""
    run_tn(ctx, cus, twin.tn_split_cases()[i], np.random.default_rng(i))


def test_tn_hybrid_plan_exact(ctx, cus):
    """more row blocks than CUs with scale != 1: whole rounds coarsely split plus a finely split tail, two reductions"""
    c = twin.TN_HYBRID_CASE
    want = run_tn(ctx, cus, c, np.random.default_rng(7))
    assert want[0]["tail_nrb"] > 0 and want[0]["nrb"] + want[0]["tail_nrb"] > cus


# ------------------------------------------------------------------ skinny x skinny
@pytest.mark.parametrize("rt", range(1, 11))
def test_ss_every_tile_shape_exact(ctx, cus, rt):
    """every (rt, ct) with rt + ct <= 18 under ss_blocked 0, 1 and 2, and the one-operand Gram; where the blocked kernel swaps the
    operand roles (rt > ct) the transposed problem must give the same numbers"""
    rng = np.random.default_rng(50 + rt)
    cases = [c for c in twin.ss_cases() if c["rt"] == rt]
    assert len(cases) >= 3
    for c in cases:
        c = dict(c, knobs=dict(c["knobs"]))
        want = run_tn(ctx, cus, c, rng, swap_check=(not c["same"] and rt > c["ct"]))
        assert want[0]["kind"] in ("ss", "ssb")
        if c["same"]:
            assert want[0]["same"] == 1


@pytest.mark.parametrize("percu", [1, 4])
def test_ss_grid_sized_by_resident_workgroups_exact(ctx, cus, percu):
    c = {"knobs": {"ss_percu": percu}, "m": 16, "k": 15, "N": 70001, "tr": 0, "scale": 1.0, "beta": 0.0, "nsplit": 0}
    want = run_tn(ctx, cus, c, np.random.default_rng(percu))
    assert want[0]["kind"] == "ss" and want[0]["nsplit"] > cus * percu // 2       # the count itself is the twin's: here only that the grid follows the knob


# ------------------------------------------------------------------ nn
def run_nn(ctx, cus, c, rng):
    N, m, r = c["N"], c["m"], c["r"]
    amp = twin.exact_amplitude(m)
    A = ints(rng, (N, m), amp)
    S = ints(rng, (m, r), amp)
    Am = hf.MultiVector.from_dense(A)
    if c["inplace"]:
        assert m == r and c["beta"] == 0.0
        Y0, Ym = A, Am
    else:
        Y0 = ints(rng, (N, r), 1 << 19) if c["beta"] != 0.0 else np.full((N, r), np.nan)
        Ym = hf.MultiVector.from_dense(Y0)
    kn = set_knobs(c["knobs"])
    want = twin.nn_plan(m, r, N, kn, cus)
    plan_clear(ctx)
    L.call("hfmi_block_gemm_small", Am.handle, L.ptr(np.ascontiguousarray(S)), float(c["alpha"]), float(c["beta"]), Ym.handle)
    got_plan = plan_read(ctx)
    assert got_plan == [want], "%r\n ran      %r\n expected %r" % (c, got_plan, want)
    ref = (A.astype(np.int64) @ S.astype(np.int64)).astype(np.float64)
    expect = c["alpha"] * ref + c["beta"] * Y0 if c["beta"] != 0.0 else c["alpha"] * ref
    got = Ym.to_dense()
    assert_exact(got, expect, repr(c))
    return want, got


@pytest.mark.parametrize("nt", range(1, 17))
def test_nn_streaming_every_instance_exact(ctx, cus, nt):
    """nn_res = 0: every <TT, NT, WAVES, R4> of the streaming kernel (4 waves at the three tile heights, 8 waves), two tiles plus
    a ragged rest, short reductions with a ragged last stage, alpha / beta, and in place"""
    rng = np.random.default_rng(300 + nt)
    cases = [c for c in twin.nn_stream_cases() if c["want"][1] == nt]
    assert len(cases) >= 8
    for c in cases:
        want, _ = run_nn(ctx, cus, c, rng)
        assert (want["TT"], want["NT"], want["WAVES"], want["R4"]) == c["want"]
    c = cases[0]
    run_nn(ctx, cus, dict(c, m=c["r"], alpha=0.5, beta=0.0, inplace=True), rng)


def test_nn_streaming_reduction_split_exact(ctx, cus):
    want, _ = run_nn(ctx, cus, twin.NN_MSPLIT_CASE, np.random.default_rng(11))
    assert want["msplit"] > 1 and want["tail_tiles"] == 1


def test_nn_streaming_tail_split_equals_uniform_split_exact(ctx, cus):
    """one whole round of tiles written directly plus tail tiles split over the reduction axis (nn_hybrid 1) against the uniform
    plan (nn_hybrid 0): the same integers"""
    c = twin.nn_tail_split_case(cus)
    outs = []
    for hyb in (1, 0):
        want, got = run_nn(ctx, cus, dict(c, knobs={"nn_res": 0, "nn_hybrid": hyb}), np.random.default_rng(12))
        assert (want["full_tiles"] == cus and want["tail_tiles"] == 3 and want["msplit"] > 1) if hyb else want["full_tiles"] == 0
        outs.append(got)
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("nt", range(1, 11))
def test_nn_resident_every_instance_exact(ctx, cus, nt):
    """both tile heights and every remainder class of the LDS-resident kernel, N = 4096 + {0, 1, 127}; the reduction is the longest
    160 KB of LDS hold at this width (1280 rows at one column tile), three rows short of it, or a short ragged one"""
    rng = np.random.default_rng(400 + nt)
    cases = [c for c in twin.nn_res_cases() if c["want"][1] == nt]
    assert len(cases) >= 4
    for c in cases:
        want, _ = run_nn(ctx, cus, c, rng)
        assert want["kind"] == "nn_res" and (want["TT"], want["NT"], want["R4"], want["UPPER"]) == c["want"]
    c = cases[0]
    run_nn(ctx, cus, dict(c, m=c["r"], alpha=1.0, beta=0.0, inplace=True), rng)


@pytest.mark.parametrize("nt", range(1, 10))
def test_nn_resident_upper_instances_are_bit_identical(ctx, cus, nt):
    """Q <- Q R^-1 of orthogonalize(): with nn_upper = 1 the record must show the UPPER instance of the intended tile height and
    remainder class, and Q and R must not differ by a bit from the nn_upper = 0 run"""
    cases = [c for c in twin.nn_upper_cases() if c["want"][1] == nt]
    assert cases
    for c in cases:
        N, k = c["N"], c["k"]
        Z = np.random.default_rng(N + k).standard_normal((N, k))
        got = {}
        for upper in (0, 1):
            kn = set_knobs(dict(c["knobs"], nn_upper=upper))
            Q = hf.MultiVector.from_dense(Z)
            plan_clear(ctx)
            R = Q.orthogonalize()
            recs = [r for r in plan_read(ctx) if r["kind"] in ("nn", "nn_res")]
            assert recs and all(r == twin.nn_plan(k, k, N, kn, cus, upper_hint=True) for r in recs), (c, recs)
            assert all((r["TT"], r["NT"], r["R4"], r["UPPER"]) == c["want"][:3] + (upper,) for r in recs), (c, recs)
            got[upper] = (R, Q.to_dense())
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), c
        Qd = got[1][1]
        assert np.abs(Qd.T @ Qd - np.eye(k)).max() < 1e-14 * max(k, 8)


# ------------------------------------------------------------------ rounding leg
def assert_family(ctx, kinds, claim):
    """the contraction launches since the last clear are of the family the case is named after"""
    recs = [r for r in plan_read(ctx) if r["kind"] in kinds]
    assert recs, "no contraction launch recorded"
    for r in recs:
        assert {key: r.get(key) for key in claim} == claim, (claim, r)


# (name, knobs, m, k, N, what the record must show).  m = 300 against five column tiles: MT = 5 at 4 waves, 3 in the 44 mode
TN_ROUNDING = [("tn-waves8", {"ss": 0}, 300, 74, 5000, {"kind": "tn", "WAVES": 8, "R4": 3}),
               ("tn-waves4", {"ss": 0, "waves": 4}, 300, 74, 5000, {"kind": "tn", "WAVES": 4, "MT": 5}),
               ("tn-waves44", {"ss": 0, "waves": 44}, 300, 74, 5000, {"kind": "tn", "WAVES": 4, "MT": 3}),
               ("tn-wide", {"ss": 0}, 200, 250, 3000, {"kind": "tn", "WAVES": 4, "NT": 16}),
               ("ss", {"ss_blocked": 0}, 70, 90, 5000, {"kind": "ss", "same": 0}),
               ("ssb", {}, 70, 90, 5000, {"kind": "ssb", "swap": 0, "PIPE": 1}),
               ("ssb-swap", {}, 140, 75, 5000, {"kind": "ssb", "swap": 1, "RT": 5, "CTL": 9})]


@pytest.mark.parametrize("name,kn,m,k,N,claim", TN_ROUNDING, ids=[t[0] for t in TN_ROUNDING])
def test_tn_rounding_against_long_double(ctx, name, kn, m, k, N, claim):
    rng = np.random.default_rng(m * 1000 + k)
    A = rng.standard_normal((N, m)) * np.logspace(0, -3, m)[None, :]
    B = rng.standard_normal((N, k)) + 0.1
    set_knobs(kn)
    Am, Bm = hf.MultiVector.from_dense(A), hf.MultiVector.from_dense(B)
    plan_clear(ctx)
    got = Am.dot_mv(Bm)
    assert_family(ctx, ("tn", "ss", "ssb"), claim)
    ref = (A.astype(np.longdouble).T @ B.astype(np.longdouble)).astype(np.float64)
    scale = np.linalg.norm(A, axis=0)[:, None] * np.linalg.norm(B, axis=0)[None, :]
    err = np.max(np.abs(got - ref) / scale)
    print("%s: max scaled error %.3e" % (name, err))
    assert err < 1e-13


NN_ROUNDING = [("stream-waves4", {"nn_res": 0, "nn_waves": 4}, 3000, 200, 74, {"kind": "nn", "WAVES": 4}),
               ("stream-waves8", {"nn_res": 0, "nn_waves": 8}, 3000, 200, 74, {"kind": "nn", "WAVES": 8}),
               ("resident", {}, 5000, 100, 74, {"kind": "nn_res", "UPPER": 0})]


@pytest.mark.parametrize("name,kn,N,m,r,claim", NN_ROUNDING, ids=[t[0] for t in NN_ROUNDING])
def test_nn_rounding_against_long_double(ctx, name, kn, N, m, r, claim):
    rng = np.random.default_rng(N + m + r)
    A = rng.standard_normal((N, m))
    S = rng.standard_normal((m, r)) * np.logspace(0, -2, r)[None, :]
    set_knobs(kn)
    Y = hf.MultiVector(N, r)
    Am = hf.MultiVector.from_dense(A)
    plan_clear(ctx)
    hf.MvDSmatMult(Am, S, Y)
    assert_family(ctx, ("nn", "nn_res"), claim)
    ref = (A.astype(np.longdouble) @ S.astype(np.longdouble)).astype(np.float64)
    err = np.linalg.norm(Y.to_dense() - ref) / np.linalg.norm(ref)
    print("%s: relative error %.3e" % (name, err))
    assert err < 1e-13
