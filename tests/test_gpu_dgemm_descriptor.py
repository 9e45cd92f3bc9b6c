"""GPU sweep over the whole descriptor of the general fp64 MFMA product (launch_dgemm of hippyflow_amd/csrc/hfmi_dgemm.hip: k_dgemm,
k_dgemm<CUT>, k_dgemm_p<128 | 64>) through ``hfmi_test_dgemm``, which passes the descriptor verbatim.  The case lists and the
reference come from tests/helpers/dgemm_twin.py (tests/test_dgemm_route_cpu.py shows that the lists reach every instance).  Every
case takes three steps: the route that ran equals the twin's, so the intended kernel ran; the values equal the twin's exactly;
every double of the returned C allocation that the twin says is not written equals its prefill as bits.

Exact leg: integer operands in [-a, a] with (K + K2) a^2 |alpha| + |beta| max|C0| < 2^53 u (twin.exact_amplitude), alpha and beta
+-powers of two, integer C0: any summation order is exact and the float64 BLAS product of the integer arrays is the reference.
Prefill: a payload NaN in pads, gaps, guards and skipped tiles; NaN in the written part when beta == 0 (beta == 0 must not read C),
small integers there otherwise.  The operands carry NaN in their own pad rows, gaps and guards: nothing there may be read.
Rounding leg: one Gaussian case per kernel against the long-double product under the derived bound of twin.rounding_bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hf = pytest.importorskip("hippyflow_amd")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dgemm_twin as twin  # noqa: E402

HFMI_OK, HFMI_ERR_INVALID = 0, -1          # include/hfmi.h


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_exact(got, want, mask, what, tile=(64, 64)):
    """equality where mask; the wrong entries are named by tile of the kernel's grid and by position inside the 16 x 16 MFMA tile"""
    bad = np.argwhere(mask & ~(got == want))
    if bad.size:
        rows = ["(tile %d,%d; row %d col %d; lane %d,%d): got %r want %r" % (i // tile[0], j // tile[1], i, j, i % 16, j % 16, got[i, j], want[i, j])
                for i, j in bad[:10]]
        tiles = sorted({(int(i) // tile[0], int(j) // tile[1]) for i, j in bad})
        pytest.fail("%s: %d wrong entries in tiles %s\n%s" % (what, len(bad), tiles[:20], "\n".join(rows)))


def launch(ctx, d, ops, pipelined=1):
    """one launch; asserts the route.  Returns (whole C allocation after the launch, route, launch status)"""
    A, B, A2, B2, C0 = ops
    got, route, status = ctx.test_dgemm(d, A, B, C0, A2, B2)
    want = twin.route(d, pipelined)
    assert route == want, "%s\n ran      %r\n expected %r" % (d["name"], route, want)
    return got, route, status


def run_case(ctx, d, rng, pipelined=1):
    """route == twin, exact values in what is written, bit-identical prefill everywhere else; returns (C allocation, written mask)"""
    ops = twin.fill_operands(d, rng)
    C0 = ops[4]
    got, route, status = launch(ctx, d, ops, pipelined)
    assert status == HFMI_OK, d["name"]
    expect, written = twin.reference(d, route, *ops)
    bm = (128, 128) if route["kernel"] == twin.P128 else (64, 128) if route["kernel"] == twin.P64 else (64, 64)
    for b in range(d["batch"]):
        assert_exact(twin.view(got, d, "C", b), twin.view(expect, d, "C", b), twin.view(written, d, "C", b), "%s batch %d" % (d["name"], b), bm)
    assert np.isfinite(got[written]).all(), d["name"]
    untouched = bits(got)[~written] == bits(C0)[~written]
    if not untouched.all():
        where = np.flatnonzero(~written)[~untouched]
        pytest.fail("%s: %d doubles outside the written part changed, first at offsets %s of the C allocation (off_C %d, ldc %d, sC %d)"
                    % (d["name"], where.size, where[:10].tolist(), d["off_C"], d["ldc"], d["sC"]))
    return got, written


def run_refusal(ctx, d, rng, error):
    ops = twin.fill_operands(d, rng)
    got, route, status = launch(ctx, d, ops)
    assert route["error"] == error and route["kernel"] == twin.NONE
    assert status == HFMI_ERR_INVALID, d["name"]
    assert (bits(got) == bits(ops[4])).all(), "%s: a refused launch wrote to C" % d["name"]


TT_IDS = [twin.tt_name(*t) for t in twin.TT]


# ------------------------------------------------------------------ pipelined kernels
@pytest.mark.parametrize("ta,tb", twin.TT, ids=TT_IDS)
def test_pipelined_128_every_axis_exact(ctx, ta, tb):
    """k_dgemm_p<ta, tb, 128> at 130 x 12161 (2 x 96 tiles, ragged both ways): a reduction of exactly two slabs, ragged slabs, a
    second product, a first product shorter than a slab, alpha / beta with the clamped old-value loads of the ragged edge, and the
    four ways to lose the 16-byte load path (vec = 0 for interior tiles)"""
    rng = np.random.default_rng(100 + 2 * ta + tb)
    cases = twin.p128_cases(ta, tb)
    for d in cases:
        run_case(ctx, d, rng)
    assert sorted(twin.route(d)["vec"] for d in cases) == [0] * 4 + [1] * 6


@pytest.mark.parametrize("ta,tb", twin.TT, ids=TT_IDS)
def test_pipelined_64_every_axis_exact(ctx, ta, tb):
    """k_dgemm_p<ta, tb, 64> at 193 x 6021 (t128 = 96, t64 = 192)"""
    rng = np.random.default_rng(200 + 2 * ta + tb)
    for d in twin.p64_cases(ta, tb):
        run_case(ctx, d, rng)


# ------------------------------------------------------------------ batch
@pytest.mark.parametrize("i", range(len(twin.batch_cases())), ids=[c["name"] for c in twin.batch_cases()])
def test_batch_with_strides_and_gaps_exact(ctx, i):
    """blockIdx.z on both kernels: 48 members (pipelined) and 3 (64 x 64), sC > ldc N with sentinel gaps, an odd stride, beta != 0"""
    run_case(ctx, twin.batch_cases()[i], np.random.default_rng(300 + i))


def test_second_product_with_batch_is_refused_and_the_context_stays_usable(ctx):
    rng = np.random.default_rng(310)
    for d in twin.batch_refusals():
        run_refusal(ctx, d, rng, twin.ERR_K2_BATCH)
        run_case(ctx, twin.batch_cases()[4], rng)          # the next launch on the same context is an ordinary one


# ------------------------------------------------------------------ lower: the eigensolver's rank-2k update
_LOWER_KEPT = {}


@pytest.mark.parametrize("lower", twin.LOWER_VALUES)
@pytest.mark.parametrize("n", twin.LOWER_SHAPES)
def test_lower_symmetric_update_exact(ctx, n, lower):
    """C -= V W^T + W V^T on a symmetric integer C with the tiles above the diagonal 128-blocks skipped: every entry of a kept tile
    equals the reference (run_case), every entry of a skipped tile equals C0 as bits (run_case), the kept tiles cover the lower
    triangle with its diagonal 128-blocks, and the kept part does not differ by a bit from the lower = 0 run"""
    d = twin.lower_case(n, lower)
    got, written = run_case(ctx, d, np.random.default_rng(400 + n))          # the same operands for every `lower` of a shape
    W = twin.view(written, d, "C")
    i, j = np.indices((n, n), sparse=True)
    if lower:
        sh = lower - 1
        assert W[(i + sh) // 128 >= (j + sh) // 128].all(), "a tile of the lower triangle or of a diagonal 128-block was skipped"
        assert not W.all(), "nothing was skipped"
    else:
        assert W.all()
        _LOWER_KEPT[n] = got
    if lower == 65:
        if n not in _LOWER_KEPT:
            _LOWER_KEPT[n] = run_case(ctx, twin.lower_case(n, 0), np.random.default_rng(400 + n))[0]
        assert (bits(got)[written] == bits(_LOWER_KEPT[n])[written]).all()


# ------------------------------------------------------------------ 64 x 64 kernel
@pytest.mark.parametrize("ta,tb", twin.TT, ids=TT_IDS)
def test_k64_small_shapes_exact(ctx, ta, tb):
    """k_dgemm<ta, tb, false>: one tile, ragged tiles, a single row and a single column, several tiles; reductions of 0, less than an
    MFMA step, less than a stage, a stage plus a rest, with a second product on some; K = K2 = 0 gives beta C"""
    rng = np.random.default_rng(500 + 2 * ta + tb)
    for d in twin.k64_cases(ta, tb):
        run_case(ctx, d, rng)


# ------------------------------------------------------------------ cut and skip
CUT_LEGS = [(cut, 0) for cut in twin.CUT_VALUES] + [(cut, 1) for cut in twin.CUT_VALUES if cut & 6]     # bits 1 and 2 leave operand elements unread


@pytest.mark.parametrize("cut,poison", CUT_LEGS, ids=["cut%d%s" % (c, "-poison" if p else "") for c, p in CUT_LEGS])
def test_cut_ranges_per_tile_exact(ctx, cut, poison):
    """k_dgemm<false, tb, true>: per 64 x 64 tile the reduction range of the twin, the tiles bit 0 skips untouched; cut = 0 runs with
    a skip pointer whose flag is down.  Poison leg: NaN in every operand element the cuts say is not read -- the result stays exact
    and finite (run_case asserts both)."""
    rng = np.random.default_rng(600 + 10 * cut + poison)
    for d in twin.cut_cases(cut, poison):
        got, written = run_case(ctx, d, rng)
        if cut & 1 and d["N"] > 64:
            assert not twin.view(written, d, "C")[:64, 64:].any()


@pytest.mark.parametrize("poison", [0, 1], ids=["plain", "poison"])
def test_products_of_the_wide_cholesky_exact(ctx, poison):
    """the shapes cw_gemm issues for k = 200: row panel, trailing update (bit 0), the two back-substitution products, R Rtot (7)"""
    rng = np.random.default_rng(700 + poison)
    for d in twin.cw_cases(poison=poison):
        run_case(ctx, d, rng)


def test_raised_skip_flag_writes_nothing(ctx):
    """flag up: the whole C allocation comes back bit-identical, on a small shape and on one of pipelined size; launch() has asserted
    that both ran the CUT kernel"""
    rng = np.random.default_rng(800)
    for d in twin.skip_up_cases():
        got, written = run_case(ctx, d, rng)
        assert not written.any() and twin.route(d)["kernel"] == twin.K64_CUT
        down = dict(d, skip=twin.SKIP_DOWN, name=d["name"] + "-down")
        got, written = run_case(ctx, down, rng)                       # flag down: the ordinary result
        assert written.any()


def test_cut_with_transposed_a_or_second_product_is_refused(ctx):
    rng = np.random.default_rng(810)
    for d in twin.cut_refusals():
        run_refusal(ctx, d, rng, twin.ERR_CUT)
    run_case(ctx, twin.cut_cases(3)[0], rng)


# ------------------------------------------------------------------ HFMI_EIG_GEMM=0
def child_main():
    """the switch is read once per process: this runs in a fresh interpreter with HFMI_EIG_GEMM=0"""
    ctx = hf.Context.default()
    for i, d in enumerate(twin.gemm0_cases()):
        route = twin.route(d, 0)
        assert route["kernel"] == twin.K64
        got, written = run_case(ctx, d, np.random.default_rng(900 + i), pipelined=0)
        assert written[twin.view(np.arange(written.size), d, "C")].all()       # `lower` is ignored: every tile is computed
    print("child ok")


_CHILD = "import sys; sys.path.insert(0, %r); import test_gpu_dgemm_descriptor as t; t.child_main()"


def test_switch_off_runs_the_64_tile_kernel_everywhere(ctx):
    """HFMI_EIG_GEMM=0: one case each of the 128-tile list, the batch list and the lower list runs the 64 x 64 kernel (the route says
    so), exactly; `lower` is ignored there, so every tile is computed"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD % here], env=dict(os.environ, HFMI_EIG_GEMM="0"), capture_output=True, text=True,
                       timeout=300, cwd=os.path.dirname(here))
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ rounding leg
@pytest.mark.parametrize("i", range(3), ids=[c["name"] for c in twin.rounding_cases()])
def test_rounding_against_long_double(ctx, i):
    """Gaussian operands, alpha = -0.7, beta = 1.3: |C - long-double reference| <= (K + K2 + 2) 2^-53 (|alpha| (|op A||op B| +
    |op A2||op B2|) + |beta C0|) elementwise -- the bound of any summation order of correctly rounded or fused operations"""
    d = twin.rounding_cases()[i]
    rng = np.random.default_rng(1000 + i)
    ops = twin.fill_operands(d, rng, gaussian=True)
    got, route, status = launch(ctx, d, ops)
    assert status == HFMI_OK
    ref, written = twin.reference(d, route, *ops, dtype=np.longdouble)
    bound = twin.rounding_bound(d, route, *ops)
    err = np.abs(twin.view(got, d, "C").astype(np.longdouble) - twin.view(ref, d, "C"))
    worst = float((err / bound).max())
    print("%s: largest error / bound = %.3f" % (d["name"], worst))
    assert written[twin.view(np.arange(written.size), d, "C")].all()
    assert (err <= bound).all(), "%s: %d entries over the bound, worst %.3f of it" % (d["name"], int((err > bound).sum()), worst)
    assert (bits(got)[~written] == bits(ops[4])[~written]).all()
