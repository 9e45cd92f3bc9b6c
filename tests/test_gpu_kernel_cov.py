"""GPU suite of the matrix-free kernel covariance operator (hfmi_op_kernel_cov / KernelCovarianceOperator, hfmi_kcov.hip): the apply
against the dense host evaluation under the worst-case bound of a length-N fp64 sum, the block storage contract on views with guard
bands, determinism, 64-bit indexing at scale, equivalence of the KLE with the explicit-matrix path, config 2's miniature, and the
argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402
from hippyflow_amd import workloads               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PANEL = 144                                       # columns per launch (KC_MAXT tiles of 16, hfmi_kcov.hip)


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def scattered(N, d, seed):
    """seeded points in the unit cube, two of them coincident"""
    pts = np.random.default_rng(seed).random((N, d))
    if N > 3:
        pts[N - 1] = pts[1]
    return pts


def within_bound(Y, Y_ref, N, absCW):
    """entrywise |Y - Y_ref| <= 8 N eps (|C| |W|): the worst case of a length-N fp64 sum in any order, the 8 for the few-ulp
    difference between the device exp / sqrt and numpy's"""
    err, bound = np.abs(Y - Y_ref), 8 * N * EPS * absCW
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("kernel_cov: N=%d k=%d max err/bound = %.3g" % (N, Y.shape[1], worst))
    assert np.all(err <= bound), worst


# Every N of {1, 15, 31, 64, 65, 193, 1000} (below a slab; ragged row tile; chunk boundary 64 / 65; more than one workgroup and a ragged
# last chunk; many workgroups) and every nvec of {1, 5, 17, 74, 138} (one ragged tile; tile boundary; 5 and 9 tiles), one shape past the
# 144-column panel so that the panel loop runs twice; d, family, ell, nugget and accumulate rotate over the cases.
CASES = [
    # N, nvec, d, family, ell, nugget, accumulate
    (1, 1, 1, "matern12", 1.0, 0.3, 0),
    (1, 138, 3, "sqexp", 0.05, 0.0, 1),
    (15, 5, 2, "matern32", 0.05, 0.0, 0),
    (15, 17, 1, "matern52", 1.0, 0.3, 1),
    (31, 74, 3, "matern12", 0.05, 0.3, 0),
    (31, 1, 2, "sqexp", 1.0, 0.0, 1),
    (64, 17, 2, "matern52", 0.05, 0.0, 0),
    (64, 138, 1, "matern32", 1.0, 0.3, 1),
    (65, 5, 3, "matern32", 1.0, 0.3, 0),
    (65, 74, 2, "matern12", 0.05, 0.0, 1),
    (193, 138, 2, "matern52", 0.05, 0.3, 0),
    (193, 1, 3, "sqexp", 0.05, 0.3, 1),
    (193, 17, 1, "sqexp", 1.0, 0.0, 0),
    (1000, 74, 3, "matern32", 0.05, 0.0, 0),
    (1000, 5, 2, "matern12", 1.0, 0.3, 1),
    (1000, 138, 1, "matern52", 0.05, 0.0, 1),
    (40, PANEL + 6, 2, "matern32", 1.0, 0.3, 0),
    (129, 2 * PANEL + 1, 3, "matern52", 0.05, 0.0, 1),
]


@pytest.mark.parametrize("N,nvec,d,family,ell,nugget,accumulate", CASES)
def test_apply_against_host(ctx, N, nvec, d, family, ell, nugget, accumulate):
    sigma = 1.3
    rng = np.random.default_rng(1000 * N + nvec)
    pts = scattered(N, d, seed=N + d)
    Cm = hf.kernel_cov_host(pts, family, sigma, ell, nugget)
    op = hf.KernelCovarianceOperator(pts, family=family, sigma=sigma, ell=ell, nugget=nugget, ctx=ctx)
    assert op.shape == (N, N)
    W = rng.standard_normal((N, nvec))
    Wd, Yd = hf.MultiVector.from_dense(W, ctx=ctx), hf.MultiVector(N, nvec, ctx=ctx)
    op.matMvMult(Wd, Yd)
    absCW = np.abs(Cm) @ np.abs(W)
    if not accumulate:
        within_bound(Yd.to_dense(), Cm @ W, N, absCW)
        return
    # Y = C W already (its own bound above); add C W2 into it: the issue's bound for each of the two sums, whose slack (the
    # worst case of an N-term sum is (N - 1) eps of 8 N eps) holds the one rounding of the final add
    W2 = rng.standard_normal((N, nvec))
    op.matMvMult(hf.MultiVector.from_dense(W2, ctx=ctx), Yd, accumulate=True)
    within_bound(Yd.to_dense(), Cm @ W + Cm @ W2, N, absCW + np.abs(Cm) @ np.abs(W2))


def test_vector_protocol(ctx):
    """mult / init_vector / shape as every DeviceOperator"""
    N = 77
    pts = scattered(N, 2, seed=5)
    op = hf.KernelCovarianceOperator(pts, ell=0.4, ctx=ctx)
    x, y = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    op.init_vector(x, 1)
    op.init_vector(y, 0)
    xh = np.random.default_rng(3).standard_normal(N)
    x.set_local(xh)
    op.mult(x, y)
    Cm = hf.kernel_cov_host(pts, "matern32", 1.0, 0.4)
    within_bound(y.get_local()[:, None], (Cm @ xh)[:, None], N, (np.abs(Cm) @ np.abs(xh))[:, None])
    assert hf.as_device_operator(op) is op


@pytest.mark.parametrize("N", [64, 65, 95])          # N % 32 in {0, 1, 31}
@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
def test_block_contract(ctx, N, layout):
    """W and Y views inside wider parents with guard columns: padding rows of Y stay +0.0, nothing outside Y's window changes.
    'wrapped': two NaN-filled parents with ld = round_up(N, 32) + 32; 'adjacent': one library parent, Y's window right after W's."""
    k, guard = 17, 2
    rng = np.random.default_rng(N)
    pts = scattered(N, 2, seed=N)
    op = hf.KernelCovarianceOperator(pts, family="matern52", sigma=1.1, ell=0.2, nugget=0.1, ctx=ctx)
    if layout == "wrapped":
        aw = ba.Arena.wrapped(ctx, N, k + 2 * guard, ld=ba.round_up(N, 32) + 32)
        ay = ba.Arena.wrapped(ctx, N, k + 2 * guard, ld=ba.round_up(N, 32) + 32)
        w, y = aw.window(guard, k), ay.window(guard, k)
        arenas = [aw, ay]
    else:
        a = ba.Arena.in_parent(ctx, N, 2 * k + 2 * guard)
        w, y = a.window(guard, k), a.window(guard + k, k)
        arenas = [a]
    W, Y0 = rng.standard_normal((N, k)), rng.standard_normal((N, k))
    for win, data in ((w, W), (y, Y0)):
        L.call("hfmi_block_upload", win.mv.handle, L.ptr(L.as_f64(data)), L.LAYOUT_DENSE)
    Cm = hf.kernel_cov_host(pts, "matern52", 1.1, 0.2, 0.1)
    absCW = np.abs(Cm) @ np.abs(W)
    for accumulate in (False, True):
        for a in arenas:
            a.snapshot()
        op.matMvMult(w.mv, y.mv, accumulate=accumulate)
        for a in arenas:
            a.check(written=[y] if y.arena is a else [], what="hfmi_op_apply(kernel_cov) accumulate=%d [%s]" % (accumulate, layout))
        # overwrite: C W; then accumulate on top of it: 2 C W (the doubling is exact)
        within_bound(y.mv.to_dense(), (2.0 if accumulate else 1.0) * (Cm @ W), N, (2.0 if accumulate else 1.0) * absCW)


def test_two_applies_are_bit_identical(ctx):
    N, k = 700, 74
    pts = scattered(N, 3, seed=11)
    W = hf.MultiVector.from_dense(np.random.default_rng(4).standard_normal((N, k)), ctx=ctx)
    op = hf.KernelCovarianceOperator(pts, family="matern32", ell=0.2, ctx=ctx)
    Y1, Y2 = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    op.matMvMult(W, Y1)
    op.matMvMult(W, Y2)
    a, b = Y1.to_dense(), Y2.to_dense()
    assert np.array_equal(a, b) and np.all(np.isfinite(a)) and np.abs(a).max() > 0


@pytest.mark.parametrize("N,k", [(20000, 16), (140000, 1)])
def test_scale_and_indexing(ctx, N, k):
    """Many workgroups and 64-bit row offsets; 64 seeded rows against the host.  N = 140000 is 1094 row tiles: more than the 4 resident
    workgroups per compute unit a 256-CU device can hold, so the grid-stride loop takes a second tile whatever the occupancy."""
    rng = np.random.default_rng(8)
    pts = scattered(N, 2, seed=8)
    W = rng.standard_normal((N, k))
    op = hf.KernelCovarianceOperator(pts, family="matern32", sigma=0.9, ell=0.1, nugget=0.2, ctx=ctx)
    Y = hf.MultiVector(N, k, ctx=ctx)
    op.matMvMult(hf.MultiVector.from_dense(W, ctx=ctx), Y)
    rows = np.sort(np.concatenate([[0, N - 1, N - 33], rng.choice(N, 61, replace=False)]))
    Cr = hf.kernel_cov_host(pts, "matern32", 0.9, 0.1, 0.2, rows=rows)
    within_bound(Y.to_dense()[rows], Cr @ W, N, np.abs(Cr) @ np.abs(W))


class _Prior:
    pass


def test_kle_equivalence_with_the_explicit_matrix(ctx):
    """M C M u = lambda M u at N = 1500 scattered 2-D points, M a positive diagonal: the matrix-free covariance and the explicit one give
    the same KLE (only the summation order of C W differs), through KLEProjector (fused solve) and through the generic doublePassG."""
    N, r, p = 1500, 20, 10
    rng = np.random.default_rng(21)
    pts = scattered(N, 2, seed=21)
    # Matern-5/2 with ell = 1: the residual bound below is about the randomized pass, not about C W -- with r + p = 30 probes and one
    # pass it needs lambda_31 / lambda_1 well under 1e-4 (6e-6 here; the CPU oracle's double pass on this pencil leaves 3e-5)
    family, sigma, ell = "matern52", 1.0, 1.0
    Cm = hf.kernel_cov_host(pts, family, sigma, ell)
    mdiag = (0.5 + rng.random(N)) / N
    M = sp.diags(mdiag).tocsr()
    MCM = mdiag[:, None] * Cm * mdiag[None, :]

    def check_invariants(d, V, E=None):
        assert np.abs(V.T @ (M @ V) - np.eye(r)).max() < 1e-10                              # test_KLEProjector.py:96-99
        if E is not None:
            assert np.linalg.norm(E - M @ V) / np.linalg.norm(M @ V) < 1e-10
        res = np.linalg.norm(MCM @ V - (M @ V) * d) / np.linalg.norm(MCM @ V)               # :110-129
        print("kle equivalence: residual %.3g" % res)
        assert res < 1e-4

    results = {}
    for name, make_C in (("matrix_free", lambda: hf.KernelCovarianceOperator(pts, family=family, sigma=sigma, ell=ell, ctx=ctx)),
                         ("explicit", lambda: hf.npToDeviceOperator(Cm, ctx=ctx))):
        prior = _Prior()
        prior.M, prior.C = M, make_C()
        params = hf.KLEParameterList()
        params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = r, p, False, False
        hf.parRandom.reseed(7)
        kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
        d, dec, enc = kle.construct_input_subspace("mass")
        check_invariants(np.asarray(d), dec.to_dense(), enc.to_dense())
        results[name, "fused"] = np.asarray(d)
        # the generic route: the same operators and the same Omega, one library call per step
        hf.parRandom.reseed(7)
        Omega = hf.MultiVector(N, r + p, ctx=ctx)
        hf.parRandom.normal(1.0, Omega)
        A = hf.MassPreconditionedCovarianceOperator(kle.C, kle.M)
        d2, U2 = hf.doublePassG(A, kle.M, hf.CsrPCGSolver(kle.M.csr, ctx=ctx), Omega, r, s=1, fused=False)
        check_invariants(np.asarray(d2), U2.to_dense())
        results[name, "generic"] = np.asarray(d2)
    for route in ("fused", "generic"):
        d_free, d_expl = results["matrix_free", route], results["explicit", route]
        gap = np.abs(d_free - d_expl).max() / d_expl[0]
        print("kle equivalence [%s]: max |delta d| / d_0 = %.3g" % (route, gap))
        assert gap <= 1e-10


def test_grid_parity_with_config2_miniature(ctx):
    """kle_kernel_workload on the fixture's 4000 nodes of a 64 x 63 grid: the leading eigenvalues against matern_d_exact, with the
    tolerances of test_gpu_configs_r2.py::test_matern_miniature_kle (same probe block, rank and passes)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "independent_eig.npz"))
    nx, ny, N = int(g["matern_nx"]), int(g["matern_ny"]), int(g["matern_N"])
    wl = workloads.kle_kernel_workload(nx, ny, N=N, sigma=float(g["matern_sigma"]), ell=float(g["matern_ell"]), ctx=ctx)
    Omega_h = np.asfortranarray(np.random.default_rng(2).standard_normal((N, 30)))
    A = hf.MassPreconditionedCovarianceOperator(wl.C_operator, wl.M_operator)
    d, U = hf.doublePassG(A, wl.M_operator, hf.CsrPCGSolver(wl.M_operator.csr), hf.MultiVector.from_dense(Omega_h, ctx=ctx), 20, s=1)
    exact = g["matern_d_exact"]
    assert np.all(d <= exact[:20] * (1 + 1e-10))
    np.testing.assert_allclose(d[:5], exact[:5], rtol=0.1)
    Ud = U.to_dense()
    assert np.abs(Ud.T @ (wl.M @ Ud) - np.eye(20)).max() < 1e-10


def test_invalid_arguments(ctx):
    lib = L.load()
    pts = L.as_f64(scattered(10, 2, seed=1))

    def create(points, N, d, family, sigma, ell, nugget):
        out = C.c_void_p()
        rc = lib.hfmi_op_kernel_cov(ctx.handle, points, N, d, family, sigma, ell, nugget, C.byref(out))
        return rc, out

    bad = {"d = 0": (L.ptr(pts), 10, 0, 1, 1.0, 0.1, 0.0), "d = 4": (L.ptr(pts), 5, 4, 1, 1.0, 0.1, 0.0),
           "ell = 0": (L.ptr(pts), 10, 2, 1, 1.0, 0.0, 0.0), "ell < 0": (L.ptr(pts), 10, 2, 1, 1.0, -0.1, 0.0),
           "nugget < 0": (L.ptr(pts), 10, 2, 1, 1.0, 0.1, -1e-3), "family = 4": (L.ptr(pts), 10, 2, 4, 1.0, 0.1, 0.0),
           "family = -1": (L.ptr(pts), 10, 2, -1, 1.0, 0.1, 0.0), "N = 0": (L.ptr(pts), 0, 2, 1, 1.0, 0.1, 0.0),
           "no points": (None, 10, 2, 1, 1.0, 0.1, 0.0)}
    for what, args in bad.items():
        rc, out = create(*args)
        assert rc == -1 and not out.value, what                                  # HFMI_ERR_INVALID, nothing created
        assert lib.hfmi_last_error().decode(), what
    with pytest.raises(ValueError):
        hf.KernelCovarianceOperator(pts, family="matern72", ctx=ctx)
    # a block of another length at apply: refused before any launch, Y untouched
    op = hf.KernelCovarianceOperator(pts, ctx=ctx)
    Y0 = np.random.default_rng(2).standard_normal((12, 3))
    W, Y = hf.MultiVector.from_dense(np.ones((12, 3)), ctx=ctx), hf.MultiVector.from_dense(Y0, ctx=ctx)
    with pytest.raises(hf.HfmiError) as e:
        op.matMvMult(W, Y)
    assert e.value.code == -1 and "length" in str(e.value)
    assert np.array_equal(Y.to_dense(), Y0)
