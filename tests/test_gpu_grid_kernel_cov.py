"""GPU suite of the kernel covariance on a regular grid applied by FFT (hfmi_op_kernel_cov_grid / GridKernelCovarianceOperator,
hfmi_fftcov.hip): the apply against the dense host covariance under Higham's FFT bound plus the reference's own summation bound, the
block storage contract on views with guard bands, bit-identical applies whatever the pairs per chunk, the vector protocol, equivalence of
the KLE with the matrix-free operator, config 2's miniature, and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402
import fftcov_twin as tw                          # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402
from hippyflow_amd import workloads               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SIGMA = 1.3
CASES = tw.cases()


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def within_bound(what, Y, Y_ref, bound):
    """per column ||Y_j - Yref_j||_2 <= bound_j; prints the worst ratio"""
    ratio = np.linalg.norm(Y - Y_ref, axis=0) / np.maximum(bound, 1e-300)
    print("grid_kernel_cov %s: N=%d k=%d worst err/bound = %.3g" % (what, Y.shape[0], Y.shape[1], ratio.max()))
    assert np.all(np.isfinite(Y)) and ratio.max() <= 1.0, float(ratio.max())


# ---------------------------------------------------------------------------------------------------------------- 1. apply against the host
@pytest.mark.parametrize("cid,shape,spacing,kind,nvec,family,ell,nugget,accumulate", CASES, ids=[c[0] for c in CASES])
def test_apply_against_host(ctx, cid, shape, spacing, kind, nvec, family, ell, nugget, accumulate):
    """Per column ||Y_j - Yref_j||_2 <= 32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W_j||_2 + 8 N eps || |C| |W_j| ||_2 with
    Yref = kernel_cov_host(points) @ W; an accumulating case is the sum of both applies' bounds.  Up to 4096 points Yref is the whole
    product.  Beyond (the three (300, 200) cases: 29 GB and half a minute of host time each) Yref is evaluated on 514 seeded rows and the
    bound is asserted on those rows; the whole columns are then held to the numpy twin (tests/helpers/fftcov_twin.py, itself under this
    bound on the host) within twice the FFT term, which both are within of the truth."""
    nodes = tw.nodes_of(shape, kind)
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=SIGMA, ell=ell, nugget=nugget, nodes=nodes, ctx=ctx)
    pts = tw.points(shape, spacing, nodes)
    N = pts.shape[0]
    assert op.shape == (N, N) and op.grid_shape == tuple(shape) and np.array_equal(op.points, pts)
    rng = np.random.default_rng(1000 + N + nvec)
    rows = tw.reference_rows(N)
    sel = slice(None) if rows is None else rows
    Ws = [rng.standard_normal((N, nvec)) for _ in range(2 if accumulate else 1)]
    Yd = hf.MultiVector(N, nvec, ctx=ctx)
    ref, bound, twin, twin_bound = 0.0, 0.0, 0.0, 0.0
    for i, W in enumerate(Ws):
        op.matMvMult(hf.MultiVector.from_dense(W, ctx=ctx), Yd, accumulate=i > 0)
        CW, absCW = tw.host_products(hf, pts, family, SIGMA, ell, nugget, W, rows=rows)
        ref = ref + CW
        bound = bound + tw.column_bounds(shape, spacing, family, SIGMA, ell, nugget, W, absCW)
        if rows is not None:
            twin = twin + tw.apply(shape, spacing, family, SIGMA, ell, nugget, W, nodes)
            twin_bound = twin_bound + 2.0 * tw.column_bounds(shape, spacing, family, SIGMA, ell, nugget, W, np.zeros((1, nvec)))
    Y = Yd.to_dense()
    within_bound(cid, Y[sel], ref, bound)
    if rows is not None:
        within_bound(cid + " (whole columns against the twin)", Y, twin, twin_bound)


# ---------------------------------------------------------------------------------------------------------------- 2. block contract
@pytest.mark.parametrize("shape", [(8, 8), (13, 5), (19, 5)])          # N = 64, 65, 95: N % 32 in {0, 1, 31}
@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
def test_block_contract(ctx, shape, layout):
    """W and Y views inside wider parents with guard columns: padding rows of Y stay +0.0, nothing outside Y's window changes.
    'wrapped': two NaN-filled parents with ld = round_up(N, 32) + 32; 'adjacent': one library parent, Y's window right after W's."""
    k, guard = 17, 2
    N = shape[0] * shape[1]
    spacing, family, ell, nugget = (0.05, 0.08), "matern52", 0.2, 0.1
    rng = np.random.default_rng(N)
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.1, ell=ell, nugget=nugget, ctx=ctx)
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
    CW, absCW = tw.host_products(hf, op.points, family, 1.1, ell, nugget, W)
    bound = tw.column_bounds(shape, spacing, family, 1.1, ell, nugget, W, absCW)
    for accumulate in (False, True):
        for a in arenas:
            a.snapshot()
        op.matMvMult(w.mv, y.mv, accumulate=accumulate)
        for a in arenas:
            a.check(written=[y] if y.arena is a else [], what="hfmi_op_apply(kernel_cov_grid) accumulate=%d [%s]" % (accumulate, layout))
        # overwrite: C W; then accumulate on top of it: 2 C W (the doubling is exact)
        f = 2.0 if accumulate else 1.0
        within_bound("contract %s acc=%d" % (layout, accumulate), y.mv.to_dense(), f * CW, f * bound)


# ---------------------------------------------------------------------------------------------------------------- 3. bit-identical applies
def test_applies_are_bit_identical_whatever_the_chunking(ctx):
    shape, k = (64, 40), 17
    nodes = tw.nodes_of(shape, "subset")
    N = nodes.size
    W = hf.MultiVector.from_dense(np.random.default_rng(4).standard_normal((N, k)), ctx=ctx)
    op = hf.GridKernelCovarianceOperator(shape, (0.013, 0.021), family="matern32", ell=0.2, nugget=0.1, nodes=nodes, ctx=ctx)
    Y1, Y2 = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    op.matMvMult(W, Y1)
    op.matMvMult(W, Y2)
    a = Y1.to_dense()
    assert np.array_equal(a, Y2.to_dense()) and np.all(np.isfinite(a)) and np.abs(a).max() > 0
    try:
        for pairs in (1, 3, 0):
            L.call("hfmi_tuning_set", b"fftcov_pairs", pairs)
            Y = hf.MultiVector(N, k, ctx=ctx)
            op.matMvMult(W, Y)
            assert np.array_equal(a, Y.to_dense()), pairs
    finally:
        L.call("hfmi_tuning_set", b"fftcov_pairs", 0)


# ---------------------------------------------------------------------------------------------------------------- 4. vector protocol
def test_vector_protocol(ctx):
    """mult / init_vector / shape as every DeviceOperator"""
    shape, spacing = (11, 7), (0.1, 0.07)
    N = 77
    op = hf.GridKernelCovarianceOperator(shape, spacing, ell=0.4, ctx=ctx)
    x, y = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    op.init_vector(x, 1)
    op.init_vector(y, 0)
    xh = np.random.default_rng(3).standard_normal(N)
    x.set_local(xh)
    op.mult(x, y)
    CW, absCW = tw.host_products(hf, op.points, "matern32", 1.0, 0.4, 0.0, xh[:, None])
    within_bound("mult", y.get_local()[:, None], CW, tw.column_bounds(shape, spacing, "matern32", 1.0, 0.4, 0.0, xh[:, None], absCW))
    assert hf.as_device_operator(op) is op
    assert np.array_equal(op.to_dense(), hf.kernel_cov_host(op.points, "matern32", 1.0, 0.4))
    mf = op.matrix_free()
    assert isinstance(mf, hf.KernelCovarianceOperator) and not isinstance(op, hf.KernelCovarianceOperator) and np.array_equal(mf.points, op.points)


# ---------------------------------------------------------------------------------------------------------------- 5. KLE equivalence
class _Prior:
    pass


def test_kle_equivalence_with_the_matrix_free_operator(ctx):
    """M C M u = lambda M u on a 48 x 31 grid, M a positive diagonal: the FFT operator and its matrix-free form give the same KLE (only
    the rounding of C W differs), through KLEProjector (fused solve) and through the generic doublePassG; extend at the operator's own
    nodes reproduces the decoder (the bound of test_gpu_kernel_cross_cov.py::test_projector_extend_reproduces_its_decoder)."""
    shape, spacing, r, p = (48, 31), (1.0 / 47, 1.0 / 30), 20, 10
    N = shape[0] * shape[1]
    rng = np.random.default_rng(21)
    family, sigma, ell = "matern52", 1.0, 1.0
    grid_op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=sigma, ell=ell, ctx=ctx)
    pts = grid_op.points
    Cm = hf.kernel_cov_host(pts, family, sigma, ell)
    mdiag = (0.5 + rng.random(N)) / N
    M = sp.diags(mdiag).tocsr()
    MCM = mdiag[:, None] * Cm * mdiag[None, :]

    def check_invariants(d, V, E=None):
        assert np.abs(V.T @ (M @ V) - np.eye(r)).max() < 1e-10
        if E is not None:
            assert np.linalg.norm(E - M @ V) / np.linalg.norm(M @ V) < 1e-10
        res = np.linalg.norm(MCM @ V - (M @ V) * d) / np.linalg.norm(MCM @ V)
        print("grid kle equivalence: residual %.3g" % res)
        assert res < 1e-4

    results = {}
    for name, C_op in (("grid", grid_op), ("matrix_free", grid_op.matrix_free())):
        prior = _Prior()
        prior.M, prior.C = M, C_op
        params = hf.KLEParameterList()
        params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = r, p, False, False
        hf.parRandom.reseed(7)
        kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
        assert kle.C is C_op and kle._covariance() is C_op                      # taken as it is, never sharded
        d, dec, enc = kle.construct_input_subspace("mass")
        d, dec_h, enc_h = np.asarray(d), dec.to_dense(), enc.to_dense()
        check_invariants(d, dec_h, enc_h)
        results[name, "fused"] = d
        hf.parRandom.reseed(7)
        Omega = hf.MultiVector(N, r + p, ctx=ctx)
        hf.parRandom.normal(1.0, Omega)
        A = hf.MassPreconditionedCovarianceOperator(kle.C, kle.M)
        d2, U2 = hf.doublePassG(A, kle.M, hf.CsrPCGSolver(kle.M.csr, ctx=ctx), Omega, r, s=1, fused=False)
        check_invariants(np.asarray(d2), U2.to_dense())
        results[name, "generic"] = np.asarray(d2)
        # the Nystrom extension at the operator's own nodes
        resid = np.linalg.norm(Cm @ enc_h - dec_h * d)
        tol = resid / d[-1] + 8 * N * EPS * (np.abs(Cm) @ np.abs(enc_h)) / d
        err = np.abs(kle.extend(pts).to_dense() - dec_h)
        print("grid kle extend [%s]: ||R||_F / lambda_r = %.3g, max err/tol = %.3g" % (name, resid / d[-1], (err / tol).max()))
        assert np.all(err <= tol)
    for route in ("fused", "generic"):
        d_grid, d_free = results["grid", route], results["matrix_free", route]
        gap = np.abs(d_grid - d_free).max() / d_free[0]
        print("grid kle equivalence [%s]: max |delta d| / d_0 = %.3g" % (route, gap))
        assert gap <= 1e-10


def test_kernel_factor_rank_goes_through_the_matrix_free_form(ctx):
    shape = (20, 15)
    grid_op = hf.GridKernelCovarianceOperator(shape, (1.0 / 19, 1.0 / 14), family="matern32", ell=0.5, ctx=ctx)
    prior = _Prior()
    prior.M, prior.C = sp.identity(300, format="csr") / 300.0, grid_op
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = 8, 4, False, False
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    kle.kernel_factor_rank = 60
    d, dec, enc = kle.construct_input_subspace("mass")
    exact = np.linalg.eigvalsh(hf.kernel_cov_host(grid_op.points, "matern32", 1.0, 0.5) / 300.0)[::-1][:8]
    d = np.asarray(d)
    # the factor's residual is positive semidefinite: its eigenvalues lie below the exact ones, and at rank 60 close to them
    assert kle.C is grid_op and np.all(d <= exact * (1 + 1e-10)) and np.all(d >= 0.99 * exact)


# ---------------------------------------------------------------------------------------------------------------- 6. config-2 miniature
def test_grid_parity_with_config2_miniature(ctx):
    """kle_grid_kernel_workload on the fixture's 4000 nodes of a 64 x 63 grid: the leading eigenvalues against matern_d_exact, with the
    assertions of test_gpu_kernel_cov.py::test_grid_parity_with_config2_miniature (same probe block, rank and passes)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "independent_eig.npz"))
    nx, ny, N = int(g["matern_nx"]), int(g["matern_ny"]), int(g["matern_N"])
    wl = workloads.kle_grid_kernel_workload(nx, ny, N=N, sigma=float(g["matern_sigma"]), ell=float(g["matern_ell"]), ctx=ctx)
    assert isinstance(wl.C_operator, hf.GridKernelCovarianceOperator) and wl.C_operator.shape == (N, N)
    assert np.abs(wl.C_operator.points - wl.points).max() <= 4 * EPS
    Omega_h = np.asfortranarray(np.random.default_rng(2).standard_normal((N, 30)))
    A = hf.MassPreconditionedCovarianceOperator(wl.C_operator, wl.M_operator)
    d, U = hf.doublePassG(A, wl.M_operator, hf.CsrPCGSolver(wl.M_operator.csr), hf.MultiVector.from_dense(Omega_h, ctx=ctx), 20, s=1)
    exact = g["matern_d_exact"]
    assert np.all(d <= exact[:20] * (1 + 1e-10))
    np.testing.assert_allclose(d[:5], exact[:5], rtol=0.1)
    Ud = U.to_dense()
    assert np.abs(Ud.T @ (wl.M @ Ud) - np.eye(20)).max() < 1e-10


# ---------------------------------------------------------------------------------------------------------------- 7. invalid arguments
def test_invalid_arguments(ctx):
    lib = L.load()

    def create(d, n, h, nodes, N, family, sigma, ell, nugget):
        out = C.c_void_p()
        na = None if n is None else np.asarray(n, dtype=np.int64)
        ha = None if h is None else np.asarray(h, dtype=np.float64)
        ga = None if nodes is None else np.asarray(nodes, dtype=np.int64)
        rc = lib.hfmi_op_kernel_cov_grid(ctx.handle, d, None if na is None else L.ptr(na), None if ha is None else L.ptr(ha),
                                         None if ga is None else L.ptr(ga), N, family, sigma, ell, nugget, C.byref(out))
        return rc, out

    ok = dict(d=2, n=[5, 4], h=[0.1, 0.2], nodes=None, N=20, family=1, sigma=1.0, ell=0.1, nugget=0.0)
    rc, out = create(**ok)
    assert rc == 0 and out.value
    lib.hfmi_op_destroy(out)
    bad = {"d = 0": dict(d=0), "d = 4": dict(d=4, n=[2, 2, 2, 2], h=[1.0] * 4, N=16), "n = 0": dict(n=[5, 0], N=0), "n < 0": dict(n=[-5, 4]),
           "n > 2048": dict(n=[2049, 1], N=2049), "h = 0": dict(h=[0.1, 0.0]), "h < 0": dict(h=[-0.1, 0.2]), "h = inf": dict(h=[0.1, np.inf]),
           "h = nan": dict(h=[np.nan, 0.2]), "N = 0": dict(N=0, nodes=[0]), "N < 0": dict(N=-3), "node out of range": dict(nodes=[0, 20], N=2),
           "node negative": dict(nodes=[-1, 3], N=2), "node repeated": dict(nodes=[3, 7, 3], N=3), "NULL nodes, N != prod n": dict(N=19),
           "more points than nodes": dict(nodes=list(range(20)) + [0], N=21), "family = 4": dict(family=4), "family = -1": dict(family=-1),
           "ell = 0": dict(ell=0.0), "ell < 0": dict(ell=-0.1), "nugget < 0": dict(nugget=-1e-3), "no n": dict(n=None), "no h": dict(h=None)}
    for what, change in bad.items():
        rc, out = create(**dict(ok, **change))
        assert rc == -1 and not out.value, what                                  # HFMI_ERR_INVALID, nothing created
        assert lib.hfmi_last_error().decode(), what
    for kw in (dict(family="matern72"), dict(nodes=[3, 3]), dict(nodes=[0, 20]), dict(ell=0.0), dict(nugget=-1.0)):
        with pytest.raises(ValueError):
            hf.GridKernelCovarianceOperator((5, 4), (0.1, 0.2), ctx=ctx, **kw)
    with pytest.raises(ValueError):
        hf.GridKernelCovarianceOperator((5, 2049), (0.1, 0.2), ctx=ctx)
    # a block of another length at apply: refused before any launch, Y untouched
    op = hf.GridKernelCovarianceOperator((5, 2), (0.1, 0.2), ctx=ctx)
    Y0 = np.random.default_rng(2).standard_normal((12, 3))
    W, Y = hf.MultiVector.from_dense(np.ones((12, 3)), ctx=ctx), hf.MultiVector.from_dense(Y0, ctx=ctx)
    with pytest.raises(hf.HfmiError) as e:
        op.matMvMult(W, Y)
    assert e.value.code == -1 and "length" in str(e.value)
    assert np.array_equal(Y.to_dense(), Y0)
    # the pivoted Cholesky factorisation reads entries of C: not of this operator, in C or in Python
    f = C.c_void_p()
    assert lib.hfmi_pchol_create(op._op, 4, 0.0, C.byref(f)) == -1 and not f.value
    with pytest.raises(ValueError):
        hf.pivoted_cholesky(op, 4)
    assert hf.pivoted_cholesky(op.matrix_free(), 4).rank == 4
