"""GPU suite of the rectangular kernel covariance (hfmi_op_kernel_cross_cov / hfmi_op_kernel_cov_rows, the kcov_cross_params
instances of k_kcov in hfmi_kcov.hip): the apply against the dense host evaluation under the bound of tests/test_gpu_kernel_cov.py
(entrywise |Y - Y_ref| <= 8 N eps (|K| |W|), N the number of sources), the diagonal, row slabs against the square apply bit for bit, the
block storage contract, determinism, transpose, the Nystrom extension of exact eigenpairs and of the pivoted Cholesky factor, the
row-sharded operator in one process and over ranks sharing the GPU, and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402
from hippyflow_amd import workloads               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PANEL = 144                                       # columns per launch (KC_MAXT tiles of 16, hfmi_kcov.hip)
FAMILIES = ["matern12", "matern32", "matern52", "sqexp"]
WORKER = os.path.join(ROOT, "tests", "helpers", "gpu_kcov_shard_worker.py")


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


def within_bound(Y, Y_ref, N, absKW, what="kernel_cross_cov"):
    """entrywise |Y - Y_ref| <= 8 N eps (|K| |W|): the worst case of a length-N fp64 sum in any order, the 8 for the few-ulp
    difference between the device exp / sqrt and numpy's (the bound of tests/test_gpu_kernel_cov.py)"""
    err, bound = np.abs(Y - Y_ref), 8 * N * EPS * absKW
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s: M=%d N=%d k=%d max err/bound = %.3g" % (what, Y.shape[0], N, Y.shape[1], worst))
    assert np.all(err <= bound), worst


def apply(op, W, ctx, accumulate=False, Y=None):
    Wd = hf.MultiVector.from_dense(W, ctx=ctx)
    Yd = hf.MultiVector(op.shape[0], W.shape[1], ctx=ctx) if Y is None else Y
    op.matMvMult(Wd, Yd, accumulate=accumulate)
    return Yd


# ---------------------------------------------------------------------------------------------------------------- 1. apply
# M over {1, 15, 16, 129, 300} (one row; a ragged and a full wave tile; a second workgroup of one row; three workgroups, ragged) and N over
# {1, 3, 63, 64, 65, 193, 1000} (below a 4-source slab; around the 64-source chunk; several chunks, ragged), both M > N and M < N; nvec over
# {1, 17, 74, 138, 150} and one shape of two full panels and a column; d, family, ell and accumulate rotate.
CASES = [
    # M, N, nvec, d, family, ell, accumulate
    (1, 1, 1, 1, "matern12", 1.0, 0),
    (1, 1000, 17, 2, "matern32", 0.05, 1),
    (15, 3, 74, 3, "matern52", 1.0, 0),
    (15, 193, 138, 1, "sqexp", 0.05, 1),
    (16, 63, 150, 2, "matern12", 0.05, 0),
    (16, 64, 1, 3, "matern32", 1.0, 1),
    (129, 65, 17, 1, "matern52", 0.05, 0),
    (129, 1000, 74, 2, "sqexp", 1.0, 1),
    (300, 3, 138, 3, "matern12", 1.0, 0),
    (300, 193, 150, 1, "matern32", 0.05, 1),
    (300, 1000, 1, 2, "matern52", 1.0, 0),
    (129, 64, 138, 3, "sqexp", 0.05, 0),
    (16, 1, 74, 2, "matern32", 1.0, 1),
    (15, 65, 2 * PANEL + 1, 3, "matern52", 0.05, 0),
]


@pytest.mark.parametrize("M,N,nvec,d,family,ell,accumulate", CASES)
def test_apply_against_host(ctx, M, N, nvec, d, family, ell, accumulate):
    sigma = 1.3
    rng = np.random.default_rng(100000 * M + 100 * N + nvec)
    S, T = scattered(N, d, seed=N + d), scattered(M, d, seed=1000 + M + d)
    K = hf.kernel_cross_cov_host(T, S, family, sigma, ell)
    op = hf.KernelCrossCovarianceOperator(T, S, family=family, sigma=sigma, ell=ell, ctx=ctx)
    assert op.shape == (M, N) and np.array_equal(op.to_dense(), K)
    W = rng.standard_normal((N, nvec))
    Yd = apply(op, W, ctx)
    absKW = np.abs(K) @ np.abs(W)
    if not accumulate:
        within_bound(Yd.to_dense(), K @ W, N, absKW)
        return
    # Y = K W already; add K W2 into it: the bound for each of the two sums, whose slack holds the one rounding of the final add
    W2 = rng.standard_normal((N, nvec))
    apply(op, W2, ctx, accumulate=True, Y=Yd)
    within_bound(Yd.to_dense(), K @ W + K @ W2, N, absKW + np.abs(K) @ np.abs(W2))


def test_vector_protocol(ctx):
    """init_vector gives the lengths M (range) and N (domain); mult maps one to the other"""
    M, N = 21, 50
    S, T = scattered(N, 2, seed=1), scattered(M, 2, seed=2)
    op = hf.KernelCrossCovarianceOperator(T, S, ell=0.4, ctx=ctx)
    x, y = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    op.init_vector(y, 0)
    op.init_vector(x, 1)
    assert (y.size(), x.size()) == (M, N)
    xh = np.random.default_rng(3).standard_normal(N)
    x.set_local(xh)
    op.mult(x, y)
    K = op.to_dense()
    within_bound(y.get_local()[:, None], (K @ xh)[:, None], N, (np.abs(K) @ np.abs(xh))[:, None])


# ---------------------------------------------------------------------------------------------------------------- 2. diagonal
@pytest.mark.parametrize("N,row0,M", [(193, 37, 100), (65, 64, 1), (1000, 0, 1000)])
def test_diagonal_sits_on_the_index(ctx, N, row0, M):
    """targets = sources[row0 : row0 + M], nugget 0.3: it lands on source i + row0 and not on the coincident pair (1, N - 1)"""
    sigma, ell, nugget, k = 1.3, 0.2, 0.3, 17
    S = scattered(N, 2, seed=N)
    T = S[row0:row0 + M]
    K = hf.kernel_cross_cov_host(T, S, "matern32", sigma, ell, nugget, diag_offset=row0)
    assert np.array_equal(K, hf.kernel_cov_host(S, "matern32", sigma, ell, nugget, rows=range(row0, row0 + M)))
    op = hf.KernelCrossCovarianceOperator(T, S, "matern32", sigma, ell, nugget, diag_offset=row0, ctx=ctx)
    W = np.random.default_rng(N).standard_normal((N, k))
    within_bound(apply(op, W, ctx).to_dense(), K @ W, N, np.abs(K) @ np.abs(W), "diagonal")
    # the unit vectors of the coincident pair pick out columns 1 and N - 1: they differ by the nugget exactly where row i + row0 == column
    E = np.zeros((N, 2))
    E[1, 0] = E[N - 1, 1] = 1.0
    cols = apply(op, E, ctx).to_dense()
    assert np.array_equal(cols != 0, np.ones_like(cols, dtype=bool))
    diff = cols[:, 0] - cols[:, 1]
    for col, c in ((1, 0), (N - 1, 1)):
        i = col - row0
        if 0 <= i < M:
            assert abs(abs(diff[i]) - nugget) <= 4 * EPS * (sigma ** 2 + nugget)
            diff[i] = 0.0
    assert np.array_equal(diff, np.zeros(M))


# ---------------------------------------------------------------------------------------------------------------- 3. slabs
@pytest.mark.parametrize("N,k,cuts", [(333, 74, [0, 37, 37, 165, 333]), (1000, 17, [0, 128, 129, 1000]), (64, 138, [0, 64])])
def test_slabs_reproduce_the_full_apply_bit_for_bit(ctx, N, k, cuts):
    pts = scattered(N, 2, seed=N + k)
    full = hf.KernelCovarianceOperator(pts, family="matern52", sigma=1.1, ell=0.2, nugget=0.1, ctx=ctx)
    W = np.random.default_rng(k).standard_normal((N, k))
    Wd = hf.MultiVector.from_dense(W, ctx=ctx)
    Yf = hf.MultiVector(N, k, ctx=ctx)
    full.matMvMult(Wd, Yf)
    ref = Yf.to_dense()
    assert np.all(np.isfinite(ref)) and np.abs(ref).min() > 0
    slabs = [full.rows(r0, r1) for r0, r1 in zip(cuts, cuts[1:])]
    assert all(s.shape == (N, N) for s in slabs)
    # every slab accumulated into a zeroed Y: the full apply
    Ya = hf.MultiVector(N, k, ctx=ctx)
    Ya.zero()
    for s in slabs:
        s.matMvMult(Wd, Ya, accumulate=True)
    assert np.array_equal(Ya.to_dense(), ref)
    # overwrite, into a Y that holds something else: the slab's rows are the full apply's, every other row is exactly 0
    for s in slabs:
        Yo = hf.MultiVector.from_dense(np.full((N, k), 7.5), ctx=ctx)
        s.matMvMult(Wd, Yo)
        expect = np.zeros((N, k))
        expect[s.row0:s.row1] = ref[s.row0:s.row1]
        got = Yo.to_dense()
        assert np.array_equal(got, expect)
        assert not np.signbit(got[:s.row0]).any() and not np.signbit(got[s.row1:]).any()      # +0.0


# ---------------------------------------------------------------------------------------------------------------- 4. block contract
@pytest.mark.parametrize("which", ["slab", "cross"])
@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
def test_block_contract(ctx, which, layout):
    """W and Y views inside wider parents with guard columns: padding rows of Y stay +0.0, nothing outside Y's window changes, in both
    accumulate modes.  'wrapped': NaN-filled parents with ld = round_up(rows, 32) + 32; 'adjacent': library parents, Y's window right
    after W's in ONE parent for the slab; the cross operator's W and Y have different lengths, so each sits between guard columns
    of its own library parent."""
    k, guard, N = 17, 2, 95
    rng = np.random.default_rng(N)
    pts = scattered(N, 2, seed=N)
    if which == "slab":
        M, r0, r1 = N, 10, 70
        op = hf.KernelCovarianceOperator(pts, family="matern52", sigma=1.1, ell=0.2, nugget=0.1, ctx=ctx).rows(r0, r1)
        K = op.to_dense()
    else:
        M = 65
        op = hf.KernelCrossCovarianceOperator(scattered(M, 2, seed=M), pts, family="matern52", sigma=1.1, ell=0.2, ctx=ctx)
        K = op.to_dense()
    if layout == "wrapped":
        aw = ba.Arena.wrapped(ctx, N, k + 2 * guard, ld=ba.round_up(N, 32) + 32)
        ay = ba.Arena.wrapped(ctx, M, k + 2 * guard, ld=ba.round_up(M, 32) + 32)
        w, y = aw.window(guard, k), ay.window(guard, k)
        arenas = [aw, ay]
    elif which == "slab":
        a = ba.Arena.in_parent(ctx, N, 2 * k + 2 * guard)
        w, y = a.window(guard, k), a.window(guard + k, k)
        arenas = [a]
    else:
        aw, ay = ba.Arena.in_parent(ctx, N, k + 2 * guard), ba.Arena.in_parent(ctx, M, k + 2 * guard)
        w, y = aw.window(guard, k), ay.window(guard, k)
        arenas = [aw, ay]
    W, Y0 = rng.standard_normal((N, k)), rng.standard_normal((M, k))
    for win, data in ((w, W), (y, Y0)):
        L.call("hfmi_block_upload", win.mv.handle, L.ptr(L.as_f64(data)), L.LAYOUT_DENSE)
    absKW = np.abs(K) @ np.abs(W)
    for accumulate in (False, True):
        for a in arenas:
            a.snapshot()
        op.matMvMult(w.mv, y.mv, accumulate=accumulate)
        for a in arenas:
            a.check(written=[y] if y.arena is a else [], what="hfmi_op_apply(%s) accumulate=%d [%s]" % (which, accumulate, layout))
        # overwrite: K W (the slab's other rows 0); then accumulate on top of it: 2 K W (the doubling is exact)
        f = 2.0 if accumulate else 1.0
        got = y.mv.to_dense()
        within_bound(got, f * (K @ W), N, f * absKW, "block contract [%s]" % which)
        if which == "slab":
            assert np.array_equal(got[:r0], np.zeros((r0, k))) and np.array_equal(got[r1:], np.zeros((N - r1, k)))
    # an accumulating slab leaves the rows outside it alone
    if which == "slab":
        L.call("hfmi_block_upload", y.mv.handle, L.ptr(L.as_f64(Y0)), L.LAYOUT_DENSE)
        op.matMvMult(w.mv, y.mv, accumulate=True)
        got = y.mv.to_dense()
        assert np.array_equal(got[:r0], Y0[:r0]) and np.array_equal(got[r1:], Y0[r1:])


# ---------------------------------------------------------------------------------------------------------------- 5. determinism
def test_two_applies_are_bit_identical(ctx):
    M, N, k = 700, 500, 74
    op = hf.KernelCrossCovarianceOperator(scattered(M, 3, seed=12), scattered(N, 3, seed=11), family="matern32", ell=0.2, ctx=ctx)
    W = np.random.default_rng(4).standard_normal((N, k))
    a, b = apply(op, W, ctx).to_dense(), apply(op, W, ctx).to_dense()
    assert np.array_equal(a, b) and np.all(np.isfinite(a)) and np.abs(a).max() > 0


# ---------------------------------------------------------------------------------------------------------------- 6. transpose
def test_transpose(ctx):
    M, N, k = 129, 65, 17
    S, T = scattered(N, 3, seed=1), scattered(M, 3, seed=2)
    op = hf.KernelCrossCovarianceOperator(T, S, family="matern52", sigma=0.9, ell=0.3, ctx=ctx)
    opT = op.transpose()
    assert opT.shape == (N, M)
    Kt = hf.kernel_cross_cov_host(T, S, "matern52", 0.9, 0.3).T
    W = np.random.default_rng(5).standard_normal((M, k))
    within_bound(apply(opT, W, ctx).to_dense(), Kt @ W, M, np.abs(Kt) @ np.abs(W), "transpose")
    with_diag = hf.KernelCrossCovarianceOperator(S[3:10], S, family="matern52", ell=0.3, nugget=0.1, diag_offset=3, ctx=ctx)
    with pytest.raises(ValueError):
        with_diag.transpose()


# ---------------------------------------------------------------------------------------------------------------- 7. Nystrom
class _Prior:
    pass


GRID = 18
SIGMA, ELL = 1.3, 0.3


@pytest.fixture(scope="module")
def grid():
    N = GRID * GRID
    return {"N": N, "pts": workloads.grid_points(N, GRID, GRID), "M": workloads.grid_mass_matrix(GRID, GRID).tocsr(),
            "other": np.random.default_rng(31).random((150, 2))}


@pytest.mark.parametrize("orthogonality", ["identity", "mass"])
@pytest.mark.parametrize("family", FAMILIES)
def test_nystrom_on_exact_eigenpairs(ctx, grid, family, orthogonality):
    """The 12 leading eigenpairs of C v = lambda v ('identity') or M C M v = lambda M v, V^T M V = I ('mass') from scipy's dense
    eigensolver; encoder E = V or M V.  C E = V Lambda, so the extension to the source points reproduces V and the extension to other
    points is K(T, X) E / lambda: both within 8 N eps (|K| |E|) / lambda entrywise (the host evaluation of C E / lambda alone stays below
    0.031 of that bound on these inputs; the one rounding of the division sits in the same slack as the final add of an accumulate)."""
    N, pts, r = grid["N"], grid["pts"], 12
    Cm = hf.kernel_cov_host(pts, family, SIGMA, ELL)
    if orthogonality == "identity":
        lam, V = sla.eigh(Cm)
        E = V = V[:, ::-1][:, :r]
    else:
        Md = grid["M"].toarray()
        lam, V = sla.eigh(Md @ Cm @ Md, Md)
        V = V[:, ::-1][:, :r]
        E = Md @ V
    lam = lam[::-1][:r]
    Ed = hf.MultiVector.from_dense(E, ctx=ctx)
    own = hf.KernelCrossCovarianceOperator(pts, pts, family, SIGMA, ELL, ctx=ctx)
    ext = hf.nystrom_extend(own, Ed, lam)
    assert (ext.size(), ext.nvec()) == (N, r)
    within_bound(ext.to_dense(), V, N, (np.abs(Cm) @ np.abs(E)) / lam, "nystrom own [%s %s]" % (family, orthogonality))
    T = grid["other"]
    K = hf.kernel_cross_cov_host(T, pts, family, SIGMA, ELL)
    other = hf.nystrom_extend(hf.KernelCrossCovarianceOperator(T, pts, family, SIGMA, ELL, ctx=ctx), Ed, lam)
    within_bound(other.to_dense(), (K @ E) / lam, N, (np.abs(K) @ np.abs(E)) / lam, "nystrom other [%s %s]" % (family, orthogonality))


@pytest.mark.parametrize("orthogonality", ["identity", "mass"])
def test_projector_extend_reproduces_its_decoder(ctx, grid, orthogonality):
    """KLEProjector.extend at the projector's own nodes.  With R = C encoder - decoder Lambda the eigen-residual of the randomized solve
    (measured here with the host matrix), decoder - C encoder / d = -R / d entrywise, and |R_ij| / d_j <= ||R||_F / lambda_r; the device
    evaluation of C encoder / d adds the apply's bound.  So: |extend - decoder|_ij <= ||R||_F / lambda_r + 8 N eps (|C| |encoder|)_ij / d_j."""
    N, pts, r = grid["N"], grid["pts"], 12
    family = "sqexp"               # lambda_49 / lambda_12 = 1e-4 on this grid: 36 extra probes make the solve's residual small
    prior = _Prior()
    prior.M = grid["M"]
    prior.C = hf.KernelCovarianceOperator(pts, family=family, sigma=SIGMA, ell=ELL, ctx=ctx)
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = r, 36, False, False
    hf.parRandom.reseed(9)
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    with pytest.raises(ValueError):
        kle.extend(pts)                                            # no subspace yet
    d, dec, enc = kle.construct_input_subspace(orthogonality)
    d, dec_h, enc_h = np.asarray(d), dec.to_dense(), enc.to_dense()
    Cm = hf.kernel_cov_host(pts, family, SIGMA, ELL)
    resid = np.linalg.norm(Cm @ enc_h - dec_h * d)
    tol = resid / d[-1] + 8 * N * EPS * (np.abs(Cm) @ np.abs(enc_h)) / d
    err = np.abs(kle.extend(pts).to_dense() - dec_h)
    print("projector extend [%s]: ||R||_F / lambda_r = %.3g, max err = %.3g, max err/tol = %.3g"
          % (orthogonality, resid / d[-1], err.max(), (err / tol).max()))
    assert np.all(err <= tol)
    # other points: the host formula with the projector's own encoder
    T = grid["other"]
    K = hf.kernel_cross_cov_host(T, pts, family, SIGMA, ELL)
    within_bound(kle.extend(T).to_dense(), (K @ enc_h) / d, N, (np.abs(K) @ np.abs(enc_h)) / d, "projector extend other")


def test_projector_extend_refuses_what_it_cannot_extend(ctx, grid):
    N, pts = grid["N"], grid["pts"]
    prior = _Prior()
    prior.M = grid["M"]
    prior.C = hf.npToDeviceOperator(hf.kernel_cov_host(pts, "matern32", SIGMA, ELL), ctx=ctx)
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = 4, 4, False, False
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    kle.construct_input_subspace("identity")
    with pytest.raises(ValueError):
        kle.extend(pts)                                            # not a kernel covariance
    prior.C = hf.KernelCovarianceOperator(pts, family="matern32", sigma=SIGMA, ell=ELL, ctx=ctx)
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    kle.R_orthogonal, kle._kle_encoder, kle.d_KLE = True, object(), np.ones(4)     # the state 'prior' orthogonality leaves
    with pytest.raises(ValueError):
        kle.extend(pts)


# ---------------------------------------------------------------------------------------------------------------- 8. factor extension
@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(41)
    return {"pts": rng.random((400, 2)), "other": rng.random((150, 2))}


@pytest.mark.parametrize("family,max_rank", [(f, 40) for f in FAMILIES] + [("matern32", 100)])
def test_factor_extension(ctx, cloud, family, max_rank):
    """L* = K(points, X_P) L_P^-T against the same formula on the host from the device's pivots and L, within 8 k eps (|K(., X_P)|
    |L_P^-T|) (k = rank sources); at the operator's own points L* reproduces L within the same bound (the host pivoted Cholesky alone
    stays below 0.012 of it on these inputs).  sample_at(own points, xi) against sample's draws L xi: |L* - L| |xi| is bounded by that
    bound times |xi|, and each of the two small products L xi, L* xi is a length-k fp64 sum: k eps (|L| |xi|) apiece."""
    pts, other = cloud["pts"], cloud["other"]
    op = hf.KernelCovarianceOperator(pts, family=family, sigma=SIGMA, ell=ELL, ctx=ctx)
    f = hf.pivoted_cholesky(op, max_rank)
    k = f.rank
    assert k >= 1
    Lh = f.L.to_dense()
    LP = Lh[f.pivots, :]
    assert np.abs(np.triu(LP, 1)).max() <= 1e-12 * np.abs(LP).max()       # lower triangular in pivot order, up to rounding
    LPinvT = sla.solve_triangular(LP, np.eye(k), lower=True).T
    XP = pts[f.pivots]
    for T, ref_is_L in ((other, False), (pts, True)):
        K = hf.kernel_cross_cov_host(T, XP, family, SIGMA, ELL)
        ext = f.extend(T)
        assert (ext.size(), ext.nvec()) == (T.shape[0], k)
        absKL = np.abs(K) @ np.abs(LPinvT)
        within_bound(ext.to_dense(), K @ LPinvT, k, absKL, "factor extend [%s %d]" % (family, k))
        if ref_is_L:
            within_bound(ext.to_dense(), Lh, k, absKL, "factor extend own [%s %d]" % (family, k))
            own_bound = 8 * k * EPS * absKL
    X, xi = f.sample(5, seed=3)
    xih = xi.to_dense()
    Xs = f.sample_at(pts, xi).to_dense()
    err = np.abs(Xs - X.to_dense())
    bound = own_bound @ np.abs(xih) + 2 * k * EPS * (np.abs(Lh) @ np.abs(xih))
    print("factor sample_at [%s %d]: max err/bound = %.3g" % (family, k, float((err / bound).max())))
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------------------------- 9. sharded, one process
def test_sharded_in_one_process(ctx):
    N, k = 333, 12
    pts = scattered(N, 2, seed=17)
    full = hf.KernelCovarianceOperator(pts, family="matern32", sigma=1.3, ell=0.3, nugget=0.05, ctx=ctx)
    W = np.random.default_rng(3).standard_normal((N, k))
    ref = apply(full, W, ctx).to_dense()
    coll = hf.NativeCollective.from_unique_id(hf.NativeCollective.unique_id(), 1, 0, ctx=ctx)
    for collective in (hf.NullCollective(), coll):
        s = full.sharded(collective)
        assert isinstance(s, hf.DeviceOperator) and s.shape == (N, N) and (s.row0, s.row1) == (0, N) and s.collective is None
        assert np.array_equal(apply(s, W, ctx).to_dense(), ref)
    # the projector's switch on a one-rank collective: same d and decoder bits as without it
    prior = _Prior()
    prior.M, prior.C = workloads.grid_mass_matrix(19, 18)[:N, :N].tocsr(), full
    out = []
    for flag in (False, True):
        params = hf.KLEParameterList()
        params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = 8, 4, False, False
        hf.parRandom.reseed(7)
        kle = hf.KLEProjector(prior, collective=coll, parameters=params, ctx=ctx)
        assert kle.shard_kernel_covariance is False
        kle.shard_kernel_covariance = flag
        d, dec, _ = kle.construct_input_subspace("mass")
        out.append((np.asarray(d), dec.to_dense()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    coll.close()


class _SumOfTwo:
    """A collective that is neither Null nor Native: two 'ranks', the other one contributing the same block (allReduce doubles)."""

    def __init__(self, rank):
        self._rank, self.calls = rank, 0

    def size(self):
        return 2

    def rank(self):
        return self._rank

    def allReduce(self, v, op):
        assert op == "sum"
        self.calls += 1
        v.scale(2.0)
        return v


def test_sharded_with_a_foreign_collective_uses_the_post_apply_hook(ctx):
    N, k = 95, 5
    pts = scattered(N, 2, seed=2)
    full = hf.KernelCovarianceOperator(pts, family="sqexp", sigma=1.0, ell=0.3, ctx=ctx)
    W = np.random.default_rng(1).standard_normal((N, k))
    ref = apply(full, W, ctx).to_dense()
    for rank in (0, 1):
        coll = _SumOfTwo(rank)
        s = full.sharded(coll)
        r0, r1 = hf.shard_rows(N, 2, rank)
        assert (s.row0, s.row1) == (r0, r1) and s.collective is coll
        got = apply(s, W, ctx).to_dense()
        expect = np.zeros((N, k))
        expect[r0:r1] = 2.0 * ref[r0:r1]
        assert coll.calls == 1 and np.array_equal(got, expect)
        with pytest.raises(hf.HfmiError) as e:
            apply(s, W, ctx, accumulate=True, Y=hf.MultiVector(N, k, ctx=ctx))
        assert "ambiguous" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- 10. ranks
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharing_the_gpu(tmp_path, world):
    """Every rank applies its row slab and the communicator's SUM completes the block: on every rank the sharded apply equals the full
    apply that rank computes itself, and the 'mass' KLE is the same with sharding on and off."""
    from hippyflow_amd.launch import spawn_ranks
    N = 333
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="60")
    assert spawn_ranks([WORKER, str(tmp_path)], world, env=env, timeout=300) == 0
    rs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    sizes = {2: [167, 166], 3: [111, 111, 111]}[world]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for rank, r in enumerate(rs):
        assert int(r["size"]) == world and int(r["rank"]) == rank
        assert list(r["rows"]) == [starts[rank], starts[rank + 1]]
        assert np.abs(r["Y_full"]).min() > 0
        assert np.array_equal(r["Y_sharded"], r["Y_full"])
        assert np.array_equal(r["Y_full"], rs[0]["Y_full"])
        assert "ambiguous" in str(r["accumulate"])
        assert np.array_equal(r["d_on"], r["d_off"]) and np.array_equal(r["dec_on"], r["dec_off"])
        assert np.array_equal(r["enc_on"], r["enc_off"])
        assert np.array_equal(r["d_on"], rs[0]["d_on"]) and np.array_equal(r["dec_on"], rs[0]["dec_on"])
        assert list(r["rows2"]) == list(hf.shard_rows(2, world, rank))
        assert np.array_equal(r["Y2_sharded"], r["Y2_full"]) and np.abs(r["Y2_full"]).min() > 0
    if world == 3:
        assert list(rs[2]["rows2"]) == [2, 2]                      # the empty shard


# ---------------------------------------------------------------------------------------------------------------- 11. arguments
def test_invalid_arguments(ctx):
    S, T = L.as_f64(scattered(10, 2, seed=1)), L.as_f64(scattered(4, 2, seed=2))
    NO = L.KERNEL_NO_DIAGONAL

    def cross(targets=T, M=4, sources=S, N=10, d=2, family=1, sigma=1.0, ell=0.1, nugget=0.0, diag=NO):
        out = C.c_void_p()
        try:
            L.call("hfmi_op_kernel_cross_cov", ctx.handle, None if targets is None else L.ptr(targets), M,
                   None if sources is None else L.ptr(sources), N, d, family, sigma, ell, nugget, diag, C.byref(out))
        finally:
            created = bool(out.value)
            if created:
                L.load().hfmi_op_destroy(out)
        return created

    def rows(points=S, N=10, d=2, family=1, sigma=1.0, ell=0.1, nugget=0.0, row0=0, nrows=10):
        out = C.c_void_p()
        try:
            L.call("hfmi_op_kernel_cov_rows", ctx.handle, None if points is None else L.ptr(points), N, d, family, sigma, ell, nugget,
                   row0, nrows, C.byref(out))
        finally:
            created = bool(out.value)
            if created:
                L.load().hfmi_op_destroy(out)
        return created

    assert cross() and cross(diag=6, nugget=0.2) and cross(diag=0) and rows() and rows(row0=10, nrows=0) and rows(row0=3, nrows=0)
    bad_cross = {"d = 0": dict(d=0), "d = 4": dict(d=4, N=5, M=2), "ell = 0": dict(ell=0.0), "ell < 0": dict(ell=-0.1),
                 "nugget < 0": dict(nugget=-1e-3, diag=0), "family = 4": dict(family=4), "family = -1": dict(family=-1),
                 "M = 0": dict(M=0), "N = 0": dict(N=0), "no targets": dict(targets=None), "no sources": dict(sources=None),
                 "diag = -2": dict(diag=-2), "diag + M > N": dict(diag=7), "nugget without a diagonal": dict(nugget=0.1)}
    bad_rows = {"d = 0": dict(d=0), "d = 4": dict(d=4, N=5, nrows=5), "ell = 0": dict(ell=0.0), "nugget < 0": dict(nugget=-1e-3),
                "family = 4": dict(family=4), "N = 0": dict(N=0, nrows=0), "no points": dict(points=None), "row0 < 0": dict(row0=-1, nrows=3),
                "nrows < 0": dict(row0=3, nrows=-1), "row0 + nrows > N": dict(row0=3, nrows=8), "row0 > N": dict(row0=11, nrows=0)}
    for make, bad in ((cross, bad_cross), (rows, bad_rows)):
        for what, kw in bad.items():
            with pytest.raises(L.HfmiError) as e:
                make(**kw)
            assert e.value.code == -1 and str(e.value), what                  # HFMI_ERR_INVALID, with a message
    # blocks of other lengths at apply: refused before any launch, Y untouched
    for op, n_in, n_out in ((hf.KernelCrossCovarianceOperator(T, S, ctx=ctx), 10, 4),
                            (hf.KernelCovarianceOperator(S, ctx=ctx).rows(2, 7), 10, 10)):
        for wn, yn in ((12, n_out), (n_in, 12), (n_out, n_in) if n_in != n_out else (12, 12)):
            Yh = np.random.default_rng(2).standard_normal((yn, 3))
            W, Y = hf.MultiVector.from_dense(np.ones((wn, 3)), ctx=ctx), hf.MultiVector.from_dense(Yh, ctx=ctx)
            with pytest.raises(hf.HfmiError) as e:
                op.matMvMult(W, Y)
            assert e.value.code == -1 and "length" in str(e.value)
            assert np.array_equal(Y.to_dense(), Yh)
    # the pivoted Cholesky factorises the square operator only: Python refuses by type, the library by kind
    slab = hf.KernelCovarianceOperator(S, ctx=ctx).rows(0, 10)
    crs = hf.KernelCrossCovarianceOperator(S, S, diag_offset=0, ctx=ctx)
    for op in (slab, crs):
        with pytest.raises(ValueError):
            hf.pivoted_cholesky(op, 4)
        out = C.c_void_p()
        with pytest.raises(L.HfmiError) as e:
            L.call("hfmi_pchol_create", op._op, 4, 0.0, C.byref(out))
        assert e.value.code == -1 and not out.value
