"""Box Whittle-Matern priors on the device at axes whose transformed line has odd factors (2^m 3^a 5^b entries, a multiple of 4:
k_boxcov_pass_mr of hfmi_boxcov.hip): every operator W^a T_s W^b against the dense host operator, long lines against numpy's FFT,
bit-identity, the block contract, the prior end to end and the C ABI.  ``Dense`` and ``host_fft_apply`` restate the helpers of
tests/test_gpu_box_prior.py, and the bound of an apply is that file's, unchanged: per column
    ||y - y_ref||_2 <= 32 max(1, log2 Ptot) eps sqrt(Ptot) ||c_s||_2 max(w^a) ||W^b x||_2 + 8 N eps || |A| |x| ||_2
with c_s = ifftn(lambda^s) over the extended (mirrored) array and Ptot = prod P_c; nothing in it assumes a power of two."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402

import hippyflow_amd as hf                        # noqa: E402
from hippyflow_amd import BoxSpectralCovariance, BoxSpectralPrior   # noqa: E402
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
POWERS = {"C": (1.0, 0.0, -1.0), "R": (-1.0, 1.0, 0.0), "S": (0.5, 0.0, -0.5), "St": (0.5, 0.5, -1.0), "Sinv": (-0.5, 0.5, 0.0)}
SPACING, THETA = (0.3, 0.2, 0.25), (1.0, 2.5, 0.5)
GAMMA, DELTA = 0.7, 1.3
NEU, PER = "neumann", "periodic"
SHAPES = [((7,), NEU), ((11,), NEU), ((13,), NEU), ((19,), NEU), ((31,), NEU), ((51,), NEU),
          ((12,), PER), ((20,), PER), ((36,), PER), ((60,), PER),
          ((7, 5), NEU), ((5, 7), NEU), ((13, 11), NEU), ((12, 7), (PER, NEU)), ((7, 12), (NEU, PER)), ((7, 3, 12), (NEU, NEU, PER)),
          ((1, 7), NEU),
          # strided lines of 24 and 60 entries, contiguous ones of 20 and 60: three lines in a workgroup of four
          ((3, 13), NEU), ((3, 31), NEU), ((11, 3), NEU), ((31, 3), NEU)]


def case_id(shape, boundary):
    b = [boundary] * len(shape) if isinstance(boundary, str) else boundary
    return "x".join("%d%s" % (n, v[0]) for n, v in zip(shape, b))


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def make_box(ctx, shape, boundary, symbol="fd", alpha=2.0):
    d = len(shape)
    return BoxSpectralCovariance(shape, SPACING[:d], GAMMA, DELTA, alpha=alpha, theta=THETA[:d], boundary=boundary, symbol=symbol, ctx=ctx)


def dev(A, ctx):
    return hf.MultiVector.from_dense(np.ascontiguousarray(A), ctx=ctx)


class Dense:
    """the dense host operators of one box and what the bound needs of them, computed once"""

    def __init__(self, box):
        self.box, self.w, self.N = box, box.weights, box.N
        lam = box.spectrum()
        idx = []
        for c, n in enumerate(box.grid_shape):
            if box.boundary[c] == PER or n == 1:
                idx.append(np.arange(n))
            else:
                k = np.arange(2 * (n - 1))
                idx.append(np.minimum(k, 2 * (n - 1) - k))
        self.lam_ext = lam[np.ix_(*idx)]
        self.Ptot = self.lam_ext.size
        self._A, self._c = {}, {}

    def A(self, s, a, b):
        if (s, a, b) not in self._A:
            self._A[(s, a, b)] = self.box.dense_power(s, a, b)
        return self._A[(s, a, b)]

    def transform_term(self, s, a, b, X):
        if s not in self._c:
            self._c[s] = np.linalg.norm(np.fft.ifftn(self.lam_ext ** s))
        return (32.0 * max(1.0, np.log2(self.Ptot)) * EPS * np.sqrt(self.Ptot) * self._c[s] * np.max(self.w ** a)
                * np.linalg.norm((self.w ** b)[:, None] * X, axis=0))

    def bound(self, s, a, b, X):
        """per column of X: the bound of the module's docstring"""
        return self.transform_term(s, a, b, X) + 8.0 * self.N * EPS * np.linalg.norm(np.abs(self.A(s, a, b)) @ np.abs(X), axis=0)


def within_bound(what, Y, Y_ref, bound):
    ratio = np.linalg.norm(Y - Y_ref, axis=0) / np.maximum(bound, 1e-300)
    print("%s: worst error / bound %.3g" % (what, ratio.max()))
    assert np.all(np.isfinite(Y)) and np.all(ratio <= 1.0), (what, ratio)


# ---------------------------------------------------------------------------------------------------------------- 1. apply against the dense operator
@pytest.mark.parametrize("alpha", [2.0, 1.5])
@pytest.mark.parametrize("symbol", ["fd", "continuous"])
@pytest.mark.parametrize("shape,boundary", SHAPES, ids=[case_id(*c) for c in SHAPES])
def test_apply_against_the_dense_host_operator(ctx, shape, boundary, symbol, alpha):
    """C, R, S, S^T and S^-1 with 1, 2 and 3 columns, and one accumulating apply (the sum of both applies' bounds)."""
    box = make_box(ctx, shape, boundary, symbol, alpha)
    D = Dense(box)
    rng = np.random.default_rng(box.N + int(10 * alpha))
    ops = {"C": box.C, "R": box.R, "S": box.S, "St": box.S.transpose(), "Sinv": box.Sinv}
    for name, op in ops.items():
        s, a, b = POWERS[name]
        assert op.power == (s, a, b) and op.shape == (box.N, box.N)
        for nvec in (1, 2, 3):
            X = rng.standard_normal((box.N, nvec))
            Y = hf.MultiVector(box.N, nvec, ctx=ctx)
            op.matMvMult(dev(X, ctx), Y)
            within_bound("%s %s nvec=%d" % (case_id(shape, boundary), name, nvec), Y.to_dense(), D.A(s, a, b) @ X, D.bound(s, a, b, X))
    s, a, b = POWERS["C"]
    X1, X2 = rng.standard_normal((box.N, 3)), rng.standard_normal((box.N, 3))
    Y = hf.MultiVector(box.N, 3, ctx=ctx)
    box.C.matMvMult(dev(X1, ctx), Y)
    box.C.matMvMult(dev(X2, ctx), Y, accumulate=True)
    within_bound("accumulate", Y.to_dense(), D.A(s, a, b) @ X1 + D.A(s, a, b) @ X2, D.bound(s, a, b, X1) + D.bound(s, a, b, X2))


# ---------------------------------------------------------------------------------------------------------------- 2. long lines against numpy's FFT
def host_fft_apply(D, s, a, b, X):
    """W^a T_s W^b X by the definition, with numpy's FFT over the mirrored array"""
    box = D.box
    shape = box.grid_shape
    out = np.empty_like(X)
    for j in range(X.shape[1]):
        x = ((D.w ** b) * X[:, j]).reshape(shape[::-1]).transpose()
        for c, n in enumerate(shape):
            if box.boundary[c] == NEU and n > 1:
                x = np.concatenate([x, np.flip(np.take(x, np.arange(1, n - 1), axis=c), axis=c)], axis=c)
        y = np.fft.ifftn(D.lam_ext ** s * np.fft.fftn(x)).real
        y = y[tuple(slice(0, n) for n in shape)]
        out[:, j] = (D.w ** a) * y.transpose().ravel()
    return out


LONG_CASES = [((1945,), NEU), ((2001,), NEU), ((3840,), PER), ((3, 1921), NEU), ((4, 4000), PER), ((193, 193), NEU), ((97, 33), NEU),
              ((20, 13, 12), (PER, NEU, PER))]


@pytest.mark.parametrize("shape,boundary", LONG_CASES, ids=[case_id(*c) for c in LONG_CASES])
def test_long_lines_and_many_workgroups_against_the_host_fft(ctx, shape, boundary):
    """The longest mixed-radix lines (3888 = 2^4 3^5, 4000 = 2^5 5^3 and 3840 = 2^8 3 5 entries; two strided lines of 3840 and of 4000 side
    by side) and grids of several workgroups with a ragged last one: y_ref is the definition evaluated with numpy's FFT.  Both sides
    are transforms, so the bound is the transform term of the module's bound twice; and R (C x) = x within the sum of the two applies'
    transform terms."""
    box = make_box(ctx, shape, boundary)
    D = Dense(box)
    X = np.random.default_rng(box.N).standard_normal((box.N, 3))
    Xd = dev(X, ctx)
    results = {}
    for name in ("C", "R", "S"):
        s, a, b = POWERS[name]
        Y = hf.MultiVector(box.N, 3, ctx=ctx)
        getattr(box, name).matMvMult(Xd, Y)
        results[name] = Y.to_dense()
        within_bound("%s %s vs host FFT" % (case_id(shape, boundary), name), results[name], host_fft_apply(D, s, a, b, X), 2.0 * D.transform_term(s, a, b, X))
    Y = hf.MultiVector(box.N, 3, ctx=ctx)
    box.R.matMvMult(dev(results["C"], ctx), Y)
    bound = D.transform_term(*POWERS["C"], X) + D.transform_term(*POWERS["R"], host_fft_apply(D, *POWERS["C"], X))
    within_bound("R C x = x", Y.to_dense(), X, bound)


# ---------------------------------------------------------------------------------------------------------------- 3. bit-identity
BIT_CASES = [((13, 11), NEU), ((12, 7, 5), (PER, NEU, NEU))]


@pytest.mark.parametrize("shape,boundary", BIT_CASES, ids=[case_id(*c) for c in BIT_CASES])
def test_two_applies_chunking_and_accumulation_give_the_same_bits(ctx, shape, boundary):
    box = make_box(ctx, shape, boundary)
    rng = np.random.default_rng(3)
    X = dev(rng.standard_normal((box.N, 5)), ctx)
    Y0 = rng.standard_normal((box.N, 5))
    for op in (box.C, box.R, box.S):
        Y1, Y2, Y3 = (hf.MultiVector(box.N, 5, ctx=ctx) for _ in range(3))
        op.matMvMult(X, Y1)
        op.matMvMult(X, Y2)
        L.call("hfmi_tuning_set", b"fftcov_pairs", 1)
        try:
            op.matMvMult(X, Y3)
        finally:
            L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
        assert np.array_equal(Y1.to_dense(), Y2.to_dense()) and np.array_equal(Y1.to_dense(), Y3.to_dense())
        Y4 = dev(Y0, ctx)
        op.matMvMult(X, Y4, accumulate=True)                # adds exactly what the overwriting apply stores
        assert np.array_equal(Y4.to_dense(), Y0 + Y1.to_dense())


# ---------------------------------------------------------------------------------------------------------------- 4. block contract
BLOCK_CASES = [((7, 5), NEU), ((12, 7), (PER, NEU))]


@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
@pytest.mark.parametrize("shape,boundary", BLOCK_CASES, ids=[case_id(*c) for c in BLOCK_CASES])
def test_block_contract_of_the_apply(ctx, shape, boundary, layout):
    """Y a view inside a wider parent with guard columns: padding rows stay +0.0, nothing outside Y's window changes, an overwriting
    apply equals the apply into a plain block bit for bit and an accumulating one adds it; blocks of another length are refused."""
    box = make_box(ctx, shape, boundary)
    N, k, guard = box.N, 3, 2
    rng = np.random.default_rng(N)
    Xin = dev(rng.standard_normal((N, k)), ctx)
    for op in (box.C, box.S.transpose()):
        plain = hf.MultiVector(N, k, ctx=ctx)
        op.matMvMult(Xin, plain)
        Dn = plain.to_dense()
        if layout == "wrapped":
            a = ba.Arena.wrapped(ctx, N, k + 2 * guard, ld=ba.round_up(N, 32) + 32)
            y = a.window(guard, k)
        else:
            a = ba.Arena.in_parent(ctx, N, 2 * k + 2 * guard)
            a.window(guard, k)
            y = a.window(guard + k, k)
        Y0 = rng.standard_normal((N, k))
        L.call("hfmi_block_upload", y.mv.handle, L.ptr(L.as_f64(Y0)), L.LAYOUT_DENSE)
        for accumulate in (True, False, True):
            a.snapshot()
            before = y.mv.to_dense()
            op.matMvMult(Xin, y.mv, accumulate=accumulate)
            a.check(written=[y], what="hfmi_op_apply of a box operator accumulate=%d [%s]" % (accumulate, layout))
            assert np.array_equal(y.mv.to_dense(), before + Dn if accumulate else Dn), accumulate
        for bad_in, bad_out in ((N + 1, N), (N, N + 1)):
            with pytest.raises(hf.HfmiError):
                op.matMvMult(hf.MultiVector(bad_in, k, ctx=ctx), hf.MultiVector(bad_out, k, ctx=ctx))


# ---------------------------------------------------------------------------------------------------------------- 5. the prior end to end
@pytest.fixture(scope="module")
def prior137(ctx):
    box = make_box(ctx, (13, 7), NEU)
    mean = np.cos(np.arange(box.N) * 0.37)
    return box, Dense(box), BoxSpectralPrior(box, mean=mean, M=sp.diags(box.weights, format="csr"), seed=1234), mean


def test_prior_sample_and_cost(ctx, prior137):
    box, D, prior, mean = prior137
    N = box.N
    rng = np.random.default_rng(5)
    xi = rng.standard_normal(N)
    S = D.A(*POWERS["S"])
    bound = D.bound(*POWERS["S"], xi[:, None])
    noise, m = hf.new_host_vector(), hf.new_host_vector()
    prior.init_vector(noise, "noise")
    prior.init_vector(m, 0)
    noise.set_local(xi)
    prior.sample(noise, m)
    within_bound("sample (host vectors)", m.get_local()[:, None] - mean[:, None], (S @ xi)[:, None], bound)
    nd, md = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    prior.init_vector(nd, "noise")
    prior.init_vector(md, 0)
    nd.set_local(xi)
    prior.sample(nd, md, add_mean=False)
    within_bound("sample (device vectors, no mean)", md.get_local()[:, None], (S @ xi)[:, None], bound)
    # cost against numpy: the apply's bound on R dm, carried through the inner product
    mm = mean + rng.standard_normal(N)
    dm = mm - mean
    Rd = D.A(*POWERS["R"])
    ref = 0.5 * dm @ (Rd @ dm)
    tol = 0.5 * np.linalg.norm(dm) * D.bound(*POWERS["R"], dm[:, None])[0] + 4 * N * EPS * np.abs(dm) @ (np.abs(Rd) @ np.abs(dm))
    got = prior.cost(mm)
    print("cost %.17g ref %.17g tol %.3g" % (got, ref, tol))
    assert abs(got - ref) <= tol
    assert prior.cost(mean) == 0.0


def test_generalized_double_pass_with_the_box_precision(ctx, prior137):
    """A = J^T J of rank 6, k = 6 and 4 extra probes: doublePassG(A, R, Rsolver) against scipy's eigh(A, R_dense) to 1e-9 relative and
    R-orthonormal eigenvectors to 1e-9, the tolerances tests/test_gpu_box_prior.py holds the (9, 5) box to."""
    box, D, prior, mean = prior137
    N, k, p = box.N, 6, 4
    rng = np.random.default_rng(21)
    J = rng.standard_normal((k, N))
    Ad = J.T @ J
    A = hf.npToDeviceOperator(Ad, ctx=ctx)
    Omega = dev(rng.standard_normal((N, k + p)), ctx)
    Rd = D.A(*POWERS["R"])
    exact = sla.eigh(Ad, 0.5 * (Rd + Rd.T), eigvals_only=True)[::-1][:k]
    d, U = hf.doublePassG(A, prior.R, prior.Rsolver, Omega, k, s=1)
    print("doublePassG rel err %.3g" % np.abs(d / exact - 1.0).max())
    np.testing.assert_allclose(d, exact, rtol=1e-9)
    Ud = U.to_dense()
    assert np.abs(Ud.T @ (Rd @ Ud) - np.eye(k)).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------- 6. the C ABI
def test_c_abi_refuses_and_creates_by_the_new_rule(ctx):
    out = C.c_void_p()

    def create(shape, boundary):
        n = np.ascontiguousarray(shape, dtype=np.int64)
        hh = np.ascontiguousarray((0.1, 0.2)[:len(shape)], dtype=np.float64)
        bd = np.ascontiguousarray(boundary, dtype=np.int32)
        L.call("hfmi_box_create", ctx.handle, len(shape), L.ptr(n), L.ptr(hh), L.ptr(bd), 1.0, 1.0, 1.5, None, 0, C.byref(out))
        return C.c_void_p(out.value)

    for shape, boundary in (((8, 5), (0, 0)), ((28,), (1,))):
        with pytest.raises(hf.HfmiError) as e:
            create(shape, boundary)
        assert e.value.code == -1 and len(str(e.value)) > 20, shape
    box = create((7, 5), (0, 0))
    try:
        lam = np.empty(35)
        L.call("hfmi_box_spectrum", box, L.ptr(lam))
    finally:
        L.call("hfmi_box_destroy", box)
    ref = BoxSpectralCovariance((7, 5), (0.1, 0.2), 1.0, 1.0, alpha=1.5)
    assert np.abs(lam / ref.spectrum().transpose().ravel() - 1.0).max() <= 64 * EPS
