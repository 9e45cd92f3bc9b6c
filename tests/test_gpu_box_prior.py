"""Box Whittle-Matern priors on the device (``BoxSpectralCovariance`` / ``BoxSpectralPrior``, hfmi_op_box, hfmi_boxcov.hip): every operator
W^a T_s W^b against the dense host operator built from cosines and exponentials (no FFT on the host side), the identities between them,
bit-identity, the prior protocol and the solvers that take a prior with a precision.

The bound of an apply, per column (the project's own, tests/test_gpu_grid_kernel_cov.py, with the weights carried along):
    ||y - y_ref||_2 <= 32 max(1, log2 Ptot) eps sqrt(Ptot) ||c_s||_2 max(w^a) ||W^b x||_2 + 8 N eps || |A| |x| ||_2
with c_s = ifftn(lambda^s) over the extended (mirrored) array, Ptot = prod P_c and y_ref = A x for the dense A = W^a T_s W^b.  The first
term is the transform's rounding, the second the host reference's own."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import block_arena as ba                          # noqa: E402
import fake_pde as fp                             # noqa: E402

import hippyflow_amd as hf                        # noqa: E402
from hippyflow_amd import BoxSpectralCovariance, BoxSpectralPrior   # noqa: E402
from hippyflow_amd import _lib as L               # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
POWERS = {"C": (1.0, 0.0, -1.0), "R": (-1.0, 1.0, 0.0), "S": (0.5, 0.0, -0.5), "St": (0.5, 0.5, -1.0), "Sinv": (-0.5, 0.5, 0.0)}
SPACING, THETA = (0.3, 0.2, 0.25), (1.0, 2.5, 0.5)
GAMMA, DELTA = 0.7, 1.3
NEU, PER = "neumann", "periodic"
SHAPES = [((2,), NEU), ((3,), NEU), ((5,), NEU), ((17,), NEU), ((33,), NEU),
          ((1,), PER), ((2,), PER), ((8,), PER), ((32,), PER),
          ((9, 5), NEU), ((1, 9), NEU), ((8, 5), (PER, NEU)), ((5, 8), (NEU, PER)), ((5, 3, 4), (NEU, NEU, PER)),
          ((3, 1), NEU), ((3, 2), NEU), ((3, 9), NEU)]      # strided lines of 1, 2 and 16 entries, three lines in a workgroup of four


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

    def bound(self, s, a, b, X):
        """per column of X: the bound of the module's docstring"""
        if s not in self._c:
            self._c[s] = np.linalg.norm(np.fft.ifftn(self.lam_ext ** s))
        first = (32.0 * max(1.0, np.log2(self.Ptot)) * EPS * np.sqrt(self.Ptot) * self._c[s] * np.max(self.w ** a)
                 * np.linalg.norm((self.w ** b)[:, None] * X, axis=0))
        return first + 8.0 * self.N * EPS * np.linalg.norm(np.abs(self.A(s, a, b)) @ np.abs(X), axis=0)


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
    # accumulate: Y = C X1, then Y += C X2
    s, a, b = POWERS["C"]
    X1, X2 = rng.standard_normal((box.N, 3)), rng.standard_normal((box.N, 3))
    Y = hf.MultiVector(box.N, 3, ctx=ctx)
    box.C.matMvMult(dev(X1, ctx), Y)
    box.C.matMvMult(dev(X2, ctx), Y, accumulate=True)
    within_bound("accumulate", Y.to_dense(), D.A(s, a, b) @ X1 + D.A(s, a, b) @ X2, D.bound(s, a, b, X1) + D.bound(s, a, b, X2))


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


LONG_CASES = [((2049,), NEU), ((4096,), PER), ((3, 2049), NEU), ((4, 4096), PER), ((65, 33), NEU), ((16, 9, 8), (PER, NEU, PER))]


@pytest.mark.parametrize("shape,boundary", LONG_CASES, ids=[case_id(*c) for c in LONG_CASES])
def test_long_lines_and_many_workgroups_against_the_host_fft(ctx, shape, boundary):
    """The longest lines (4096 entries: one contiguous line of 64 KiB per workgroup, two strided ones side by side) and grids of several
    workgroups with a ragged last one, where a dense reference is out of reach: y_ref is the definition evaluated with numpy's FFT.
    Both sides are transforms, so the bound is the transform term of the module's bound twice (the dense reference's term has no
    counterpart here); and R (C x) = x within the sum of the two applies' transform terms, as every composition in this file."""
    box = make_box(ctx, shape, boundary)
    D = Dense(box)
    X = np.random.default_rng(box.N).standard_normal((box.N, 3))
    Xd = dev(X, ctx)

    def transform_term(s, a, b, V):
        c = np.linalg.norm(np.fft.ifftn(D.lam_ext ** s))
        return (32.0 * max(1.0, np.log2(D.Ptot)) * EPS * np.sqrt(D.Ptot) * c * np.max(D.w ** a) * np.linalg.norm((D.w ** b)[:, None] * V, axis=0))

    results = {}
    for name in ("C", "R", "S"):
        s, a, b = POWERS[name]
        Y = hf.MultiVector(box.N, 3, ctx=ctx)
        getattr(box, name).matMvMult(Xd, Y)
        results[name] = Y.to_dense()
        within_bound("%s %s vs host FFT" % (case_id(shape, boundary), name), results[name], host_fft_apply(D, s, a, b, X), 2.0 * transform_term(s, a, b, X))
    # R (C x) = x
    Y = hf.MultiVector(box.N, 3, ctx=ctx)
    box.R.matMvMult(dev(results["C"], ctx), Y)
    bound = transform_term(*POWERS["C"], X) + transform_term(*POWERS["R"], host_fft_apply(D, *POWERS["C"], X))
    within_bound("R C x = x", Y.to_dense(), X, bound)


def test_spectrum_of_the_library_is_the_host_formula(ctx):
    for shape, boundary in (((9, 5), NEU), ((5, 3, 4), (NEU, NEU, PER)), ((1, 9), NEU)):
        for symbol in ("fd", "continuous"):
            box = make_box(ctx, shape, boundary, symbol, 1.5)
            lam = np.empty(box.N)
            L.call("hfmi_box_spectrum", box.handle, L.ptr(lam))
            ref = box.spectrum().transpose().ravel()         # k0 fastest
            assert np.abs(lam / ref - 1.0).max() <= 64 * EPS


# ---------------------------------------------------------------------------------------------------------------- 2. identities
IDENT_CASES = [((33,), NEU), ((32,), PER), ((9, 5), NEU), ((8, 5), (PER, NEU)), ((5, 3, 4), (NEU, NEU, PER))]


@pytest.mark.parametrize("shape,boundary", IDENT_CASES, ids=[case_id(*c) for c in IDENT_CASES])
def test_identities_between_the_operators(ctx, shape, boundary):
    """R (C x) = x, S (S^T x) = C x, Sinv (S x) = x, each within the sum of the two applies' bounds: the first apply's on x, the
    second's on the exact intermediate A x."""
    box = make_box(ctx, shape, boundary)
    D = Dense(box)
    X = np.random.default_rng(7).standard_normal((box.N, 3))
    Xd = dev(X, ctx)

    def composed(first, second):
        T, Y = hf.MultiVector(box.N, 3, ctx=ctx), hf.MultiVector(box.N, 3, ctx=ctx)
        first.matMvMult(Xd, T)
        second.matMvMult(T, Y)
        return Y.to_dense(), D.bound(*first.power, X) + D.bound(*second.power, D.A(*first.power) @ X)

    Y, bound = composed(box.C, box.R)
    within_bound("R C x = x", Y, X, bound)
    Y, bound = composed(box.S.transpose(), box.S)
    within_bound("S S^T x = C x", Y, D.A(*POWERS["C"]) @ X, bound)
    Y, bound = composed(box.S, box.Sinv)
    within_bound("Sinv S x = x", Y, X, bound)


def test_dense_factor_squares_to_the_covariance(ctx):
    """(9, 5): the dense S S^T, made on the device by S (S^T I), against to_dense("C"): column j within the sum of the two applies'
    bounds, S^T's on e_j and S's on the exact S^T e_j."""
    box = make_box(ctx, (9, 5), NEU)
    D = Dense(box)
    N = box.N
    I = np.eye(N)
    T, Y = hf.MultiVector(N, N, ctx=ctx), hf.MultiVector(N, N, ctx=ctx)
    box.S.transpose().matMvMult(dev(I, ctx), T)
    box.S.matMvMult(T, Y)
    within_bound("S^T e_j", T.to_dense(), D.A(*POWERS["St"]), D.bound(*POWERS["St"], I))
    within_bound("S S^T against C", Y.to_dense(), box.to_dense("C"), D.bound(*POWERS["St"], I) + D.bound(*POWERS["S"], D.A(*POWERS["St"])))


# ---------------------------------------------------------------------------------------------------------------- 3. bit-identity
BIT_CASES = [((33,), NEU), ((9, 5), NEU), ((8, 5), (PER, NEU)), ((5, 3, 4), (NEU, NEU, PER))]


@pytest.mark.parametrize("shape,boundary", BIT_CASES, ids=[case_id(*c) for c in BIT_CASES])
def test_two_applies_and_any_chunking_give_the_same_bits(ctx, shape, boundary):
    box = make_box(ctx, shape, boundary)
    X = dev(np.random.default_rng(3).standard_normal((box.N, 5)), ctx)
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
    # the factor's transposed applies are its transpose's applies; the transpose of the transpose is the factor
    St = box.S.transpose()
    assert St.transpose() is box.S and St.power == POWERS["St"]
    Y1, Y2 = hf.MultiVector(box.N, 5, ctx=ctx), hf.MultiVector(box.N, 5, ctx=ctx)
    St.matMvMult(X, Y1)
    box.S.matMvTranspmult(X, Y2)
    assert np.array_equal(Y1.to_dense(), Y2.to_dense())
    x, y = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    box.S.init_vector(x, 0)
    box.S.init_vector(y, 1)
    x.set_local(X.to_dense()[:, 0])
    box.S.transpmult(x, y)
    St.matMvMult(X.view(0, 1), Y1.view(0, 1))
    assert np.array_equal(y.get_local(), Y1.to_dense()[:, 0])


@pytest.mark.parametrize("layout", ["wrapped", "adjacent"])
@pytest.mark.parametrize("shape,boundary", BIT_CASES, ids=[case_id(*c) for c in BIT_CASES])
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


# ---------------------------------------------------------------------------------------------------------------- 4. the prior protocol
@pytest.fixture(scope="module")
def prior95(ctx):
    box = make_box(ctx, (9, 5), NEU)
    mean = np.cos(np.arange(box.N) * 0.37)
    return box, Dense(box), BoxSpectralPrior(box, mean=mean, M=sp.diags(box.weights, format="csr"), seed=1234), mean


def test_prior_sample_and_cost(ctx, prior95):
    box, D, prior, mean = prior95
    N = box.N
    rng = np.random.default_rng(5)
    xi = rng.standard_normal(N)
    S = D.A(*POWERS["S"])
    bound = D.bound(*POWERS["S"], xi[:, None])
    noise, m = hf.new_host_vector(), hf.new_host_vector()
    prior.init_vector(noise, "noise")
    prior.init_vector(m, 0)
    assert noise.get_local().shape == (N,) and m.get_local().shape == (N,)
    noise.set_local(xi)
    prior.sample(noise, m)
    within_bound("sample (host vectors)", m.get_local()[:, None] - mean[:, None], (S @ xi)[:, None], bound)
    prior.sample(noise, m, add_mean=False)
    within_bound("sample without the mean", m.get_local()[:, None], (S @ xi)[:, None], bound)
    nd, md = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    prior.init_vector(nd, "noise")
    prior.init_vector(md, 0)
    nd.set_local(xi)
    prior.sample(nd, md)
    assert np.array_equal(md.get_local(), m.get_local() + mean)
    assert np.array_equal(prior.mean.get_local(), mean)
    with pytest.raises(ValueError):
        short = hf.new_host_vector()
        short.init(N - 1)
        prior.sample(short, m)
    # cost against numpy: the apply's bound on R dm, carried through the inner product
    mm = mean + rng.standard_normal(N)
    dm = mm - mean
    Rd = D.A(*POWERS["R"])
    ref = 0.5 * dm @ (Rd @ dm)
    tol = 0.5 * np.linalg.norm(dm) * D.bound(*POWERS["R"], dm[:, None])[0] + 4 * N * EPS * np.abs(dm) @ (np.abs(Rd) @ np.abs(dm))
    for arg in (mm, md):
        if arg is md:
            md.set_local(mm)
        got = prior.cost(arg)
        print("cost %.17g ref %.17g tol %.3g" % (got, ref, tol))
        assert abs(got - ref) <= tol
    assert prior.cost(mean) == 0.0


def test_prior_sample_block_is_the_seeded_fill_through_the_factor(ctx, prior95):
    box, D, _, mean = prior95
    N, n = box.N, 6
    prior = BoxSpectralPrior(box, mean=mean, seed=77)
    again = BoxSpectralPrior(box, mean=mean, seed=77)
    other = BoxSpectralPrior(box, mean=mean, seed=78)
    blocks = [prior.sample_block(n) for _ in range(2)]
    for stream, B in enumerate(blocks):
        assert B.shape == (n, N)
        Xi = hf.MultiVector(N, n, ctx=ctx)
        L.call("hfmi_randn_fill", Xi.handle, C.c_uint64(77), C.c_uint32(stream), 1.0)
        Y = hf.MultiVector(N, n, ctx=ctx)
        box.S.matMvMult(Xi, Y)
        assert np.array_equal(B, Y.to_dense().T + mean[None, :])
        xi = Xi.to_dense()
        within_bound("sample_block stream %d" % stream, (B - mean[None, :]).T, D.A(*POWERS["S"]) @ xi, D.bound(*POWERS["S"], xi))
    assert not np.array_equal(blocks[0], blocks[1])
    assert np.array_equal(again.sample_block(n), blocks[0]) and np.array_equal(again.sample_block(n), blocks[1])
    assert not np.array_equal(other.sample_block(n), blocks[0])


def test_prior_draws_have_the_covariance(ctx, prior95):
    """4096 draws: every entry of the sample covariance (known mean) within 6 sqrt((C_ii C_jj + C_ij^2) / 4096) of C."""
    box, D, _, mean = prior95
    prior = BoxSpectralPrior(box, mean=mean, seed=2024)
    X = prior.sample_block(4096) - mean[None, :]
    Cd = box.to_dense("C")
    emp = X.T @ X / 4096.0
    dg = np.diag(Cd)
    z = np.abs(emp - Cd) / np.sqrt((np.outer(dg, dg) + Cd ** 2) / 4096.0)
    print("worst deviation %.2f sigma" % z.max())
    assert z.max() <= 6.0


def test_prior_precision_and_solver_are_device_operators(ctx, prior95):
    box, D, prior, mean = prior95
    N = box.N
    assert isinstance(prior.R, hf.DeviceOperator) and prior.R is box.R and prior.C is box.C
    op = hf.as_device_operator(prior.Rsolver)
    assert isinstance(op, hf.DeviceOperator) and not isinstance(op, hf.HostCallbackOperator) and op is box.C
    x = np.random.default_rng(9).standard_normal(N)
    ref, bound = D.A(*POWERS["C"]) @ x, D.bound(*POWERS["C"], x[:, None])
    xh, yh = hf.new_host_vector(), hf.new_host_vector()
    prior.Rsolver.init_vector(xh, 1)
    prior.Rsolver.init_vector(yh, 0)
    xh.set_local(x)
    prior.Rsolver.solve(yh, xh)
    within_bound("Rsolver (host vectors)", yh.get_local()[:, None], ref[:, None], bound)
    xd, yd = hf.Vector(ctx=ctx), hf.Vector(ctx=ctx)
    prior.R.init_vector(xd, 1)
    prior.R.init_vector(yd, 0)
    xd.set_local(x)
    prior.Rsolver.solve(yd, xd)
    assert np.array_equal(yd.get_local(), yh.get_local())
    prior.R.solve(yd, xd)                                   # the precision's own inverse is the covariance
    assert np.array_equal(yd.get_local(), yh.get_local())


# ---------------------------------------------------------------------------------------------------------------- 5. solvers
def test_generalized_double_pass_with_the_box_precision(ctx, prior95):
    """A = J^T J of rank 6, k = 6 and 4 extra probes: doublePassG(A, R, Rsolver) against scipy's eigh(A, R_dense) to 1e-9 relative (the
    tolerance tests/test_gpu_configs_r2.py holds doublePassG to); doublePassC(A, C) gives the same eigenvalues."""
    box, D, prior, mean = prior95
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
    dc, Uc, Ec = hf.doublePassC(A, prior.C, Omega, k, s=1)
    print("doublePassC rel err %.3g" % np.abs(dc / exact - 1.0).max())
    np.testing.assert_allclose(dc, exact, rtol=1e-9)
    np.testing.assert_allclose(dc, d, rtol=1e-9)


def test_mass_orthogonal_kle_is_the_analytical_one(ctx, prior95, tmp_path):
    """KLEProjector over the prior with M = diag(w), orthogonality 'mass', rank + oversampling = N: C W phi_k = lambda_k phi_k, so the
    r largest lambda_k come back to 1e-10 relative."""
    box, D, prior, mean = prior95
    r = 8
    params = hf.KLEParameterList()
    params['rank'], params['oversampling'] = r, box.N - r
    params['verbose'], params['save_and_plot'] = False, False
    params['output_directory'] = str(tmp_path) + "/"
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    d, dec, enc = kle.construct_input_subspace('mass')
    exact = np.sort(box.spectrum().ravel())[::-1][:r]
    print("KLE rel err %.3g" % np.abs(np.asarray(d) / exact - 1.0).max())
    np.testing.assert_allclose(d, exact, rtol=1e-10)


class _HostPrecisionPrior:
    """The same Gaussian with the dense precision as a HOST operator and no ``C``: the route a prior assembled on the host takes.  Draws
    are the box prior's, so identical seeds give identical samples."""

    def __init__(self, prior, Rd):
        self._p = prior
        self.R = fp.MatrixOperator(0.5 * (Rd + Rd.T))
        self.Rsolver = prior.Rsolver
        self.mean = prior.mean

    def init_vector(self, x, dim):
        self._p.init_vector(x, dim)

    def sample(self, noise, m, add_mean=True):
        self._p.sample(noise, m, add_mean=add_mean)


def test_active_subspace_projector_takes_the_box_prior_unchanged(ctx, prior95, tmp_path):
    """(9, 5), the fake PDE of 45 unknowns with 14 observations: ``ActiveSubspaceProjector`` prior-preconditioned over a ``BoxSpectralPrior``
    (R and R^-1 on the device, the projector's existing doublePassG route) against the same projector over the same Gaussian with the
    dense R as a host operator and the same seeds.  The two runs differ in the rounding of the applies of R alone, a perturbation of the
    pencil of relative size eps cond(R) ~ 1e-12 here, and eigenvalues of a symmetric definite pencil move by at most that times the
    largest one: |d1 - d2| <= 1e-9 d_max (the 1e-9 doublePassG is held to, tests/test_gpu_configs_r2.py); decoder and encoder biorthogonal."""
    box, D, prior, mean = prior95
    N, k = box.N, 7
    Rd = D.A(*POWERS["R"])

    def run(pr, tag):
        obs = fp.ProtocolObservable(fp.NumpyProblem(N, hf.HostVector), fp.MatrixOperator(fp.observation_matrix(14, N)))
        hf.parRandom.reseed(11)
        hf.parRandom.split(0)
        params = hf.ActiveSubspaceParameterList()
        params['samples_per_process'], params['rank'], params['oversampling'] = 6, k, 3
        params['serialized_sampling'], params['verbose'], params['save_and_plot'] = False, False, False
        params['output_directory'] = os.path.join(str(tmp_path), tag) + "/"
        AS = hf.ActiveSubspaceProjector(obs, pr, parameters=params)
        d, dec, enc = AS.construct_input_subspace(prior_preconditioned=True)
        return AS, np.asarray(d), dec.to_dense(), enc.to_dense()

    AS1, d1, dec1, enc1 = run(BoxSpectralPrior(box, mean=mean), "box")
    AS2, d2, dec2, enc2 = run(_HostPrecisionPrior(BoxSpectralPrior(box, mean=mean), Rd), "host")
    assert AS1.E_GN is None and AS1.prior_preconditioned            # the route with R, not doublePassC
    print("AS projector, box prior against the dense host R: |d1 - d2| / d_max %.3g, relative %.3g" % (np.abs(d1 - d2).max() / d2[0], np.max(np.abs(d1 / d2 - 1.0))))
    assert d1.shape == (k,) and d1[-1] > 0
    assert np.abs(d1 - d2).max() <= 1e-9 * d2[0]
    assert np.abs(enc1.T @ dec1 - np.eye(k)).max() <= 1e-10
    assert np.abs(dec1.T @ (Rd @ dec1) - np.eye(k)).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- 6. the C ABI
def test_c_abi_refusals_and_shared_lifetime(ctx):
    out = C.c_void_p()

    def create(shape=(9, 5), h=(0.1, 0.2), boundary=(0, 0), gamma=1.0, delta=1.0, alpha=2.0, theta=(1.0, 1.0), symbol=0, d=None):
        n = np.ascontiguousarray(shape, dtype=np.int64)
        hh, bd = np.ascontiguousarray(h, dtype=np.float64), np.ascontiguousarray(boundary, dtype=np.int32)
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        L.call("hfmi_box_create", ctx.handle, len(shape) if d is None else d, L.ptr(n), L.ptr(hh), L.ptr(bd), gamma, delta, alpha,
               None if th is None else L.ptr(th), symbol, C.byref(out))
        return C.c_void_p(out.value)

    bad = [dict(shape=(4, 5)), dict(shape=(9, 2050)), dict(shape=(6, 5), boundary=(1, 0)), dict(shape=(8192, 5), boundary=(1, 0)),
           dict(shape=(0, 5)), dict(d=0), dict(d=4), dict(h=(0.1, 0.0)), dict(h=(np.nan, 0.1)), dict(h=(np.inf, 0.1)), dict(gamma=0.0),
           dict(gamma=np.inf), dict(delta=-1.0), dict(delta=np.nan), dict(alpha=0.0), dict(alpha=np.inf), dict(theta=(1.0, -2.0)),
           dict(theta=(np.nan, 1.0)), dict(boundary=(0, 2)), dict(boundary=(-1, 0)), dict(symbol=2), dict(symbol=-1)]
    for change in bad:
        with pytest.raises(hf.HfmiError) as e:
            create(**change)
        assert e.value.code == -1 and len(str(e.value)) > 20, change
    with pytest.raises(hf.HfmiError):
        L.call("hfmi_op_box", None, 1.0, 0.0, -1.0, C.byref(out))
    box = create(theta=None)                               # theta NULL: all ones
    ref = BoxSpectralCovariance((9, 5), (0.1, 0.2), 1.0, 1.0, ctx=ctx)
    lam = np.empty(45)
    L.call("hfmi_box_spectrum", box, L.ptr(lam))
    assert np.abs(lam / ref.spectrum().transpose().ravel() - 1.0).max() <= 64 * EPS
    for powers in ((np.nan, 0.0, 0.0), (1.0, np.inf, 0.0), (1.0, 0.0, np.nan)):
        with pytest.raises(hf.HfmiError):
            L.call("hfmi_op_box", box, *powers, C.byref(out))
    # the operator shares the box's state: the box may go first
    op = C.c_void_p()
    L.call("hfmi_op_box", box, 1.0, 0.0, -1.0, C.byref(op))
    L.call("hfmi_box_destroy", box)
    gc.collect()
    X = dev(np.random.default_rng(0).standard_normal((45, 2)), ctx)
    Y, Yref = hf.MultiVector(45, 2, ctx=ctx), hf.MultiVector(45, 2, ctx=ctx)
    L.call("hfmi_op_apply", op, X.handle, Y.handle, 0)
    L.call("hfmi_op_destroy", op)
    ref.C.matMvMult(X, Yref)
    assert np.array_equal(Y.to_dense(), Yref.to_dense())
    L.call("hfmi_box_destroy", None)
