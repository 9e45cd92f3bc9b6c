"""GPU suite: orthogonalisation and double pass beyond 256 vectors, up to 2048 (hfmi_chol_wide.hip, qr_chol_wide, the wide back end of double_pass_impl).

  1. the wide Cholesky + inverse kernel family through hfmi_test_chol_wide: Higham's backward bound, the inverse, triangularity,
     bit-identical reruns, the shifted and the failing attempt against the numpy twin;
  2. orthogonalize against the unique thin QR;                     3. the wide route against the narrow one where both exist;
  4. Borthogonalize;   5. double pass on exact-rank operators;      6. double pass against the oracle on the same Omega;
  7. doublePassG against scipy.linalg.eigh(A, B);   8. KLEProjector / PODProjector with rank + oversampling > 256;
  9. the block storage contract at k = 300;   10. limits, and that wide calls leave the narrow path's results bit-identical.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import hippyflow_amd as hf
from hippyflow_amd import _lib as L
from oracle import hippylib_restated as hp_o

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import block_arena as ba  # noqa: E402
from chol_wide_twin import chol_wide, gram_with_condition, qr_shift_rel  # noqa: E402

pytestmark = pytest.mark.gpu

U_ROUND = 1.1102230246251565e-16


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


# ====================================================================== 1. the kernel family
def dev_chol_wide(ctx, G, shift_rel, pivot_tol=0.0):
    G = L.as_f64(G)
    k = G.shape[0]
    R, X, st = np.empty((k, k)), np.empty((k, k)), np.empty(4)
    L.call("hfmi_test_chol_wide", ctx.handle, k, L.ptr(G), float(shift_rel), float(pivot_tol), L.ptr(R), L.ptr(X), L.ptr(st))
    return R, X, {"min_pivot_ratio": st[0], "gram_dev": st[1], "shifted": int(st[2]), "failed": int(st[3])}


@pytest.mark.parametrize("k", [65, 129, 130, 257, 300, 511, 512, 513, 1000, 2048])
def test_chol_wide_against_lapack_and_the_twin(ctx, k):
    G = gram_with_condition(k, 1e4, seed=k)
    shift_rel = qr_shift_rel(2 * k, k)
    R, X, st = dev_chol_wide(ctx, G, shift_rel)
    assert st["shifted"] == 0 and st["failed"] == 0
    gamma = (k + 1) * U_ROUND / (1 - (k + 1) * U_ROUND)
    back = np.linalg.norm(R.T @ R - G)
    inv = np.linalg.norm(R @ X - np.eye(k)) / np.sqrt(k)
    kappa = np.linalg.cond(R)
    print("chol_wide k=%d: ||R^T R - G||_F = %.3e (bound %.3e), ||R X - I||_F / sqrt(k) = %.3e (bound %.3e)"
          % (k, back, gamma * np.trace(G), inv, 8 * k * U_ROUND * kappa))
    assert back <= gamma * np.trace(G)
    assert inv <= 8 * k * U_ROUND * kappa
    assert not np.tril(R, -1).any() and not np.tril(X, -1).any() and np.all(np.diag(R) > 0)
    Rt, Xt, stt = chol_wide(G, shift_rel)
    assert np.abs(R - Rt).max() <= 1e-12 * np.abs(Rt).max() and np.abs(X - Xt).max() <= 1e-11 * np.abs(Xt).max()
    assert abs(st["gram_dev"] - stt["gram_dev"]) <= 1e-12 * stt["gram_dev"]
    assert abs(st["min_pivot_ratio"] - stt["min_pivot_ratio"]) <= 1e-9 * stt["min_pivot_ratio"]
    assert abs(np.linalg.cholesky(G).T - R).max() <= 1e-12 * np.abs(R).max()
    R2, X2, st2 = dev_chol_wide(ctx, G, shift_rel)
    assert np.array_equal(R, R2) and np.array_equal(X, X2) and st == st2


def test_chol_wide_shifted_and_failed(ctx):
    k, n = 300, 600
    Z = np.random.default_rng(0).standard_normal((n, k))
    Z[:, 77] = Z[:, 5]
    G = Z.T @ Z
    shift_rel = qr_shift_rel(n, k)
    R, X, st = dev_chol_wide(ctx, G, shift_rel)
    Rt, Xt, stt = chol_wide(G, shift_rel)
    assert (st["shifted"], st["failed"]) == (1, 0) == (stt["shifted"], stt["failed"])
    Gs = G + shift_rel * np.trace(G) * np.eye(k)
    assert np.linalg.norm(R.T @ R - Gs) <= 1e-13 * np.linalg.norm(Gs)
    assert not np.tril(R, -1).any() and not np.tril(X, -1).any()
    Gn = gram_with_condition(k, 1e4, seed=9)
    Gn[70, 3] = np.nan
    Gi = gram_with_condition(k, 1e4, seed=9)
    Gi[200, 200] = -1.0
    for bad in (Gn, Gi):
        _, _, st = dev_chol_wide(ctx, bad, shift_rel)
        assert st["failed"] == 1 and chol_wide(bad, shift_rel)[2]["failed"] == 1


# ====================================================================== 2. orthogonalize
def graded(rng, N, k, cond):
    """the blocks of test_fuzz_orthogonalize_against_unique_thin_qr"""
    return rng.standard_normal((N, k)) @ np.diag(np.logspace(0, -np.log10(cond), k)) @ np.linalg.qr(rng.standard_normal((k, k)))[0]


QR_CASES = [(257, 257, 1e2), (300, 257, 1e3), (1000, 272, 1e4), (4225, 320, 1e5), (2100, 513, 1e6), (20000, 300, 1e7),
            (3000, 1000, 1e8), (4100, 2048, 1e5), (2048, 2048, 1e3)]


@pytest.mark.parametrize("N,k,cond", QR_CASES)
def test_orthogonalize_against_unique_thin_qr(ctx, N, k, cond):
    Z = graded(np.random.default_rng(N + k), N, k, cond)
    Q = hf.MultiVector.from_dense(Z, ctx=ctx)
    R = Q.orthogonalize()
    Qd = Q.to_dense()
    o = np.linalg.norm(Qd.T @ Qd - np.eye(k)) / np.sqrt(k)
    rec = np.linalg.norm(Qd @ R - Z) / np.linalg.norm(Z)
    print("orthogonalize N=%d k=%d cond=%.0e: %d passes, orthonormality %.3e, reconstruction %.3e" % (N, k, cond, Q.last_qr_passes, o, rec))
    assert o < 1e-12 and rec < 1e-12
    assert np.allclose(np.tril(R, -1), 0) and np.all(np.diag(R) > 0)


def test_orthogonalize_mgs_gives_the_same_factor(ctx):
    N, k = 1000, 272
    Z = graded(np.random.default_rng(N + k), N, k, 1e4)
    Qc, Qm = hf.MultiVector.from_dense(Z, ctx=ctx), hf.MultiVector.from_dense(Z, ctx=ctx)
    Rc, Rm = Qc.orthogonalize(L.QR_CHOL), Qm.orthogonalize(L.QR_MGS)
    assert np.abs(Rc - Rm).max() <= 1e-9 * np.abs(Rm).max()


def test_orthogonalize_duplicated_column(ctx):
    N, k = 1000, 272
    Z = np.random.default_rng(5).standard_normal((N, k))
    Z[:, 100] = Z[:, 3]
    with pytest.raises(hf.HfmiError) as e:
        hf.MultiVector.from_dense(Z, ctx=ctx).orthogonalize(L.QR_CHOL)
    assert e.value.code == -4, e.value
    Q = hf.MultiVector.from_dense(Z, ctx=ctx)
    R = Q.orthogonalize(L.QR_AUTO)
    Qd = Q.to_dense()
    assert R[100, 100] == 0.0 and not Qd[:, 100].any() and np.all(np.isfinite(Qd))
    keep = [j for j in range(k) if j != 100]
    assert np.abs(Qd[:, keep].T @ Qd[:, keep] - np.eye(k - 1)).max() < 1e-10


# ====================================================================== 3. wide == narrow where both exist
@pytest.mark.parametrize("k", [64, 138, 256])
def test_wide_route_equals_narrow_route(ctx, k):
    N = 4225
    Z = graded(np.random.default_rng(k), N, k, 1e4)
    Qn = hf.MultiVector.from_dense(Z, ctx=ctx)
    Rn = Qn.orthogonalize(L.QR_CHOL)
    L.call("hfmi_tuning_set", b"qr_wide_min", 17)
    try:
        Qw = hf.MultiVector.from_dense(Z, ctx=ctx)
        Rw = Qw.orthogonalize(L.QR_CHOL)
    finally:
        L.call("hfmi_tuning_set", b"qr_wide_min", 257)
    dq, dr = np.abs(Qw.to_dense() - Qn.to_dense()).max(), np.abs(Rw - Rn).max()
    print("wide vs narrow k=%d: max |dQ| = %.3e, max |dR| = %.3e" % (k, dq, dr))
    assert dq <= 1e-11 and dr <= 1e-11


# ====================================================================== 4. Borthogonalize
def tridiag_spd(N, seed):
    rng = np.random.default_rng(seed)
    off = -0.3 * (0.5 + rng.random(N - 1))
    main = 1.0 + rng.random(N)
    return sp.diags([off, main, off], [-1, 0, 1], format="csr")


@pytest.mark.parametrize("N,k", [(3000, 300), (4100, 1000)])
def test_borthogonalize(ctx, N, k):
    B = tridiag_spd(N, 1)
    Z = graded(np.random.default_rng(N), N, k, 1e3)
    Q = hf.MultiVector.from_dense(Z, ctx=ctx)
    BQ, R = Q.Borthogonalize(hf.CsrOperator(B, ctx=ctx))
    Qd = Q.to_dense()
    BQd = B @ Qd
    assert np.abs(Qd.T @ BQd - np.eye(k)).max() < 1e-10
    assert np.linalg.norm(BQ.to_dense() - BQd) <= 1e-12 * np.linalg.norm(BQd)
    assert np.allclose(np.tril(R, -1), 0) and np.all(np.diag(R) > 0)
    assert np.linalg.norm(Qd @ R - Z) <= 1e-11 * np.linalg.norm(Z)


# ====================================================================== 5. double pass, exact rank
_EXACT = {}


def exact_rank_problem(N, rank):
    """A = X diag(lam) X^T, X orthonormal, lam geometric over four decades (computed once per shape)"""
    if (N, rank) not in _EXACT:
        rng = np.random.default_rng(N + rank)
        X = np.linalg.qr(rng.standard_normal((N, rank)))[0]
        lam = np.logspace(0, -4, rank)
        A = (X * lam) @ X.T
        _EXACT[N, rank] = (0.5 * (A + A.T), lam)
    return _EXACT[N, rank]


DP_SHAPES = [(1200, 300, 320, 300), (2600, 600, 640, 600), (4200, 2000, 2048, 2000)]
DP_CASES = [(sh, route) for sh in DP_SHAPES for route in ("fused", "generic")] + [(DP_SHAPES[0], "mgs")]


@pytest.mark.parametrize("shape,route", DP_CASES, ids=["%dx%d-%s" % (s[0], s[2], r) for s, r in DP_CASES])
def test_double_pass_exact_rank(ctx, shape, route):
    N, rank, k, r = shape
    A, lam = exact_rank_problem(N, rank)
    op = hf.npToDeviceOperator(A, ctx=ctx)
    Om = hf.MultiVector.from_dense(np.random.default_rng(k).standard_normal((N, k)), ctx=ctx)
    d, U = hf.doublePass(op, Om, r, s=1, fused=(route != "generic"), use_mgs=(route == "mgs"))
    Ud = U.to_dense()
    e = np.max(np.abs(d - lam[:r]) / np.maximum(lam[:r], 1e-7 * lam[0]))
    o = np.linalg.norm(Ud.T @ Ud - np.eye(r))
    res = np.linalg.norm(A @ Ud - Ud * d) / np.linalg.norm(A)
    print("double pass %s N=%d k=%d: eigenvalues %.3e, orthonormality %.3e, residual %.3e" % (route, N, k, e, o, res))
    assert e <= 1e-8 and o < 1e-9 and res < 1e-9


# ====================================================================== 6. double pass against the oracle
@pytest.mark.parametrize("s", [1, 2])
def test_double_pass_against_the_oracle(ctx, s):
    N, n, latent, k, r = 4225, 600, 400, 420, 400
    rng = np.random.default_rng(60 + s)
    U0 = np.linalg.qr(rng.standard_normal((N, latent)))[0]
    X = (rng.standard_normal((n, latent)) * np.exp(-0.02 * np.arange(latent))) @ U0.T
    Om = rng.standard_normal((N, k))
    d, U = hf.doublePass(hf.SnapshotGramOperator(X, ctx=ctx), hf.MultiVector.from_dense(Om, ctx=ctx), r, s=s)
    d_ref, _ = hp_o.double_pass_blas3(lambda W: np.asfortranarray(X.T @ (X @ W) / n), np.asfortranarray(Om), r, s=s)
    big = d_ref > (1e-10 if s == 1 else 1e-5) * d_ref[0]
    e = np.max(np.abs(d[big] - d_ref[big]) / np.maximum(d_ref[big], 1e-7 * d_ref[0]))
    Ud = U.to_dense()
    o = np.linalg.norm(Ud[:, big].T @ Ud[:, big] - np.eye(int(big.sum())))
    print("double pass vs oracle s=%d: %d eigenvalues compared, %.3e, orthonormality %.3e" % (s, int(big.sum()), e, o))
    assert big.sum() >= 200 and e < 1e-8 and o < 1e-9


# ====================================================================== 7. doublePassG
def test_double_pass_g_against_dense_generalized_eigh(ctx):
    N, rank, k, r = DP_SHAPES[0]
    A, _ = exact_rank_problem(N, rank)
    B = tridiag_spd(N, 2)
    w = sl.eigh(A, B.toarray(), eigvals_only=True)[::-1][:r]
    Om = hf.MultiVector.from_dense(np.random.default_rng(7).standard_normal((N, k)), ctx=ctx)
    Bop = hf.CsrOperator(B, ctx=ctx)
    d, U = hf.doublePassG(hf.npToDeviceOperator(A, ctx=ctx), Bop, hf.CsrPCGSolver(B, rel_tol=1e-14, ctx=ctx), Om, r, s=1)
    big = w > 1e-7 * w[0]
    np.testing.assert_allclose(d[big], w[big], rtol=1e-8)
    Ud = U.to_dense()
    assert np.abs(Ud.T @ (B @ Ud) - np.eye(r)).max() < 1e-10


# ====================================================================== 8. projectors
class _Prior:
    pass


def _eig_parity(d, d_ref):
    return np.max(np.abs(np.asarray(d) - d_ref) / np.maximum(d_ref, 1e-7 * d_ref[0]))


def test_kle_projector_with_320_probes(ctx):
    from hippyflow_amd.projectors import _draw_omega
    N, r, p = 2000, 300, 20
    rng = np.random.default_rng(31)
    pts = rng.random((N, 2))
    mdiag = (0.5 + rng.random(N)) / N
    M = sp.diags(mdiag).tocsr()
    Cm = hf.kernel_cov_host(pts, "matern12", 1.0, 0.2)
    prior = _Prior()
    prior.M, prior.C = M, hf.KernelCovarianceOperator(pts, family="matern12", sigma=1.0, ell=0.2, ctx=ctx)
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = r, p, False, False
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    for mode in ("mass", "identity"):
        hf.parRandom.reseed(11)
        Om = np.asfortranarray(_draw_omega(N, r + p, hf.NullCollective(), ctx).to_dense())
        if mode == "mass":
            d_ref, _ = hp_o.double_pass_blas3(lambda W: np.asfortranarray(mdiag[:, None] * (Cm @ (mdiag[:, None] * W))), Om, r, s=1,
                                              apply_B=lambda W: mdiag[:, None] * W, apply_Binv=lambda W: W / mdiag[:, None])
        else:
            d_ref, _ = hp_o.double_pass_blas3(lambda W: np.asfortranarray(Cm @ W), Om, r, s=1)
        hf.parRandom.reseed(11)
        d, dec, enc = kle.construct_input_subspace(mode)
        e = _eig_parity(d, d_ref)
        print("KLE %s with %d probes: eigenvalue parity %.3e" % (mode, r + p, e))
        assert len(d) == r and e <= 1e-8
        V, E = dec.to_dense(), enc.to_dense()
        want = M @ V if mode == "mass" else V
        assert np.linalg.norm(E - want) <= 1e-12 * np.linalg.norm(want)
        gram = V.T @ (M @ V) if mode == "mass" else V.T @ V
        assert np.abs(gram - np.eye(r)).max() < 1e-10


def test_pod_projector_with_300_probes(ctx):
    from hippyflow_amd.projectors import _draw_omega
    N, n, r, p = 3000, 400, 280, 20
    rng = np.random.default_rng(41)
    U0 = np.linalg.qr(rng.standard_normal((N, 350)))[0]
    X = (rng.standard_normal((n, 350)) * np.exp(-0.02 * np.arange(350))) @ U0.T

    class Obs:
        def sample_observables(self, m, prior, noise):
            return X[:m]

    params = hf.PODParameterList()
    params["rank"], params["oversampling"], params["sample_per_process"], params["verbose"] = r, p, n, False
    params["output_directory"] = None
    hf.parRandom.reseed(13)
    Om = np.asfortranarray(_draw_omega(N, r + p, hf.NullCollective(), ctx).to_dense())
    d_ref, _ = hp_o.double_pass_blas3(lambda W: np.asfortranarray(X.T @ (X @ W) / n), Om, r, s=1)
    hf.parRandom.reseed(13)
    pod = hf.PODProjector(Obs(), prior=None, parameters=params, ctx=ctx)
    pod.construct_subspace()
    e = _eig_parity(pod.d, d_ref)
    print("POD with %d probes: eigenvalue parity %.3e" % (r + p, e))
    assert len(pod.d) == r and e <= 1e-8
    Ud = hf.mv_to_dense(pod.U_MV)
    assert np.linalg.norm(Ud.T @ Ud - np.eye(r)) < 1e-9


# ====================================================================== 9. block storage contract
@pytest.mark.parametrize("extra", [0, 96])
def test_block_contract_at_300_vectors(ctx, extra):
    N, k, r, g = 1003, 300, 290, 2
    rng = np.random.default_rng(9)
    ld = ba.round_up(N, 32) + extra
    # hfmi_borth_qr: Q written, nothing else
    Z = graded(rng, N, k, 1e3)
    aq = ba.Arena.wrapped(ctx, N, k + 2 * g, ld=ld)
    q = aq.window(g, k)
    L.call("hfmi_block_upload", q.mv.handle, L.ptr(L.as_f64(Z)), L.LAYOUT_DENSE)
    aq.snapshot()
    R = q.mv.orthogonalize(L.QR_CHOL)
    aq.check(written=[q], what="hfmi_borth_qr at 300 vectors")           # guards untouched, rows N..ld-1 still zero
    Qd = q.mv.to_dense()
    assert np.linalg.norm(Qd.T @ Qd - np.eye(k)) / np.sqrt(k) < 1e-12 and np.linalg.norm(Qd @ R - Z) < 1e-12 * np.linalg.norm(Z)
    # hfmi_double_pass: U written, Omega read-only
    A, lam = exact_rank_problem(N, 280)
    op = hf.npToDeviceOperator(A, ctx=ctx)
    ao, au = ba.Arena.wrapped(ctx, N, k + 2 * g, ld=ld), ba.Arena.wrapped(ctx, N, r + 2 * g, ld=ld)
    om, u = ao.window(g, k), au.window(g, r)
    L.call("hfmi_block_upload", om.mv.handle, L.ptr(L.as_f64(rng.standard_normal((N, k)))), L.LAYOUT_DENSE)
    L.call("hfmi_block_upload", u.mv.handle, L.ptr(np.ones((N, r))), L.LAYOUT_DENSE)
    ao.snapshot()
    au.snapshot()
    d = np.empty(r)
    L.call("hfmi_double_pass", op._op, om.mv.handle, r, 1, 0, L.ptr(d), u.mv.handle)
    ao.check(written=[], what="hfmi_double_pass at 300 probes: Omega")
    au.check(written=[u], what="hfmi_double_pass at 300 probes: U")
    assert np.max(np.abs(d[:280] - lam) / np.maximum(lam, 1e-7)) <= 1e-8


# ====================================================================== 10. limits and reuse
def test_limits(ctx):
    N = 2100
    with pytest.raises(hf.HfmiError) as e:
        hf.MultiVector(N, 2049, ctx=ctx).orthogonalize()
    assert "2048" in str(e.value) and e.value.code == -1
    op = hf.SnapshotGramOperator(np.random.default_rng(0).standard_normal((5, N)), ctx=ctx)
    with pytest.raises(hf.HfmiError) as e:
        hf.doublePass(op, hf.MultiVector(N, 2049, ctx=ctx), 10)
    assert "2048" in str(e.value) and e.value.code == -1
    Om = hf.MultiVector.from_dense(np.random.default_rng(1).standard_normal((N, 257)), ctx=ctx)
    with pytest.raises(hf.HfmiError) as e:
        hf.singlePass(op, Om, 10)
    assert "at most 256" in str(e.value)


def test_wide_calls_leave_the_narrow_path_alone():
    """one context: wide (300), narrow (24), wide (520), narrow again; every narrow result equals the same solve on a fresh context,
    bit for bit -- the wide arena and the wide temporaries share nothing with the narrow path"""
    N = 4225
    rng = np.random.default_rng(17)
    X = (rng.standard_normal((40, 40)) * np.exp(-0.2 * np.arange(40))) @ np.linalg.qr(rng.standard_normal((N, 40)))[0].T
    Om24, Z24 = rng.standard_normal((N, 24)), rng.standard_normal((N, 24))
    A600, _ = exact_rank_problem(1200, 300)

    def narrow(c):
        d, U = hf.doublePass(hf.SnapshotGramOperator(X, ctx=c), hf.MultiVector.from_dense(Om24, ctx=c), 20, s=1)
        Q = hf.MultiVector.from_dense(Z24, ctx=c)
        R = Q.orthogonalize()
        return d, U.to_dense(), Q.to_dense(), R

    def wide(c, k):
        Om = hf.MultiVector.from_dense(np.random.default_rng(k).standard_normal((1200, k)), ctx=c)
        hf.doublePass(hf.npToDeviceOperator(A600, ctx=c), Om, 250, s=1)
        hf.MultiVector.from_dense(np.random.default_rng(k + 1).standard_normal((N, k)), ctx=c).orthogonalize()

    want = narrow(hf.Context(0))
    c = hf.Context(0)
    wide(c, 300)
    first = narrow(c)
    wide(c, 520)
    second = narrow(c)
    for got in (first, second):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
