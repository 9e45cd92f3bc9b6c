"""GPU tests of the single-pass randomized eigensolvers (singlePass / singlePassG, hippylib randomizedEigensolver), the
one-workgroup LU solve behind them, the streamed sketch and the projectors' opt-in route."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

import hippyflow_amd as hf                     # noqa: E402  (a broken import of the package is a failure, not a skip)
from hippyflow_amd import _lib as L            # noqa: E402
from hippyflow_amd import projectors as P      # noqa: E402
from hippyflow_amd import workloads            # noqa: E402
from oracle import hippylib_restated as hp_o    # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from single_pass_restated import single_pass, single_pass_g, subspace_angle  # noqa: E402

SIZES = [1, 2, 17, 30, 64, 74, 84, 138, 139, 200, 256]


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def _omega(N, m, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((N, m)))


def _snapshots(n, N, decay, seed):
    rng = np.random.default_rng(seed)
    U0, _ = np.linalg.qr(rng.standard_normal((n, n)))
    W0, _ = np.linalg.qr(rng.standard_normal((N, n)))
    return ((U0 * np.exp(-decay * np.arange(n))) @ W0.T) * np.sqrt(n)      # (n, N): one snapshot per row


def _eig_rel(d, d_ref):
    return np.abs(np.asarray(d) - np.asarray(d_ref)).max() / np.abs(d_ref).max()


# ------------------------------------------------------------------ 1. the LU solve kernel
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("kind", ["random", "graded"])
def test_small_solve_matches_numpy(ctx, m, kind):
    rng = np.random.default_rng(m)
    W = rng.standard_normal((m, m))
    if kind == "graded":
        W = W * np.exp(-0.04 * np.arange(m))[None, :] * np.exp(-0.02 * np.arange(m))[:, None]
    Z = rng.standard_normal((m, m))
    X = hf.small_solve(W, Z, ctx)
    ref = np.linalg.solve(W, Z)
    cond = np.linalg.cond(W)
    resid = np.linalg.norm(W @ X - Z) / (np.linalg.norm(W) * np.linalg.norm(X))
    assert resid <= 1e-12 * cond
    assert np.linalg.norm(X - ref) / np.linalg.norm(ref) <= 1e-12 * cond


def test_small_solve_rejects_singular_and_nonfinite(ctx):
    rng = np.random.default_rng(3)
    W = rng.standard_normal((40, 40))
    W[:, 7] = W[:, 2]
    with pytest.raises(hf.HfmiError, match="singular"):
        hf.small_solve(W, np.eye(40), ctx)
    W = rng.standard_normal((40, 40))
    W[3, 3] = np.inf
    with pytest.raises(hf.HfmiError, match="non-finite"):
        hf.small_solve(W, np.eye(40), ctx)
    with pytest.raises(hf.HfmiError, match="overflowed"):          # finite input whose solution overflows
        hf.small_solve(np.diag([1e-200, 1.0]), np.full((2, 2), 1e200), ctx)


# ------------------------------------------------------------------ 2. exact-rank standard problem
@pytest.mark.parametrize("m", [30, 74, 138])
def test_exact_rank_hep_snapshot_gram(ctx, m):
    N = 20000
    X = _snapshots(m, N, 0.05, m)
    A = hf.SnapshotGramOperator(X)
    Omega = hf.MultiVector.from_dense(_omega(N, m, 100 + m))
    d, U = hf.singlePass(A, Omega, m)
    G = X @ X.T / m
    lam, u = np.linalg.eigh(G)
    lam, u = lam[::-1], u[:, ::-1]
    assert _eig_rel(d, lam) <= 1e-10
    Ud = U.to_dense()
    assert np.abs(Ud.T @ Ud - np.eye(m)).max() <= 1e-12
    V = X.T @ u[:, :10] / np.sqrt(m * lam[:10])
    assert subspace_angle(Ud[:, :10], V) <= 1e-8


# ------------------------------------------------------------------ 3. exact-rank generalized problem
def test_exact_rank_ghep_jtj_mass(ctx):
    nx = ny = 63
    N = nx * ny
    ndata, q = 10, 6
    m = ndata * q
    rng = np.random.default_rng(4)
    J = rng.standard_normal((ndata, q, N)) * np.exp(-0.1 * np.arange(q))[None, :, None] / np.sqrt(N)
    A = hf.MeanJTJfromDataOperator(J)
    M = workloads.grid_mass_matrix(nx, ny).tocsr()
    Mop = hf.CsrOperator(M)
    Minv = hf.CsrPCGSolver(M)
    Omega = hf.MultiVector.from_dense(_omega(N, m, 5))
    k = m - 4
    d, U = hf.singlePassG(A, Mop, Minv, Omega, k)
    Jf = J.reshape(m, N)
    Ad = Jf.T @ Jf / ndata
    lam = sla.eigh(Ad, M.toarray(), eigvals_only=True, subset_by_index=[N - m, N - 1])[::-1]
    assert _eig_rel(d, lam[:k]) <= 1e-9
    Ud = U.to_dense()
    assert np.abs(Ud.T @ (M @ Ud) - np.eye(k)).max() <= 1e-10


# ------------------------------------------------------------------ 4. device == restatement
def _decaying_dense(N, n, rate, seed):
    rng = np.random.default_rng(seed)
    W, _ = np.linalg.qr(rng.standard_normal((N, n)))
    lam = np.exp(-rate * np.arange(n))
    return (W * lam) @ W.T


def _operators(N, seed):
    """(device operator, dense matrix) pairs with decaying spectra shaped like configs 2-4"""
    rng = np.random.default_rng(seed)
    out = {}
    X = _snapshots(120, N, 0.06, seed)                                   # config 3: snapshot Gram
    out["snapshot_gram"] = (hf.SnapshotGramOperator(X), X.T @ X / 120)
    J = rng.standard_normal((16, 8, N)) * np.exp(-0.25 * np.arange(8))[None, :, None] * np.exp(-0.08 * np.arange(16))[:, None, None]
    Jf = J.reshape(128, N)
    out["jtj"] = (hf.MeanJTJfromDataOperator(J), Jf.T @ Jf / 16)           # config 4: mean J^T J
    Cd = _decaying_dense(N, 200, 0.05, seed + 1)                          # config 2: explicit covariance
    out["dense"] = (hf.npToDeviceOperator(Cd), Cd)
    dg = np.exp(-0.05 * np.arange(N))
    out["csr"] = (hf.CsrOperator(sp.diags(dg, format="csr")), np.diag(dg))
    out["host"] = (hf.HostCallbackOperator(lambda W, Cd=Cd: Cd @ W, N), Cd)
    return out


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("name", ["snapshot_gram", "jtj", "dense", "csr", "host"])
def test_device_equals_restatement(ctx, name, s):
    N, m, k = 1500, 40, 10
    op, Ad = _operators(N, 21)[name]
    Om = _omega(N, m, 7)
    d, U = hf.singlePass(op, hf.MultiVector.from_dense(Om), k, s=s)
    d_r, U_r = single_pass(Ad, Om, k, s=s)
    assert _eig_rel(d, d_r) <= 1e-10
    assert subspace_angle(U.to_dense()[:, :5], U_r[:, :5]) <= 1e-8


@pytest.mark.parametrize("s", [1, 2])
def test_device_equals_restatement_generalized_and_generic_route(ctx, s):
    N, m, k = 1200, 40, 10
    M, _ = _fem(N)
    Cd = _decaying_dense(N, 200, 0.05, 9)
    Om = _omega(N, m, 8)
    Mop, Minv = hf.CsrOperator(M), hf.CsrPCGSolver(M)
    d, U = hf.singlePassG(hf.npToDeviceOperator(Cd), Mop, Minv, hf.MultiVector.from_dense(Om), k, s=s)
    Md = M.toarray()
    d_r, U_r = single_pass_g(Cd, Md, None, Om, k, s=s)
    assert _eig_rel(d, d_r) <= 1e-10
    assert subspace_angle(U.to_dense()[:, :5], U_r[:, :5], B=Md) <= 1e-8
    # the generic route (operator without a device form) computes the same
    d2, U2 = hf.singlePass(hf.npToDeviceOperator(Cd), hf.MultiVector.from_dense(Om), k, s=s, fused=False)
    d2_r, U2_r = single_pass(Cd, Om, k, s=s)
    assert _eig_rel(d2, d2_r) <= 1e-10
    assert subspace_angle(U2.to_dense()[:, :5], U2_r[:, :5]) <= 1e-8


def _fem(N):
    h = 1.0 / (N - 1)
    main = np.full(N, 4 * h / 6)
    main[[0, -1]] = 2 * h / 6
    M = sp.diags([np.full(N - 1, h / 6), main, np.full(N - 1, h / 6)], [-1, 0, 1], format="csr")
    kd = np.full(N, 2 / h)
    kd[[0, -1]] = 1 / h
    K = sp.diags([np.full(N - 1, -1 / h), kd, np.full(N - 1, -1 / h)], [-1, 0, 1], format="csr")
    return M, K


# ------------------------------------------------------------------ 5. application count
@pytest.mark.parametrize("s", [1, 2, 3])
def test_operator_applied_s_times(ctx, s):
    N, m = 800, 20
    Ad = _decaying_dense(N, 60, 0.1, 2)
    calls = []

    def fn(W):
        calls.append(W.shape[1])
        return Ad @ W

    op = hf.HostCallbackOperator(fn, N)
    Om = hf.MultiVector.from_dense(_omega(N, m, 1))
    hf.singlePass(op, Om, 8, s=s)
    assert len(calls) == s
    calls.clear()
    hf.doublePass(op, Om, 8, s=s)
    assert len(calls) == s + 1


# ------------------------------------------------------------------ 6. projectors
def _kle_prior(N):
    M, K = _fem(N)
    A = (M + 0.02 * K).toarray()
    Rm = A @ np.diag(1.0 / np.asarray(M.sum(axis=1)).ravel()) @ A
    Rm = 0.5 * (Rm + Rm.T)

    class Prior:
        pass

    prior = Prior()
    prior.M = M
    prior.R = sp.csr_matrix(Rm)
    prior.Rsolver = hp_o.SparseLUSolver(sp.csr_matrix(Rm))       # host black box, like PETSc in the reference
    prior.Rsolver.N = N
    return prior, M


def _spy_solvers(monkeypatch):
    """records (name, result, result of a direct call with the same arguments) of every randomized solve a projector makes"""
    seen = []
    real = {"singlePass": hf.singlePass, "singlePassG": hf.singlePassG, "doublePass": hf.doublePass, "doublePassG": hf.doublePassG}

    def spy(name):
        def f(*args, **kw):
            out = real[name](*args, **kw)
            again = real[name](*args, **kw)                       # a direct call with the same arguments
            seen.append((name, out, again))
            return out
        return f

    for name in real:
        monkeypatch.setattr(P, name, spy(name))
    return seen


def _same(out, again):
    return np.array_equal(out[0], again[0]) and np.array_equal(out[1].to_dense(), again[1].to_dense())


@pytest.mark.parametrize("orthogonality", ["mass", "identity"])
def test_kle_projector_single_pass_route(ctx, monkeypatch, orthogonality):
    N, r = 600, 20
    prior, M = _kle_prior(N)
    seen = _spy_solvers(monkeypatch)
    params = hf.KLEParameterList()
    params["rank"], params["verbose"], params["save_and_plot"] = r, False, False
    kle = hf.KLEProjector(prior, parameters=params)
    hf.parRandom.reseed(5)
    d_dp, dec_dp, _ = kle.construct_input_subspace(orthogonality)
    assert [s[0] for s in seen] == ["doublePassG" if orthogonality == "mass" else "doublePass"]
    seen.clear()
    kle.randomized_eigensolver = "single_pass"
    hf.parRandom.reseed(5)
    d, dec, enc = kle.construct_input_subspace(orthogonality)
    name, out, again = seen[0]
    assert name == ("singlePassG" if orthogonality == "mass" else "singlePass")
    assert np.array_equal(d, out[0]) and np.array_equal(out[0], again[0])
    assert np.array_equal(dec.to_dense(), again[1].to_dense())
    V, E = dec.to_dense(), enc.to_dense()
    if orthogonality == "mass":
        assert np.linalg.norm(V.T @ (M @ V) - np.eye(r)) / np.sqrt(r) < 1e-10
        assert np.linalg.norm(E - M @ V) / np.linalg.norm(M @ V) < 1e-10
    else:
        assert np.linalg.norm(V.T @ V - np.eye(r)) / np.sqrt(r) < 1e-10
    assert np.abs(d[:5] - d_dp[:5]).max() / d_dp[0] < 1e-2                  # same probe block, close spectra


class _Obs:
    """Jacobian samples of a small AS problem (the interface ActiveSubspaceProjector reads) and observables for POD"""

    def __init__(self, N, q, ns, seed):
        rng = np.random.default_rng(seed)
        P0, _ = np.linalg.qr(rng.standard_normal((N, q)))
        self.J = np.einsum("ioc,tc->iot", rng.standard_normal((ns, q, q)) * np.exp(-0.3 * np.arange(q)), P0)
        self.N, self.q = N, q
        self.X = (rng.standard_normal((ns, 30)) * np.exp(-0.2 * np.arange(30))) @ rng.standard_normal((30, N)) / np.sqrt(N)

    def jacobian_data(self, n):
        return self.J[:n]

    def input_dimension(self):
        return self.N

    def output_dimension(self):
        return self.q

    def sample_observables(self, n, prior, control):
        return self.X[:n]


@pytest.mark.parametrize("prior_preconditioned", [False, True])
def test_active_subspace_projector_single_pass_route(ctx, monkeypatch, prior_preconditioned):
    N, q, ns, r = 600, 12, 10, 8
    prior, _ = _kle_prior(N)
    obs = _Obs(N, q, ns, 3)
    seen = _spy_solvers(monkeypatch)
    params = hf.ActiveSubspaceParameterList()
    params["rank"], params["oversampling"], params["samples_per_process"] = r, 4, ns
    params["verbose"], params["save_and_plot"] = False, False
    asp = hf.ActiveSubspaceProjector(obs, prior, parameters=params)
    asp.randomized_eigensolver = "single_pass"
    hf.parRandom.reseed(7)
    d, dec, enc = asp.construct_input_subspace(prior_preconditioned=prior_preconditioned)
    name, out, again = seen[-1]
    assert name == ("singlePassG" if prior_preconditioned else "singlePass")
    assert np.array_equal(d, out[0]) and _same(out, again)
    V = dec.to_dense()
    if prior_preconditioned:
        Rm = prior.R.toarray()
        assert np.linalg.norm(V.T @ (Rm @ V) - np.eye(r)) / np.sqrt(r) < 1e-7      # R: cond ~1e9 (as in the KLE 'prior' test)
        assert np.linalg.norm(enc.to_dense() - Rm @ V) / np.linalg.norm(Rm @ V) < 1e-10
    else:
        assert np.linalg.norm(V.T @ V - np.eye(r)) / np.sqrt(r) < 1e-10
    # the range of mean J^T J has dimension q = r + p: the sketch is exact
    Jf = obs.J.reshape(-1, N)
    if not prior_preconditioned:
        lam = np.linalg.eigvalsh(Jf.T @ Jf / ns)[::-1][:r]
        assert np.abs(d - lam).max() / lam[0] < 1e-9
    seen.clear()
    asp.randomized_eigensolver = "double_pass"
    hf.parRandom.reseed(7)
    asp.construct_input_subspace(prior_preconditioned=prior_preconditioned)
    assert seen[-1][0] == ("doublePassG" if prior_preconditioned else "doublePass")


def test_pod_projector_single_pass_route(ctx, monkeypatch):
    N, ns, r = 700, 40, 10
    obs = _Obs(N, 5, ns, 4)
    seen = _spy_solvers(monkeypatch)
    params = hf.PODParameterList()
    params["rank"], params["oversampling"], params["sample_per_process"] = r, 20, ns      # r + p = rank of the snapshots
    params["verbose"] = False
    pod = hf.PODProjector(obs, object(), parameters=params)
    pod.randomized_eigensolver = "single_pass"
    hf.parRandom.reseed(2)
    pod.construct_subspace()
    name, out, again = seen[-1]
    assert name == "singlePass" and _same(out, again)
    lam = np.linalg.eigvalsh(obs.X @ obs.X.T / ns)[::-1][:r]           # rank 30 <= r + p: the sketch is exact
    assert np.abs(pod.d - lam).max() / lam[0] < 1e-9
    pod.randomized_eigensolver = "double_pass"
    hf.parRandom.reseed(2)
    pod.construct_subspace()
    assert seen[-1][0] == "doublePass"


def test_projector_default_is_bit_identical_double_pass(ctx):
    assert hf.ActiveSubspaceProjector.randomized_eigensolver == "double_pass"
    assert hf.KLEProjector.randomized_eigensolver == "double_pass"
    assert hf.BoundaryRestrictedKLEProjector.randomized_eigensolver == "double_pass"
    assert hf.PODProjector.randomized_eigensolver == "double_pass"
    N, r = 500, 12
    prior, _ = _kle_prior(N)
    params = hf.KLEParameterList()
    params["rank"], params["verbose"], params["save_and_plot"] = r, False, False
    kle = hf.KLEProjector(prior, parameters=params)
    hf.parRandom.reseed(9)
    d1, v1, _ = kle.construct_input_subspace("identity")
    hf.parRandom.reseed(9)
    Om = P._draw_omega(N, r + params["oversampling"], hf.NullCollective(), ctx)
    d2, v2 = hf.doublePass(kle.C, Om, r, s=1)
    assert np.array_equal(d1, d2) and np.array_equal(v1.to_dense(), v2.to_dense())


# ------------------------------------------------------------------ 7. streamed sketch
def _batches(X, sizes):
    i = 0
    for b in sizes:
        yield X[i:i + b]
        i += b


def test_streamed_sketch_snapshots(ctx):
    N, m, k = 5000, 40, 12
    sizes = [1, 7, 64, 13, 1, 40, 25]
    X = _snapshots(sum(sizes), N, 0.05, 3)
    Om = hf.MultiVector.from_dense(_omega(N, m, 4))
    sk = hf.StreamedSketch(Om, kind="snapshots")
    for b in _batches(X, sizes):
        sk.add(b)
    with pytest.raises(ValueError):
        hf.StreamedSketch(Om).add(np.zeros((3, N + 1)))
    A = hf.SnapshotGramOperator(X)
    Y_ref = hf.MultiVector(N, m)
    A.matMvMult(Om, Y_ref)
    Yr = Y_ref.to_dense()
    assert np.linalg.norm(sk.sketch().to_dense() - Yr) / np.linalg.norm(Yr) <= 1e-13
    d, U = sk.singlePass(k)
    d_ref, U_ref = hf.singlePass(A, Om, k)
    assert _eig_rel(d, d_ref) <= 1e-11
    assert subspace_angle(U.to_dense()[:, :6], U_ref.to_dense()[:, :6]) <= 1e-8


def test_streamed_sketch_jacobians_with_noise(ctx):
    N, m, k, q, n = 3000, 30, 10, 6, 25
    rng = np.random.default_rng(6)
    J = rng.standard_normal((n, q, N)) * np.exp(-0.3 * np.arange(q))[None, :, None]
    G = np.diag(1.0 + np.arange(q) * 0.5)
    Om = hf.MultiVector.from_dense(_omega(N, m, 2))
    sk = hf.StreamedSketch(Om, kind="jacobian", noise_cov_inv=G)
    for i in range(n):
        sk.add(J[i])
    with pytest.raises(ValueError):
        sk.add(J[0][:q - 1])
    A = hf.MeanJTJfromDataOperator(J, noise_cov_inv=G)
    Y_ref = hf.MultiVector(N, m)
    A.matMvMult(Om, Y_ref)
    Yr = Y_ref.to_dense()
    assert np.linalg.norm(sk.sketch().to_dense() - Yr) / np.linalg.norm(Yr) <= 1e-13
    d, U = sk.singlePass(k)
    d_ref, U_ref = hf.singlePass(A, Om, k)
    assert _eig_rel(d, d_ref) <= 1e-11
    assert subspace_angle(U.to_dense()[:, :5], U_ref.to_dense()[:, :5]) <= 1e-8


def test_generalized_generic_route_and_streamed_sketch_equal_the_restatement(ctx):
    N, m, k, n = 1000, 30, 8, 60
    M, _ = _fem(N)
    Md = M.toarray()
    X = _snapshots(n, N, 0.08, 12)
    Ad = X.T @ X / n
    Om = _omega(N, m, 13)
    d_r, U_r = single_pass_g(Ad, Md, None, Om, k)
    Mop, Minv = hf.CsrOperator(M), hf.CsrPCGSolver(M)

    class HostA:                                 # no device form: the generic route
        def matMvMult_np(self, W):
            return Ad @ W

    d, U = hf.singlePassG(hf.HostCallbackOperator(HostA(), N), Mop, Minv, hf.MultiVector.from_dense(Om), k, fused=False)
    assert _eig_rel(d, d_r) <= 1e-10
    assert subspace_angle(U.to_dense()[:, :5], U_r[:, :5], B=Md) <= 1e-8
    Omv = hf.MultiVector.from_dense(Om)
    sk = hf.StreamedSketch(Omv, kind="snapshots")
    for b in _batches(X, [3, 17, 40]):
        sk.add(b)
    d2, U2 = sk.singlePassG(k, Mop, Minv)
    assert _eig_rel(d2, d_r) <= 1e-10
    U2d = U2.to_dense()
    assert subspace_angle(U2d[:, :5], U_r[:, :5], B=Md) <= 1e-8
    assert np.abs(U2d.T @ (Md @ U2d) - np.eye(k)).max() <= 1e-10


# ------------------------------------------------------------------ 8. two ranks sharing one GPU
def test_two_ranks_single_pass_and_streamed_sketch(tmp_path):
    from hippyflow_amd.launch import spawn_ranks
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "gpu_single_pass_worker.py")
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="60")
    assert spawn_ranks([worker, str(tmp_path)], 2, env=env, timeout=600) == 0
    rs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]
    r0 = rs[0]
    for rank, res in enumerate(rs):
        assert int(res["size"]) == 2 and int(res["rank"]) == rank
        for s in (1, 2):
            np.testing.assert_array_equal(res["d_coll_s%d" % s], r0["d_coll_s%d" % s])      # every rank holds the same result
            # s = 1: Wt = Omega^T Q is a square Gaussian-like sketch, and its solve amplifies the rank reduction's round-off
            # (~1e-16 on the sketch, checked below) by cond(Wt): measured 7e-12 here, 2.6e-12 between single and double pass on
            # ONE rank.  s = 2 (Wt = (A Omega)^T Q, well conditioned) meets 1e-12.
            assert _eig_rel(res["d_coll_s%d" % s], r0["d_all_s%d" % s]) <= (1e-11 if s == 1 else 1e-12)
            assert _eig_rel(res["d_dp_coll_s%d" % s], r0["d_dp_all_s%d" % s]) <= 1e-12      # the double pass, same operator
            assert subspace_angle(res["U_coll_s%d" % s][:, :4], r0["U_all_s%d" % s][:, :4]) <= 1e-8
        Ya = r0["sketch_all"]
        assert np.linalg.norm(res["sketch_coll"] - Ya) / np.linalg.norm(Ya) <= 1e-12
        assert _eig_rel(res["d_sketch_coll"], r0["d_sketch_all"]) <= 1e-12
        assert _eig_rel(res["d_sketch_coll"], r0["d_stored_all"]) <= 1e-12
        assert subspace_angle(res["U_sketch_coll"][:, :5], r0["U_stored_all"][:, :5]) <= 1e-8


# ------------------------------------------------------------------ 9. error paths
def test_error_paths(ctx):
    N = 1000
    Ad = _decaying_dense(N, 80, 0.1, 3)
    op = hf.npToDeviceOperator(Ad)
    Om = hf.MultiVector.from_dense(_omega(N, 20, 3))
    with pytest.raises(hf.HfmiError, match="rank"):
        hf.singlePass(op, Om, 21)
    with pytest.raises(hf.HfmiError, match="s must be"):
        hf.singlePass(op, Om, 10, s=0)
    with pytest.raises(hf.HfmiError, match="256"):
        hf.singlePass(op, hf.MultiVector.from_dense(_omega(N, 257, 1)), 10)
    d = np.empty(10)
    U_bad = hf.MultiVector(N, 9)
    with pytest.raises(hf.HfmiError, match="U must be"):
        L.call("hfmi_single_pass", op._op, Om.handle, 10, 1, 0, L.ptr(d), U_bad.handle)
    dup = _omega(N, 20, 3)
    dup[:, 5] = dup[:, 3]
    with pytest.raises(hf.HfmiError, match="rank-deficient"):
        hf.singlePass(op, hf.MultiVector.from_dense(dup), 10)
