"""GPU parity tests, path level: operators, the randomized double pass and the projector classes against the
oracle (same Omega, same operator samples) and the golden vectors produced by the reference's own code.

Tolerances: eigenvalue relative error and subspace angle as stated per test (north star: eigenvalue
rel-err < 1e-6 vs the reference path); invariants with the tolerances of the reference's tests
(hippyflow/test/test_KLEProjector.py:92-129,183-217; test_derivativeSubspace.py:92-102;
test_PODProjector.py:154-208)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

hf = pytest.importorskip("hippyflow_amd")
from oracle import hippyflow_restated as hf_o   # noqa: E402
from oracle import hippylib_restated as hp_o    # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _fem(N):
    h = 1.0 / (N - 1)
    main = np.full(N, 4 * h / 6)
    main[[0, -1]] = 2 * h / 6
    M = sp.diags([np.full(N - 1, h / 6), main, np.full(N - 1, h / 6)], [-1, 0, 1], format="csr")
    kd = np.full(N, 2 / h)
    kd[[0, -1]] = 1 / h
    K = sp.diags([np.full(N - 1, -1 / h), kd, np.full(N - 1, -1 / h)], [-1, 0, 1], format="csr")
    return M, K


def _snapshots(n, N, rate, seed):
    rng = np.random.default_rng(seed)
    U0, _ = np.linalg.qr(rng.standard_normal((n, n)))
    W0, _ = np.linalg.qr(rng.standard_normal((N, n)))
    return (U0 * np.exp(-rate * np.arange(n))) @ W0.T


def _csr(g, N):
    return sp.csr_matrix((g["M_data"], g["M_indices"], g["M_indptr"]), shape=(N, N))


# ------------------------------------------------------------------ operators (a2, a3, a4, a9)
def test_snapshot_gram_operator(ctx):
    X = _snapshots(40, 3001, 0.2, 0)
    W = np.random.default_rng(1).standard_normal((3001, 9))
    op = hf.SnapshotGramOperator(X)
    Y = hf.MultiVector(3001, 9)
    op.matMvMult(hf.MultiVector.from_dense(W), Y)
    assert rel(Y.to_dense(), hf_o.snapshot_gram_block(X, W)) < 1e-13
    # column protocol: mult(x, y) on vectors
    x, y = hf.Vector(), hf.Vector()
    op.init_vector(x, 1)
    op.init_vector(y, 0)
    x.set_local(W[:, 0])
    op.mult(x, y)
    assert rel(y.get_local(), hf_o.snapshot_gram_block(X, W[:, :1])[:, 0]) < 1e-13
    lro = hf.LowRankOperator(np.ones(40) / 40, hf.MultiVector.from_vectors(X))
    lro.matMvMult(hf.MultiVector.from_dense(W), Y)
    assert rel(Y.to_dense(), hf_o.snapshot_gram_block(X, W)) < 1e-13


def test_mean_jtj_operator_matches_reference_golden(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "mean_jtj.npz"))
    J, x = g["J"], g["x"]
    for gamma, want in ((None, g["y"]), (g["Gamma_inv"], g["y_gamma"])):
        op = hf.MeanJTJfromDataOperator(J, prior=None, noise_cov_inv=gamma)
        assert (op.ndata, op.r, op.dM) == J.shape
        Y = hf.MultiVector(J.shape[2], x.shape[1])
        op.matMvMult(hf.MultiVector.from_dense(x), Y)
        np.testing.assert_allclose(Y.to_dense(), want, rtol=1e-12, atol=1e-12)   # reference's own output
        xv, yv = hf.Vector(), hf.Vector()
        op.init_vector(xv, 1)
        op.init_vector(yv, 0)
        xv.set_local(x[:, 2])
        op.mult(xv, yv)
        np.testing.assert_allclose(yv.get_local(), want[:, 2], rtol=1e-12, atol=1e-12)


def test_mean_jtj_jjt_larger(ctx):
    rng = np.random.default_rng(2)
    J = rng.standard_normal((12, 20, 2500)) * np.exp(-0.1 * np.arange(20))[None, :, None]
    W = rng.standard_normal((2500, 17))
    Y = hf.MultiVector(2500, 17)
    hf.MeanJTJfromDataOperator(J).matMvMult(hf.MultiVector.from_dense(W), Y)
    assert rel(Y.to_dense(), hf_o.mean_jtj_block(J, W)) < 1e-13
    Wq = rng.standard_normal((20, 6))
    Yq = hf.MultiVector(20, 6)
    hf.MeanJJTfromDataOperator(J).matMvMult(hf.MultiVector.from_dense(Wq), Yq)
    assert rel(Yq.to_dense(), hf_o.mean_jjt_block(J, Wq)) < 1e-13


def test_dense_sym_and_mcm_operator(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "kle_and_consumers.npz"))
    N = g["x"].shape[0]
    M = _csr(g, N)
    C = hf.npToDeviceOperator(g["Cov"])
    op = hf.MassPreconditionedCovarianceOperator(C, hf.CsrOperator(M))
    x, y = hf.Vector(), hf.Vector()
    op.init_vector(x, 0)
    op.init_vector(y, 0)
    x.set_local(g["x"])
    op.mult(x, y)
    np.testing.assert_allclose(y.get_local(), g["mcm"], rtol=1e-12)                 # reference's own output
    # consumers of the eigenvectors
    U = hf.MultiVector.from_dense(g["U"])
    ppp = hf.PriorPreconditionedProjector(U, hf.CsrOperator(M), lambda v, dim: v.init(N))
    ppp.mult(x, y)
    np.testing.assert_allclose(y.get_local(), g["prior_precond_proj"], rtol=1e-11, atol=1e-13)
    V = hf.MultiVector.from_dense(g["V"])
    lrr = hf.LowRankRectangularOperator(U, g["s"], V)
    x13, y13 = hf.Vector(), hf.Vector()
    x13.init(13)
    y13.init(13)
    x13.set_local(g["x13"])
    lrr.mult(x13, y)
    np.testing.assert_allclose(y.get_local(), g["lowrank_mult"], rtol=1e-11, atol=1e-13)
    lrr.transpmult(x, y13)
    np.testing.assert_allclose(y13.get_local(), g["lowrank_transpmult"], rtol=1e-11, atol=1e-13)


def test_dense_sym_large(ctx):
    rng = np.random.default_rng(3)
    N, k = 3000, 84
    A = rng.standard_normal((N, N))
    Cm = A @ A.T / N + np.eye(N)
    W = rng.standard_normal((N, k))
    Y = hf.MultiVector(N, k)
    hf.npToDeviceOperator(Cm).matMvMult(hf.MultiVector.from_dense(W), Y)
    assert rel(Y.to_dense(), Cm @ W) < 1e-13


def test_host_callback_and_summed_list(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "operators.npz"))
    Js, x13 = g["Js"], g["x13"]
    ops = [hf.HostCallbackOperator(hp_o.DenseOperator(Ji.T @ Ji), 13) for Ji in Js]
    x, y = hf.Vector(), hf.Vector()
    x.init(13)
    y.init(13)
    x.set_local(x13)
    ops[0].mult(x, y)
    np.testing.assert_allclose(y.get_local(), g["jtj"], rtol=1e-12)
    hf.SummedListOperator(ops, average=True).mult(x, y)
    np.testing.assert_allclose(y.get_local(), g["summed_avg"], rtol=1e-12)          # reference's own output

    class Boom:
        def mult(self, x, y):
            raise ValueError("boom")

    with pytest.raises(ValueError):
        hf.HostCallbackOperator(Boom(), 13).mult(x, y)


def test_collective_operator_null(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "collectives.npz"))
    nc = hf.NullCollective()
    assert nc.size() == int(g["null_size"]) and nc.rank() == int(g["null_rank"])
    with pytest.raises(NotImplementedError):
        nc.allReduce(1.0, "max")
    X = _snapshots(8, 500, 0.3, 4)
    op = hf.CollectiveOperator(hf.SnapshotGramOperator(X), nc, mpi_op="avg")
    W = np.random.default_rng(5).standard_normal((500, 4))
    Y = hf.MultiVector(500, 4)
    hf.MatMvMult(op, hf.MultiVector.from_dense(W), Y)
    assert rel(Y.to_dense(), hf_o.snapshot_gram_block(X, W)) < 1e-13


# ------------------------------------------------------------------ double pass (a5, a6)
def _check_eigs(d, U, d_ref, U_ref, tol_d, tol_angle, lead, apply_B=None):
    assert hp_o.eig_rel_err(d, d_ref) < tol_d, "eigenvalues: %g" % hp_o.eig_rel_err(d, d_ref)
    ang = hp_o.principal_angle(np.asfortranarray(U[:, :lead]), np.asfortranarray(U_ref[:, :lead]), apply_B)
    assert ang < tol_angle, "subspace angle %g" % ang


@pytest.mark.parametrize("fused", [True, False])
def test_double_pass_config1_vs_oracle(ctx, fused):
    """Config 1 shape: N=4225, 256 snapshots, r=20, p=10, sigma_j = exp(-0.35 j)."""
    n, N, r, p = 256, 4225, 20, 10
    X = _snapshots(n, N, 0.35, 0)
    Omega = np.asfortranarray(np.random.default_rng(1).standard_normal((N, r + p)))
    d_ref, U_ref = hp_o.double_pass(hf_o.SnapshotGramOperator(X), Omega, r, s=1)
    op = hf.SnapshotGramOperator(X)
    d, U = hf.doublePass(op, hf.MultiVector.from_dense(Omega), r, s=1, fused=fused)
    Ud = U.to_dense()
    # same Omega, same operator: agreement far below the 1e-6 target (lambda_20/lambda_1 = 1.7e-6)
    _check_eigs(d, Ud, d_ref, U_ref, 1e-8, 1e-6, 12)
    assert np.linalg.norm(Ud.T @ Ud - np.eye(r)) / np.sqrt(r) < 1e-10            # test_KLEProjector.py:183-196
    AU = hf_o.snapshot_gram_block(X, Ud)
    assert np.linalg.norm(AU - Ud * d) / np.linalg.norm(AU) < 1e-4                # :198-217
    exact = np.linalg.eigvalsh(X @ X.T / n)[::-1][:r]
    assert hp_o.eig_rel_err(d, exact) < 1e-5                                      # randomization error only


def test_double_pass_mgs_route_and_power_iterations(ctx):
    X = _snapshots(60, 2000, 0.3, 2)
    Omega = np.asfortranarray(np.random.default_rng(3).standard_normal((2000, 25)))
    op = hf.SnapshotGramOperator(X)
    for s in (1, 2):
        d_ref, U_ref = hp_o.double_pass(hf_o.SnapshotGramOperator(X), Omega, 15, s=s)
        d, U = hf.doublePass(op, hf.MultiVector.from_dense(Omega), 15, s=s, use_mgs=True)
        _check_eigs(d, U.to_dense(), d_ref, U_ref, 1e-7, 1e-6, 8)
        d2, U2 = hf.doublePass(op, hf.MultiVector.from_dense(Omega), 15, s=s)
        _check_eigs(d2, U2.to_dense(), d_ref, U_ref, 1e-7, 1e-6, 8)


def test_rank_deficient_snapshot_set(ctx):
    """Fewer snapshots than probe vectors: A has rank n < k; the reference's MGS zeroes dependent
    columns and the trailing Ritz values are 0."""
    X = _snapshots(12, 900, 0.2, 5)
    Omega = np.asfortranarray(np.random.default_rng(6).standard_normal((900, 20)))
    d_ref, _ = hp_o.double_pass(hf_o.SnapshotGramOperator(X), Omega, 16, s=1)
    d, U = hf.doublePass(hf.SnapshotGramOperator(X), hf.MultiVector.from_dense(Omega), 16, s=1)
    np.testing.assert_allclose(d[:12], d_ref[:12], rtol=1e-8)
    assert np.all(np.abs(d[12:]) < 1e-12 * d[0])


@pytest.mark.parametrize("binv", ["pcg", "host_lu"])
def test_double_pass_g_kle_mass(ctx, binv):
    """KLE 'mass' mode: M C M v = lambda M v (KLEProjector.py:146-168) with the reference test's
    invariants (test_KLEProjector.py:91-129) and oracle parity on the same Omega."""
    rng = np.random.default_rng(4)
    N, r, p = 1500, 24, 10
    M, K = _fem(N)
    A = (M + 0.02 * K).toarray()
    R = A @ np.diag(1.0 / np.asarray(M.sum(axis=1)).ravel()) @ A
    Cm = np.linalg.inv(R)
    Cm = 0.5 * (Cm + Cm.T)
    Omega = np.asfortranarray(rng.standard_normal((N, r + p)))
    KLE_o = hf_o.MassPreconditionedCovarianceOperator(hp_o.DenseOperator(Cm), hp_o.SparseOperator(M))
    d_ref, V_ref = hp_o.double_pass_g(KLE_o, hp_o.SparseOperator(M), hp_o.SparseLUSolver(M), Omega, r, s=1)
    Mop = hf.CsrOperator(M)
    KLE = hf.MassPreconditionedCovarianceOperator(hf.npToDeviceOperator(Cm), Mop)
    Msolver = hf.CsrPCGSolver(M) if binv == "pcg" else hp_o.SparseLUSolver(M)      # device CG or host black box
    d, V = hf.doublePassG(KLE, Mop, Msolver, hf.MultiVector.from_dense(Omega), r, s=1)
    Vd = V.to_dense()
    _check_eigs(d, Vd, d_ref, V_ref, 1e-7, 1e-5, 10, lambda W: M @ W)
    assert np.linalg.norm(Vd.T @ (M @ Vd) - np.eye(r)) / np.sqrt(r) < 1e-10
    MCMV = M @ (Cm @ (M @ Vd))
    assert np.linalg.norm(MCMV - (M @ Vd) * d) / np.linalg.norm(MCMV) < 1e-4
    # generic (host-orchestrated) route gives the same answer
    d2, V2 = hf.doublePassG(KLE, Mop, Msolver, hf.MultiVector.from_dense(Omega), r, s=1, fused=False)
    _check_eigs(d2, V2.to_dense(), d_ref, V_ref, 1e-7, 1e-5, 10, lambda W: M @ W)


def test_boundary_restricted_kle_projector(ctx):
    """BoundaryRestrictedKLEProjector (KLEProjector.py:336-435): doublePassG with the boundary mass matrix M_b
    inside the operator (M_b C M_b) and its invertible completion B = M_b + I_interior as the inner product.
    Checked against the dense generalized eigenproblem and the oracle's doublePassG on the same Omega."""
    import scipy.linalg as sla
    nx = 24
    N = nx * nx
    idx = np.arange(N).reshape(nx, nx)
    ring = np.concatenate([idx[0, :-1], idx[:-1, -1], idx[-1, :0:-1], idx[:0:-1, 0]])   # boundary nodes, in order
    h = 1.0 / (nx - 1)
    Mb = sp.lil_matrix((N, N))
    for a, b in zip(ring, np.roll(ring, -1)):                                            # 1-D P1 mass per boundary edge
        Mb[a, a] += h / 3
        Mb[b, b] += h / 3
        Mb[a, b] += h / 6
        Mb[b, a] += h / 6
    Mb = Mb.tocsr()
    M, K = _fem(N)
    Rm = ((M + 0.05 * K) @ sp.diags(1.0 / np.asarray(M.sum(axis=1)).ravel()) @ (M + 0.05 * K)).toarray()
    Rm = 0.5 * (Rm + Rm.T)

    class Prior:
        pass

    prior = Prior()
    prior.Rsolver = hp_o.SparseLUSolver(sp.csr_matrix(Rm))
    prior.Rsolver.N = N
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"] = 12, 8
    with pytest.raises(ValueError):
        hf.BoundaryRestrictedKLEProjector(prior, None, parameters=params)
    proj = hf.BoundaryRestrictedKLEProjector(prior, None, parameters=params, boundary_mass=Mb)
    B = proj.make_boundary_restricted_mass_matrix(fill_nullspace=True)
    interior = np.setdiff1d(np.arange(N), ring)
    assert np.allclose(B.diagonal()[interior], 1.0) and np.allclose((B - Mb).diagonal()[ring], 0.0)   # :382-394
    hf.parRandom.reseed(7)
    d, dec, enc = proj.construct_input_subspace()
    V, E = dec.to_dense(), enc.to_dense()
    r = 12
    Bd = B.toarray()
    assert np.linalg.norm(V.T @ Bd @ V - np.eye(r)) / np.sqrt(r) < 1e-10
    assert rel(E, Mb @ V) < 1e-12
    Cm = np.linalg.inv(Rm)
    A_dense = Mb @ Cm @ Mb.toarray()
    A_dense = 0.5 * (A_dense + A_dense.T)
    w = sla.eigh(A_dense, Bd, eigvals_only=True)[::-1][:r]
    np.testing.assert_allclose(d[:4], w[:4], rtol=1e-6)                                 # randomization error only
    np.testing.assert_allclose(d[:8], w[:8], rtol=1e-3)
    # Ritz values from below, against the spectrum of the operator the solve applies: C through the prior's own sparse LU.  Rm has
    # a condition number near 4e9, so the dense inverse above is another rounding of C: its leading eigenvalues differ from these by
    # a few 1e-9 and move with the host BLAS thread count, more than the 1e-10 of the bound.
    CMb = np.empty((N, N))
    prior.Rsolver.solve(CMb, Mb.toarray())
    A_applied = Mb @ CMb
    A_applied = 0.5 * (A_applied + A_applied.T)
    w_applied = sla.eigh(A_applied, Bd, eigvals_only=True)[::-1][:r]
    assert np.all(d[:r] <= w_applied[:r] * (1 + 1e-10))
    # same Omega through the oracle's doublePassG
    hf.parRandom.reseed(7)
    Omega = hf.MultiVector(N, 20)
    hf.parRandom.normal(1.0, Omega)
    d_ref, U_ref = hp_o.double_pass_g(hp_o.DenseOperator(A_dense), hp_o.SparseOperator(B), hp_o.SparseLUSolver(B),
                                      np.asfortranarray(Omega.to_dense()), r, s=1)
    np.testing.assert_allclose(d, d_ref, rtol=1e-8)


# ------------------------------------------------------------------ projectors
@pytest.mark.parametrize("method", ["hep", "ghep", "inverse_ghep"])
@pytest.mark.parametrize("shifted", [True, False])
def test_pod_from_data_matches_reference_golden(ctx, golden_dir, shifted, method):
    """All three methods of PODProjectorFromData.construct_subspace against the reference's own outputs (the
    reference runs numpy eigh for 'hep' and ARPACK for the two generalized forms; the device serves all three
    through the n x n Gram problem they share)."""
    g = np.load(os.path.join(golden_dir, "pod_from_data.npz"))
    N, r = int(g["N"]), int(g["r"])
    M = _csr(g, N)
    d, phi, Mphi, shift = hf.PODProjectorFromData(None, M).construct_subspace(g["u_data"].copy(), r, shifted=shifted, method=method)
    tag = "%s_%d" % (method, int(shifted))
    np.testing.assert_allclose(shift, g["shift_" + tag], atol=1e-14)
    np.testing.assert_allclose(d, g["d_" + tag], rtol=1e-7, atol=1e-12 * g["d_" + tag][0])
    cos = np.abs(np.einsum("ij,ij->j", phi[:, :6], M @ g["phi_" + tag][:, :6]))
    np.testing.assert_allclose(cos, 1.0, atol=1e-8)
    eye = np.eye(r)
    assert np.linalg.norm(eye - phi.T @ Mphi) / np.linalg.norm(eye) < 1e-8        # test_PODProjector.py:154-168
    assert np.linalg.norm(M @ phi - Mphi) / np.linalg.norm(Mphi) < 1e-8           # :170-174
    assert (not np.allclose(shift, 0)) == shifted                                 # :176-186
    with pytest.raises(ValueError):
        hf.PODProjectorFromData(None, M).construct_subspace(g["u_data"].copy(), r, method="lanczos")


def test_pod_projector_class(ctx, tmp_path):
    X = _snapshots(100, 2500, 0.3, 8)
    params = hf.PODParameterList()
    assert params["rank"] == 20 and params["oversampling"] == 10 and params["sample_per_process"] == 100
    params["verbose"] = False
    params["output_directory"] = str(tmp_path) + "/"

    class Obs:
        def sample_observables(self, n, prior, noise):
            return X[:n]

    hf.parRandom.reseed(7)
    pod = hf.PODProjector(Obs(), prior=None, parameters=params)
    pod.construct_subspace()
    exact = np.linalg.eigvalsh(X @ X.T / 100)[::-1][:20]
    assert hp_o.eig_rel_err(pod.d[:10], exact[:10]) < 1e-6
    saved = np.load(os.path.join(str(tmp_path), "POD_projector.npy"))
    assert saved.shape == (2500, 20)
    np.testing.assert_array_equal(saved, hf.mv_to_dense(pod.U_MV))
    np.testing.assert_array_equal(np.load(os.path.join(str(tmp_path), "POD_d.npy")), pod.d)
    try:                                               # the spectrum plot the reference leaves beside them (PODProjector.py:386-389)
        import matplotlib  # noqa: F401
        assert os.path.getsize(os.path.join(str(tmp_path), "POD_eigenvalues_20.pdf")) > 1000
    except ImportError:
        pass


def test_projector_defaults_are_per_instance(ctx):
    """The reference's `parameters = PODParameterList()` default argument is ONE list shared by every projector built without
    one; here each instance gets its own (test_errors raises `rank` in place)."""
    a, b = hf.PODProjector(object(), object(), ctx=ctx), hf.PODProjector(object(), object(), ctx=ctx)
    a.parameters['rank'] = 7
    assert b.parameters['rank'] == 20 and a.collective is not b.collective and a.collective.size() == 1
    c, d = hf.ActiveSubspaceProjector(object(), object(), ctx=ctx), hf.ActiveSubspaceProjector(object(), object(), ctx=ctx)
    c.parameters['rank'] = 9
    assert d.parameters['rank'] == 128 and d.collective.rank() == 0


def test_kle_projector_class(ctx):
    """The reference's KLE test, mass and identity modes (test_KLEProjector.py:80-217)."""
    N = 1200
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
    params = hf.KLEParameterList()
    assert params["rank"] == 128 and params["input_decoder_name"] == "KLE_decoder"
    params["rank"], params["verbose"], params["save_and_plot"] = 30, False, False
    kle = hf.KLEProjector(prior, parameters=params)
    d, dec, enc = kle.construct_input_subspace("mass")
    V, E = dec.to_dense(), enc.to_dense()
    r = 30
    assert kle.M_orthogonal is True
    assert np.linalg.norm(V.T @ (M @ V) - np.eye(r)) / np.sqrt(r) < 1e-10         # :96-99
    assert rel(E, M @ V) < 1e-10                                                  # :101-108
    Cm = np.linalg.inv(Rm)
    MCMV = M @ (Cm @ (M @ V))
    assert np.linalg.norm(MCMV - (M @ V) * d) / np.linalg.norm(MCMV) < 1e-4       # :110-129
    d2, dec2, _ = kle.construct_input_subspace("identity")
    V2 = dec2.to_dense()
    assert np.linalg.norm(V2.T @ V2 - np.eye(r)) / np.sqrt(r) < 1e-10             # :183-196
    CV = Cm @ V2
    assert np.linalg.norm(CV - V2 * d2) / np.linalg.norm(CV) < 1e-4               # :198-217
    # orthogonality='prior' (KLESubspaceConstructorSLEPc, KLEProjector.py:285-334): the eigenpairs of A v = mu M v scaled to
    # decoder = v / mu, eigenvalues 1 / mu^2, encoder = R decoder = the dominant eigenpairs of M u = lambda R u, u^T R u = 1;
    # here by the randomized generalized solve instead of Krylov-Schur
    import scipy.linalg as sla
    d3, dec3, enc3 = kle.construct_input_subspace("prior")
    V3, E3 = dec3.to_dense(), enc3.to_dense()
    assert kle.M_orthogonal is False and kle.R_orthogonal is True
    # (R has entries of 2e6 and a condition number of ~1e9: V^T R V is orthonormal to eps * cond, not to 1e-10 as with B = M)
    assert np.linalg.norm(V3.T @ (Rm @ V3) - np.eye(r)) / np.sqrt(r) < 1e-7
    assert rel(E3, Rm @ V3) < 1e-10
    lam = sla.eigh(M.toarray(), Rm, eigvals_only=True)[::-1][:r]
    assert np.all(np.diff(d3) <= 0) and np.max(np.abs(d3[:10] - lam[:10]) / lam[:10]) < 1e-6
    CMV3 = Cm @ (M @ V3)                                         # M u = lambda R u  <=>  C M u = lambda u
    res3 = np.linalg.norm(CMV3 - V3 * d3) / np.linalg.norm(CMV3)
    assert res3 < 1e-4, res3
    mu = 1.0 / np.sqrt(d3)                                       # the reference's sqrt-precision eigenvalues: (v = mu u)^T M v = 1
    assert np.abs(np.diag((V3 * mu).T @ (M @ (V3 * mu))) - 1.0).max() < 1e-3
    # projection-error test of the basis (KLEProjector.py:202-282) on prior-like samples x = C^{1/2}-ish noise
    kle.construct_input_subspace("mass")
    Xs = (np.linalg.cholesky(Cm + 1e-12 * np.eye(N)) @ np.random.default_rng(3).standard_normal((N, 12))).T
    avg, std = kle.test_errors(ranks=[5, 15, 30], samples=Xs)
    assert avg.shape == (3,) and avg[0] > avg[1] > avg[2] > 0 and np.all(std >= 0)
    Vm = kle.V_KLE.to_dense()
    E = Xs.T - Vm[:, :15] @ (Vm[:, :15].T @ (M @ Xs.T))
    np.testing.assert_allclose(avg[1], np.mean(np.linalg.norm(E, axis=0) / np.linalg.norm(Xs.T, axis=0)), rtol=1e-8)


def test_active_subspace_batched_equals_serialized(ctx, tmp_path):
    """The reference's own AS test: with identical Omega and samples the batched (device operator over
    stored Jacobians) and the serialized (host black box re-applied every pass) constructions give the
    same eigenvalues, ||d_batch - d_serial||_2 < 1e-12 (test_derivativeSubspace.py:92-102) -- here 1e-9
    relative because the two routes sum in different orders on different hardware (GPU MFMA vs host BLAS)
    and the prior solve amplifies that by cond(R)."""
    rng = np.random.default_rng(9)
    ns, q, N = 16, 30, 1800
    P, _ = np.linalg.qr(rng.standard_normal((N, q)))
    J = np.einsum("ioc,tc->iot", rng.standard_normal((ns, q, q)) * np.exp(-0.15 * np.arange(q))[None, None, :], P)
    M, K = _fem(N)
    A = (M + 1e-6 * K)                                   # cond(R) ~ 1e3: solves do not amplify summation-order noise
    Rm = (A @ sp.diags(1.0 / np.asarray(M.sum(axis=1)).ravel()) @ A).tocsr()

    class Prior:
        pass

    prior = Prior()
    prior.R = Rm
    prior.Rsolver = hp_o.SparseLUSolver(Rm)

    class Obs:
        def jacobian_data(self, n):
            return J[:n]

        def input_dimension(self):
            return N

        def output_dimension(self):
            return q

        def jtj_host_operator(self):
            return hf_o.MeanJTJOperator(J)      # host black box with the reference's protocol

        def jjt_host_operator(self):
            class JJT:
                def matMvMult_np(self, W):
                    return hf_o.mean_jjt_block(J, W)
            return JJT()

    results = {}
    for serialized in (False, True):
        params = hf.ActiveSubspaceParameterList()
        assert params["rank"] == 128 and params["samples_per_process"] == 64 and params["serialized_sampling"] is True
        params["rank"], params["oversampling"], params["samples_per_process"] = 20, 8, ns
        params["serialized_sampling"], params["verbose"], params["store_Omega"] = serialized, False, True
        params["output_directory"] = str(tmp_path) + "/"
        hf.parRandom.reseed(123)
        asp = hf.ActiveSubspaceProjector(Obs(), prior, parameters=params)
        d, dec, enc = asp.construct_input_subspace(prior_preconditioned=True)
        dn, decn, _ = asp.construct_output_subspace()
        results[serialized] = (d, dec.to_dense(), enc.to_dense(), dn, asp.Omega_GN.to_dense())
    d_b, V_b, E_b, dn_b, Om_b = results[False]
    d_s, V_s, E_s, dn_s, Om_s = results[True]
    np.testing.assert_array_equal(Om_b, Om_s)
    assert np.linalg.norm(d_b - d_s) / np.linalg.norm(d_b) < 1e-9
    assert np.linalg.norm(dn_b - dn_s) / np.linalg.norm(dn_b) < 1e-9
    # oracle parity on the same Omega, R-orthonormality, encoder = R decoder
    d_ref, V_ref = hp_o.double_pass_g(hf_o.MeanJTJOperator(J), hp_o.SparseOperator(Rm), hp_o.SparseLUSolver(Rm),
                                      np.asfortranarray(Om_b), 20, s=1)
    assert hp_o.eig_rel_err(d_b, d_ref) < 1e-7
    assert np.linalg.norm(V_b.T @ (Rm @ V_b) - np.eye(20)) / np.sqrt(20) < 1e-10
    assert rel(E_b, Rm @ V_b) < 1e-10
    saved = np.load(os.path.join(str(tmp_path), "AS_%d_input_decoder.npy" % ns))
    assert saved.shape == (N, 20)
    assert os.path.exists(os.path.join(str(tmp_path), "AS_%d_d_GN.npy" % ns))
    assert os.path.exists(os.path.join(str(tmp_path), "AS_%d_output_decoder.npy" % ns))


# ------------------------------------------------------------------ size-independent properties at larger sizes
def test_large_pod_properties(ctx):
    """Down-scaled config 3 (N=50,000, 512 snapshots, r=128, p=10) generated on the device: invariants only."""
    from hippyflow_amd import workloads
    wl = workloads.pod_workload(N=50000, n=512, latent=192, rate=0.05, seed=3)
    hf.parRandom.reseed(5)
    Omega = hf.MultiVector(50000, 138)
    hf.parRandom.normal(1.0, Omega)
    d, U = hf.doublePass(wl.operator, Omega, 128, s=1)
    G = U.dot_mv(U)
    assert np.linalg.norm(G - np.eye(128)) / np.sqrt(128) < 1e-10
    AU = hf.MultiVector(50000, 128)
    wl.operator.matMvMult(U, AU)
    Rn = hf.MultiVector(AU)
    hf.MvDSmatMult(U, np.diag(d), Rn)
    Rn.axpy(-1.0, AU)
    assert np.linalg.norm(Rn.norm()) / np.linalg.norm(AU.norm()) < 1e-4
    assert hp_o.eig_rel_err(d[:64], wl.exact_eigenvalues[:64]) < 1e-6            # known spectrum of the synthetic set


# ------------------------------------------------------------------ RCCL plumbing on one GPU (world size 1)
@pytest.mark.timeout(1200)      # the first `import torch` on a fresh box can take minutes while the image pages in
def test_torch_collective_on_device_blocks(ctx):
    """The multi-GPU route end to end with a 1-rank nccl group: zero-copy tensor view of a block, in-place
    all-reduce / bcast in HBM, and the fused solve's post-apply hook (the driver runs the real 2/4/8-GPU case)."""
    torch = pytest.importorskip("torch")
    import torch.distributed as dist
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        coll = hf.TorchCollective()
        assert coll.size() == 1 and coll.rank() == 0
        rng = np.random.default_rng(0)
        D = rng.standard_normal((1003, 5))
        mv = hf.MultiVector.from_dense(D)
        t, stage = coll._tensor_of(mv)
        assert stage is None and t.data_ptr() == mv.device_ptr(), "zero-copy view of the block's HBM"
        assert coll.allReduce(mv, "avg") is mv
        np.testing.assert_array_equal(mv.to_dense(), D)
        coll.allReduce(mv, "sum")
        coll.bcast(mv, root=0)
        np.testing.assert_array_equal(mv.to_dense(), D)
        v = mv[2]
        coll.allReduce(v, "avg")
        np.testing.assert_array_equal(v.get_local(), D[:, 2])
        assert coll.allReduce(2.5, "avg") == 2.5 and coll.allReduce(3, "sum") == 3
        with pytest.raises(NotImplementedError):
            coll.allReduce(mv, "max")
        # fused double pass with the all-reduce hook vs the plain operator
        X = _snapshots(50, 2000, 0.3, 1)
        Omega = hf.MultiVector.from_dense(np.random.default_rng(2).standard_normal((2000, 18)))
        op = hf.SnapshotGramOperator(X)
        d0, U0 = hf.doublePass(op, Omega, 12)
        d1, U1 = hf.doublePass(hf.CollectiveOperator(op, coll, mpi_op="avg"), Omega, 12)
        d2, U2 = hf.doublePass(hf.MatrixMultCollectiveOperator(op, coll, mpi_op="avg"), Omega, 12, fused=False)
        np.testing.assert_array_equal(d0, d1)
        np.testing.assert_array_equal(U0.to_dense(), U1.to_dense())
        np.testing.assert_allclose(d2, d0, rtol=1e-12)
    finally:
        if created:
            dist.destroy_process_group()


# ------------------------------------------------------------------ BASELINE sizes: size-independent properties
def test_full_size_config3_pod_properties(ctx):
    """Config 3 at full size (2048 snapshots x N = 5e5, r = 128, p = 10; 8.2 GB of snapshots generated in HBM):
    orthonormality, eigen-residual and the known spectrum of the synthetic snapshot set."""
    from hippyflow_amd import workloads
    wl = workloads.pod_workload(N=500000, n=2048, latent=256, rate=0.05, seed=3)
    hf.parRandom.reseed(1)
    Omega = hf.MultiVector(500000, 138)
    hf.parRandom.normal(1.0, Omega)
    d, U = hf.doublePass(wl.operator, Omega, 128, s=1)
    assert np.linalg.norm(U.dot_mv(U) - np.eye(128)) / np.sqrt(128) < 1e-10
    AU = hf.MultiVector(500000, 128)
    wl.operator.matMvMult(U, AU)
    Rn = hf.MultiVector(AU)
    hf.MvDSmatMult(U, np.diag(d), Rn)
    Rn.axpy(-1.0, AU)
    assert np.linalg.norm(Rn.norm()) / np.linalg.norm(AU.norm()) < 1e-4
    assert hp_o.eig_rel_err(d[:40], wl.exact_eigenvalues[:40]) < 1e-6        # randomization error grows towards r
    assert hp_o.eig_rel_err(d[:100], wl.exact_eigenvalues[:100]) < 1e-2
    # linearity of the operator application at full size: A(2 W1 - 3 W2) = 2 A W1 - 3 A W2
    W1, W2 = hf.MultiVector(500000, 16), hf.MultiVector(500000, 16)
    hf.parRandom.normal(1.0, W1)
    hf.parRandom.normal(1.0, W2)
    Y1, Y2, Y3 = hf.MultiVector(500000, 16), hf.MultiVector(500000, 16), hf.MultiVector(500000, 16)
    wl.operator.matMvMult(W1, Y1)
    wl.operator.matMvMult(W2, Y2)
    W3 = hf.MultiVector(W1)
    W3.scale(2.0)
    W3.axpy(-3.0, W2)
    wl.operator.matMvMult(W3, Y3)
    Y3.axpy(-2.0, Y1)
    Y3.axpy(3.0, Y2)
    assert np.linalg.norm(Y3.norm()) < 1e-12 * np.linalg.norm(Y1.norm())


def test_full_size_config2_kle_properties(ctx):
    """Config 2 at full size (explicit dense covariance on N = 1e5 points, 80 GB in HBM; r = 64, p = 20): the invariants
    of the reference's own KLE test (test_KLEProjector.py:91-129: M-orthonormality 1e-10, encoder = M decoder,
    eigen-residual) and the factored oracle on the same Omega."""
    from hippyflow_amd import workloads
    import scipy.sparse.linalg as spla
    wl = workloads.kle_workload(400, 250, latent=256, rate=0.08, seed=2)
    N, r, k = wl.N, 64, 84
    A = hf.MassPreconditionedCovarianceOperator(wl.C_operator, wl.M_operator)
    B, Binv = wl.M_operator, hf.CsrPCGSolver(wl.M_operator.csr)
    hf.parRandom.reseed(1)
    Omega = hf.MultiVector(N, k)
    hf.parRandom.normal(1.0, Omega)
    d, U = hf.doublePassG(A, B, Binv, Omega, r, s=1)
    assert np.all(np.diff(d) <= 0) and d[-1] > 0
    MU = hf.MultiVector(N, r)
    hf.MatMvMult(B, U, MU)
    assert np.linalg.norm(U.dot_mv(MU) - np.eye(r)) / np.sqrt(r) < 1e-10, "U^T M U = I"
    Md = wl.M @ U.to_dense()
    assert rel(MU.to_dense(), Md) < 1e-13, "encoder = M decoder"
    AU = hf.MultiVector(N, r)
    A.matMvMult(U, AU)
    Rn = hf.MultiVector(AU)
    hf.MvDSmatMult(MU, np.diag(d), Rn)                    # A U - M U diag(d)
    Rn.axpy(-1.0, AU)
    # the residual of a randomized solve is set by the discarded tail: lambda_85 / lambda_1 = exp(-0.08 * 84) = 1.2e-3
    # for this synthetic spectrum (the reference's 1e-4 is for its faster-decaying prior covariance)
    assert np.linalg.norm(Rn.norm()) / np.linalg.norm(AU.norm()) < 1e-2
    # the same solve by the CPU restatement, operator in factored form
    F, lam, M = wl.F_host, wl.lam, wl.M
    lu = spla.splu(M.tocsc())
    d_ref, _ = hp_o.double_pass_blas3(lambda W: np.asfortranarray(M @ (F @ (lam[:, None] * (F.T @ (M @ W))))),
                                      np.asfortranarray(Omega.to_dense()), r, apply_B=lambda W: M @ W,
                                      apply_Binv=lambda W: np.asfortranarray(lu.solve(np.ascontiguousarray(W))))
    assert hp_o.eig_rel_err(d, d_ref) < 1e-9


def test_config4_shard_of_eight_gpu_run(ctx):
    """The per-GPU share of config 4 at 8 GPUs (64 of 512 samples, N = 2e5, 10 GB of Jacobians): the local
    operator against the factored host form of the same samples, plus prior-free double-pass invariants."""
    from hippyflow_amd import workloads
    N, q = 200000, 100
    wl = workloads.as_workload(N, 64, q=q, latent=q, rate=0.06, seed=4, first_sample=3 * 64, ns_total=512)
    hf.parRandom.reseed(2)
    W = hf.MultiVector(N, 74)
    hf.parRandom.normal(1.0, W)
    Y = hf.MultiVector(N, 74)
    wl.operator.matMvMult(W, Y)
    P = wl.P.to_dense()
    H = np.einsum("ioc,iod->cd", wl.A, wl.A) / 64          # mean A_i^T A_i of THIS shard (samples 192..255)
    ref = P @ (H @ (P.T @ W.to_dense()))
    assert rel(Y.to_dense(), ref) < 1e-12
    A0 = workloads.sample_factor(4, 3 * 64, q, q) * wl.s    # the shard starts at global sample 192
    np.testing.assert_array_equal(wl.A[0], A0)
    d, U = hf.doublePass(wl.operator, W, 64, s=1)
    assert np.linalg.norm(U.dot_mv(U) - np.eye(64)) / 8 < 1e-10
    d_ref, _ = hp_o.double_pass_blas3(lambda Z: np.asfortranarray(P @ (H @ (P.T @ Z))), np.asfortranarray(W.to_dense()), 64)
    assert hp_o.eig_rel_err(d, d_ref) < 1e-9


@pytest.mark.parametrize("N,k,r", [(1, 1, 1), (5, 3, 2), (31, 4, 4), (33, 256, 200), (100, 20, 20)])
def test_ragged_and_extreme_shapes(ctx, N, k, r):
    """Edge cases: vectors shorter than one 32-row stage, a single probe vector, the maximum block width (256)."""
    rng = np.random.default_rng(N + k)
    n = max(1, min(N, 7))
    X = rng.standard_normal((n, N))
    kk = min(k, N)                      # more probe vectors than the space has dimensions is rank deficient by construction
    rr = min(r, kk)
    Omega = np.asfortranarray(rng.standard_normal((N, kk)))
    d, U = hf.doublePass(hf.SnapshotGramOperator(X), hf.MultiVector.from_dense(Omega), rr, s=1)
    d_ref, U_ref = hp_o.double_pass(hf_o.SnapshotGramOperator(X), Omega, rr, s=1)
    nz = d_ref > 1e-12 * max(d_ref[0], 1e-300)
    np.testing.assert_allclose(d[nz], d_ref[nz], rtol=1e-8)
    assert np.all(np.abs(d[~nz]) <= 1e-10 * max(d_ref[0], 1e-300))
    with pytest.raises(AssertionError):
        hf.doublePass(hf.SnapshotGramOperator(X), hf.MultiVector.from_dense(Omega), kk + 1)


@pytest.mark.parametrize("gamma", [False, True])
def test_gram_form_rayleigh_quotient_equals_literal(ctx, gamma):
    """T = scale (X Q)^T Gamma (X Q) (default, fused route) against the reference's literal T = (A Q)^T Q."""
    rng = np.random.default_rng(21)
    J = rng.standard_normal((9, 12, 1500)) * np.exp(-0.2 * np.arange(12))[None, :, None]
    Gam = None
    if gamma:
        Gm = rng.standard_normal((12, 12))
        Gam = Gm @ Gm.T + 12 * np.eye(12)
    Omega = np.asfortranarray(rng.standard_normal((1500, 10)))
    op = hf.MeanJTJfromDataOperator(J, noise_cov_inv=Gam)
    d_ref, U_ref = hp_o.double_pass(hf_o.MeanJTJOperator(J, Gam), Omega, 7)
    d1, U1 = hf.doublePass(op, hf.MultiVector.from_dense(Omega), 7)
    d2, U2 = hf.doublePass(op, hf.MultiVector.from_dense(Omega), 7, literal_T=True)
    d3, U3 = hf.doublePass(op, hf.MultiVector.from_dense(Omega), 7, fused=False)
    for d, U in ((d1, U1), (d2, U2), (d3, U3)):
        np.testing.assert_allclose(d, d_ref, rtol=1e-10)
        assert hp_o.principal_angle(np.asfortranarray(U.to_dense()[:, :5]), U_ref[:, :5]) < 1e-7


def test_accuracy_enhanced_svd_of_a_jacobian(ctx):
    """randomized SVD of a per-sample Jacobian (activeSubspaceProjector.py:813-834,1026)."""
    rng = np.random.default_rng(31)
    q, N, k, p = 40, 3000, 12, 8
    Uj, _ = np.linalg.qr(rng.standard_normal((q, q)))
    Vj, _ = np.linalg.qr(rng.standard_normal((N, q)))
    sj = np.exp(-0.5 * np.arange(q))
    J = (Uj * sj) @ Vj.T
    Omega = np.asfortranarray(rng.standard_normal((N, k + p)))
    U_ref, d_ref, V_ref = hp_o.accuracy_enhanced_svd(lambda W: J @ W, lambda Y: J.T @ Y, Omega, k, s=1)
    U, d, V = hf.accuracyEnhancedSVD(hf.DenseJacobianOperator(J), hf.MultiVector.from_dense(Omega), k, s=1)
    Ud, Vd = U.to_dense(), V.to_dense()
    np.testing.assert_allclose(d, d_ref, rtol=1e-9)
    np.testing.assert_allclose(d, sj[:k], rtol=1e-6)                                    # true singular values
    assert np.linalg.norm(Ud.T @ Ud - np.eye(k)) < 1e-10 and np.linalg.norm(Vd.T @ Vd - np.eye(k)) < 1e-10
    assert hp_o.principal_angle(np.asfortranarray(Ud[:, :8]), U_ref[:, :8]) < 1e-6
    assert hp_o.principal_angle(np.asfortranarray(Vd[:, :8]), V_ref[:, :8]) < 1e-6
    assert np.linalg.norm((Ud * d) @ Vd.T - J) / np.linalg.norm(J) < 2 * sj[k] / sj[0] + 1e-8


def test_projection_errors_and_downstream_formats(ctx, tmp_path):
    """projection-error test of a basis and the loader side of the on-disk formats."""
    N, n = 1500, 60
    X = _snapshots(n, N, 0.25, 12)
    params = hf.PODParameterList()
    params["verbose"], params["rank"], params["output_directory"] = False, 20, str(tmp_path) + "/"

    class Obs:
        def sample_observables(self, k, prior, noise):
            return X[:k]

    params["sample_per_process"] = n
    hf.parRandom.reseed(3)
    pod = hf.PODProjector(Obs(), None, parameters=params)
    pod.construct_subspace()
    avg, std = pod.test_output_errors(ranks=[5, 10, 20])
    U = pod.U_MV.to_dense()
    for r, a in zip((5, 10, 20), avg):
        E = X.T - U[:, :r] @ (U[:, :r].T @ X.T)
        np.testing.assert_allclose(a, np.mean(np.linalg.norm(E, axis=0) / np.linalg.norm(X.T, axis=0)), rtol=1e-9)
    assert avg[0] > avg[1] > avg[2] and np.all(std >= 0)
    ranks, avg2, _ = hf.projection_error_test(pod.U_MV, X, ranks=[None, 3], d=pod.d, cut_off=pod.d[10])
    assert ranks == [3]                                           # ranks beyond the numerical rank are dropped
    # the training-side loader accepts what the projectors save
    proj = hf.get_projectors(str(tmp_path) + "/", pod_tolerance=pod.d[7] * 0.999)
    assert set(proj) == {"POD"} and proj["POD"].shape == (N, 8)
    proj["KLE"] = np.random.default_rng(0).standard_normal((N, 6))
    pin, pout = hf.modify_projectors(proj, "kle", "pod")
    assert pin.shape == (N, 6) and pout.shape == (N, 8)
    G = pin.T @ pin
    np.testing.assert_allclose(G, np.eye(6) * G[0, 0], atol=1e-12 * G[0, 0])          # orthogonal, equal norms
    np.testing.assert_allclose(np.linalg.norm(pin), 1.0 / (N / (32.0 * 6)), rtol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(pout), 1.0, rtol=1e-12)


# ------------------------------------------------------------------ derivative training data
def test_derivative_datasets_from_stored_jacobians(ctx, tmp_path):
    """The three derivative products DataGenerator dumps (dataGenerator.py:163-191) from stored Jacobians, and the
    .npz files compress_dataset writes (:634-655) with the key names the training scripts load."""
    rng = np.random.default_rng(5)
    ndata, q, N, r_in, r_out, rM = 6, 24, 1500, 9, 7, 5
    # numerically rank-rM Jacobians (graded singular values + 1e-11 noise): the randomized SVD with rM probe vectors
    # and no oversampling -- what the reference runs -- is then exact to the noise level
    left = np.linalg.qr(rng.standard_normal((ndata, q, rM)))[0] * np.logspace(1, -1, rM)
    J = left @ np.linalg.qr(rng.standard_normal((N, rM)))[0].T + 1e-11 * rng.standard_normal((ndata, q, N))
    Psi = np.linalg.qr(rng.standard_normal((N, r_in)))[0]
    Phi = np.linalg.qr(rng.standard_normal((q, r_out)))[0]
    MPhi = Phi * np.linspace(1.0, 2.0, q)[:, None]                      # a diagonal "mass" on the outputs
    JPsi = hf.jacobian_times_input_basis(J, Psi)
    assert JPsi.shape == (ndata, q, r_in)
    assert rel(JPsi, np.einsum("iqn,nr->iqr", J, Psi)) < 1e-13
    JsP = hf.jacobian_transpose_times_output_basis(J, MPhi)
    assert JsP.shape == (ndata, N, r_out)
    assert rel(JsP, np.einsum("iqn,qr->inr", J, MPhi)) < 1e-13
    U, sig, V = hf.jacobian_svds(J, rM, seed=3)
    assert U.shape == (ndata, q, rM) and sig.shape == (ndata, rM) and V.shape == (ndata, N, rM)
    for i in range(ndata):
        s_ref = np.linalg.svd(J[i], compute_uv=False)[:rM]
        np.testing.assert_allclose(sig[i], s_ref, rtol=1e-7)
        assert np.linalg.norm(U[i].T @ U[i] - np.eye(rM)) < 1e-10 and np.linalg.norm(V[i].T @ V[i] - np.eye(rM)) < 1e-10
        assert np.linalg.norm(J[i] @ V[i] - U[i] * sig[i]) / np.linalg.norm(sig[i]) < 1e-6
    m_data, q_data = rng.standard_normal((ndata, N)), rng.standard_normal((ndata, q))
    d = str(tmp_path) + "/"
    hf.derivative_dataset(d, J, m_data, q_data, output_decoder=Phi, output_encoder=MPhi)
    hf.derivative_dataset(d, J, input_decoder=Psi, input_encoder=Psi)
    hf.derivative_dataset(d, J, svd_rank=rM, seed=3)
    mq = np.load(d + "mq_data.npz")
    assert sorted(mq.files) == ["m_data", "q_data"] and mq["m_data"].shape == (ndata, N)
    f = np.load(d + "JstarPhi_data.npz")
    assert sorted(f.files) == ["JstarPhi_data", "MPhi", "Phi"] and rel(f["JstarPhi_data"], JsP) == 0.0
    f = np.load(d + "JPsi_data.npz")
    assert sorted(f.files) == ["JPsi_data", "Psi", "input_encoder"] and rel(f["JPsi_data"], JPsi) == 0.0
    f = np.load(d + "Jsvd_data.npz")
    assert sorted(f.files) == ["U_data", "V_data", "sigma_data"]
    np.testing.assert_allclose(f["sigma_data"], sig, rtol=1e-12)         # same seed -> same Omega -> same factors


def test_jtj_jjt_and_serially_sampled_operator(ctx, golden_dir):
    """JTJ / JJT over a Jacobian-protocol object against the reference's own outputs (jacobian.py:142-193; goldens
    made by running hf.JTJ / hf.JJT / SummedListOperator of the reference), and the serially sampled accumulation
    (activeSubspaceProjector.py:98-257) against the sample mean it defines."""
    g = np.load(os.path.join(golden_dir, "operators.npz"))
    Js, x13, x9 = g["Js"], g["x13"], g["x9"]
    Jops = [hf.DenseJacobianOperator(Ji) for Ji in Js]
    x, y = hf.Vector(), hf.Vector()
    x.init(13)
    x.set_local(x13)
    jtj = hf.JTJ(Jops[0])
    jtj.init_vector(y, 0)
    jtj.mult(x, y)
    np.testing.assert_allclose(y.get_local(), g["jtj"], rtol=1e-12)
    xq, yq = hf.Vector(), hf.Vector()
    xq.init(9)
    xq.set_local(x9)
    jjt = hf.JJT(Jops[0])
    jjt.init_vector(yq, 0)
    jjt.mult(xq, yq)
    np.testing.assert_allclose(yq.get_local(), g["jjt"], rtol=1e-12)
    hf.SummedListOperator([hf.JTJ(J) for J in Jops], average=True).mult(x, y)
    np.testing.assert_allclose(y.get_local(), g["summed_avg"], rtol=1e-12)
    # block form == column form
    W = np.random.default_rng(0).standard_normal((13, 5))
    Y = hf.MultiVector(13, 5)
    hf.MatMvMult(jtj, hf.MultiVector.from_dense(W), Y)
    assert rel(Y.to_dense(), Js[0].T @ (Js[0] @ W)) < 1e-13

    class Observable:
        """Linear toy observable: the 'forward solve' just selects which stored Jacobian is the linearisation."""
        def __init__(self):
            self.i = -1
            self.solves = 0

        def generate_vector(self, kind):
            v = hf.Vector()
            v.init(13 if kind == 1 else 9)
            return v

        def init_vector(self, v, dim):
            v.init(9 if dim == 0 else 13)

        def solveFwd(self, u, lin):
            self.solves += 1
            self.i = (self.i + 1) % len(Jops)

        def setLinearizationPoint(self, lin):
            self.lin = lin

        def jacobian(self):
            return Jops[self.i]

    class Prior:
        def sample(self, noise, m):
            m.zero()
            m.axpy(1.0, noise)

    obs, noise = Observable(), hf.Vector()
    noise.init(13)
    for operation, Wd, ref in (("JTJ", W, np.mean([J.T @ (J @ W) for J in Js], axis=0)),
                               ("JJT", np.random.default_rng(1).standard_normal((9, 4)), None)):
        op = hf.SeriallySampledJacobianOperator(obs, noise, Prior(), operation=operation, nsamples=len(Js))
        if ref is None:
            ref = np.mean([J @ (J.T @ Wd) for J in Js], axis=0)
        Yd = hf.MultiVector(ref.shape[0], Wd.shape[1])
        op.matMvMult(hf.MultiVector.from_dense(Wd), Yd)            # accumulates into a zeroed block
        assert rel(Yd.to_dense(), ref) < 1e-13
        op.matMvMult(hf.MultiVector.from_dense(Wd), Yd)            # ... and again: twice the mean (:214-221)
        assert rel(Yd.to_dense(), 2 * ref) < 1e-13
        v = hf.Vector()
        op.init_vector(v)
        assert v.size() == ref.shape[0]
    assert obs.solves == 4 * len(Js)
    ms = [hf.Vector() for _ in Js]
    for m in ms:
        m.init(13)
    obs.i = -1
    op = hf.SeriallySampledJacobianOperator(obs, noise, Prior(), operation="JTJ", ms=ms, average=False)
    Yd = hf.MultiVector(13, 5)
    op.matMvMult(hf.MultiVector.from_dense(W), Yd)
    assert rel(Yd.to_dense(), np.sum([J.T @ (J @ W) for J in Js], axis=0)) < 1e-13
    with pytest.raises(AssertionError):
        op.matMvMult(hf.MultiVector.from_dense(W), hf.MultiVector(13, 4))

    # the reference re-draws a sample whose forward solve fails (activeSubspaceProjector.py:180-211): every third solve
    # of this observable raises, the operator draws again and still averages len(Js) successful samples
    class Flaky(Observable):
        def solveFwd(self, u, lin):
            self.solves += 1
            if self.solves % 3 == 0:
                raise RuntimeError("Newton did not converge")
            self.i = (self.i + 1) % len(Jops)

    flaky = Flaky()
    op = hf.SeriallySampledJacobianOperator(flaky, noise, Prior(), operation="JTJ", nsamples=len(Js))
    Yd = hf.MultiVector(13, 5)
    op.matMvMult(hf.MultiVector.from_dense(W), Yd)
    assert rel(Yd.to_dense(), np.mean([J.T @ (J @ W) for J in Js], axis=0)) < 1e-13
    assert op.solver_failures == (flaky.solves // 3) and flaky.solves == len(Js) + op.solver_failures

    class Broken(Observable):
        def solveFwd(self, u, lin):
            raise RuntimeError("mesh is inverted")

    op = hf.SeriallySampledJacobianOperator(Broken(), noise, Prior(), operation="JTJ", nsamples=2)
    op.max_solver_retries = 4
    with pytest.raises(RuntimeError, match="5 consecutive draws"):
        op.matMvMult(hf.MultiVector.from_dense(W), hf.MultiVector(13, 5))


def test_state_space_identity_operator_and_reference_names(ctx):
    """StateSpaceIdentityOperator (fullStateObservable.py:18-52) and the reference's spelling of the dense wrapper."""
    M, _ = _fem(300)
    Mop = hf.CsrOperator(M)
    x, y, p = hf.Vector(), hf.Vector(), hf.Vector()
    ident = hf.StateSpaceIdentityOperator(Mop)
    ident.init_vector(x, 0)
    ident.init_vector(y, 0)
    ident.init_vector(p, 1)
    v = np.random.default_rng(2).standard_normal(300)
    x.set_local(v)
    ident.mult(x, y)
    np.testing.assert_array_equal(y.get_local(), v)
    ident.transpmult(x, p)
    np.testing.assert_allclose(p.get_local(), M @ v, rtol=1e-13)
    hf.StateSpaceIdentityOperator(Mop, use_mass_matrix=False).transpmult(x, p)
    np.testing.assert_array_equal(p.get_local(), v)
    assert hf.npToDolfinOperator is hf.npToDeviceOperator


def test_active_subspace_error_tests_and_low_rank_jacobians(ctx, tmp_path):
    """ActiveSubspaceProjector.test_errors (activeSubspaceProjector.py:1037-1230) and construct_low_rank_Jacobians
    (:690-900): projection errors decrease with rank and match a numpy evaluation of the same projector; the Jacobian
    SVD dump has the reference's file names, keys and ranks."""
    rng = np.random.default_rng(11)
    ns, q, N = 12, 20, 900
    P, _ = np.linalg.qr(rng.standard_normal((N, q)))
    J = np.einsum("ioc,tc->iot", rng.standard_normal((ns, q, q)) * np.exp(-0.3 * np.arange(q))[None, None, :], P)
    M, K = _fem(N)
    A = (M + 1e-6 * K)
    Rm = (A @ sp.diags(1.0 / np.asarray(M.sum(axis=1)).ravel()) @ A).tocsr()

    class Prior:
        pass

    prior = Prior()
    prior.R = Rm
    prior.Rsolver = hp_o.SparseLUSolver(Rm)
    m_data, q_data = rng.standard_normal((ns, N)), rng.standard_normal((ns, q))

    class Obs:
        def jacobian_data(self, n):
            return J[:n]

        def mq_data(self, n):
            return m_data[:n], q_data[:n]

    params = hf.ActiveSubspaceParameterList()
    params["rank"], params["oversampling"], params["samples_per_process"] = 12, 6, ns
    params["serialized_sampling"], params["verbose"], params["save_and_plot"] = False, False, False
    params["jacobian_data_per_process"], params["jacobian_rank"] = ns, 6
    params["output_directory"] = str(tmp_path) + "/"
    asp = hf.ActiveSubspaceProjector(Obs(), prior, parameters=params)
    Xs = rng.standard_normal((9, N)) @ (0.05 * np.eye(N) + P @ P.T)          # mostly inside the Jacobians' row space
    Qs = rng.standard_normal((9, q))
    avg_in, std_in, avg_out, std_out = asp.test_errors(test_input=True, test_output=True, ranks=[2, 6, 12], samples=Xs,
                                                       output_samples=Qs)
    assert avg_in.shape == (3,) and avg_in[0] > avg_in[1] > avg_in[2] > 0 and np.all(std_in >= 0)
    assert avg_out[0] > avg_out[1] > avg_out[2] >= 0
    V = asp.V_GN.to_dense()
    for i, r in enumerate((2, 6, 12)):                                         # x - V_r V_r^T R x  (:1093-1111)
        E = Xs.T - V[:, :r] @ (V[:, :r].T @ (Rm @ Xs.T))
        ref = np.mean(np.linalg.norm(E, axis=0) / np.linalg.norm(Xs.T, axis=0))
        assert abs(avg_in[i] - ref) < 1e-10 * max(ref, 1.0)
    only_in = asp.test_errors(ranks=[6], samples=Xs)
    assert len(only_in) == 2
    # batched sampling (this projector): the STORED samples, rank = min(rank, q, N), whole arrays under jacobian_data/ (:906-1045)
    Ub, sb, Vb = asp.construct_low_rank_Jacobians()
    assert Ub.shape == (ns, q, 12) and sb.shape == (ns, 12) and Vb.shape == (ns, N, 12)
    jd = str(tmp_path) + "/jacobian_data/"
    for stem, arr in (("Us", Ub), ("sigmas", sb), ("Vs", Vb), ("ms", m_data), ("qs", q_data)):
        np.testing.assert_array_equal(np.load(jd + stem + "_on_proc_0.npy"), arr)
    np.testing.assert_allclose(sb[0][:3], np.linalg.svd(J[0], compute_uv=False)[:3], rtol=1e-6)
    again = asp.construct_low_rank_Jacobians()                                 # check_for_data: complete files are returned as they are
    np.testing.assert_array_equal(again[1], sb)
    assert not os.path.exists(str(tmp_path) + "/J_on_proc0.npz")
    # serialized sampling: fresh samples, rank = min(jacobian_rank, q, N), J_on_proc / mq_on_proc archives (:690-900)
    params["serialized_sampling"] = True
    U_data, sigma, V_data = asp.construct_low_rank_Jacobians()
    assert U_data.shape == (ns, q, 6) and sigma.shape == (ns, 6) and V_data.shape == (ns, N, 6)
    f = np.load(str(tmp_path) + "/J_on_proc0.npz")
    assert sorted(f.files) == ["U_data", "V_data", "sigma_data"]
    mq = np.load(str(tmp_path) + "/mq_on_proc0.npz")
    assert sorted(mq.files) == ["m_data", "q_data"] and mq["m_data"].shape == (ns, N)
    for i in range(ns):                                                        # rank-6 SVD of a rapidly decaying J
        s_ref = np.linalg.svd(J[i], compute_uv=False)[:6]
        np.testing.assert_allclose(sigma[i][:3], s_ref[:3], rtol=2e-2)
        assert np.linalg.norm(U_data[i].T @ U_data[i] - np.eye(6)) < 1e-10
