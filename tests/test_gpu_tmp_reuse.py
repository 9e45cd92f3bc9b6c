"""GPU tests of the context's cached temporaries (``enum hfmi_tmp_slot``, hfmi_internal.h): a slot's block is kept between
calls and may be wider than the next request, is regrown for a wider one and replaced for another length, and the slots of
nested owners (fused solve > QR > composition > composition > sparse solve) are all live at once.  None of that may show in a
result.  N = 1000 is not a multiple of 32, so the leading dimension of every block differs from its length."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hippyflow_amd as hf                     # noqa: E402  (a broken import of the package is a failure, not a skip)
from hippyflow_amd import _lib as L            # noqa: E402
from hippyflow_amd import workloads            # noqa: E402

GRIDS = {1000: (40, 25), 520: (26, 20)}


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def _snapshots(n, N, decay, seed):
    rng = np.random.default_rng(seed)
    U0, _ = np.linalg.qr(rng.standard_normal((n, n)))
    W0, _ = np.linalg.qr(rng.standard_normal((N, n)))
    return ((U0 * np.exp(-decay * np.arange(n))) @ W0.T) * np.sqrt(n)      # (n, N): one snapshot per row


def _omega(N, k, ctx):
    return hf.MultiVector.from_dense(np.random.default_rng(1000 * k + N).standard_normal((N, k)), ctx=ctx)


class _Problem:
    """A (snapshot Gram, rank 64), B = M (P1 mass matrix) and B^-1 = the sparse solver, all on one context"""

    def __init__(self, N, ctx):
        M = workloads.grid_mass_matrix(*GRIDS[N]).tocsr()
        self.A = hf.SnapshotGramOperator(hf.MultiVector.from_vectors(_snapshots(64, N, 0.05, N), ctx=ctx), ctx=ctx)
        self.B = hf.CsrOperator(M, ctx=ctx)
        self.Binv = hf.CsrPCGSolver(M, ctx=ctx)


def _sketch_eig(p, Omega, r):
    N, k, ctx = Omega.size(), Omega.nvec(), Omega.ctx
    Ybar, Y = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    p.A.matMvMult(Omega, Ybar)
    p.Binv.matMvMult(Ybar, Y)
    d, U = np.empty(r), hf.MultiVector(N, r, ctx=ctx)
    L.call("hfmi_sketch_eig", Omega.handle, Y.handle, Ybar.handle, p.B._op, int(r), 0, L.ptr(d), U.handle)
    return d, U


SOLVERS = {
    "double_pass": lambda p, Om, r: hf.doublePass(p.A, Om, r),
    "double_pass_g": lambda p, Om, r: hf.doublePassG(p.A, p.B, p.Binv, Om, r),
    "single_pass_g": lambda p, Om, r: hf.singlePassG(p.A, p.B, p.Binv, Om, r),
    "sketch_eig": _sketch_eig,
}


def _solve(name, p, N, k, ctx):
    d, U = SOLVERS[name](p, _omega(N, k, ctx), k // 2)
    return np.array(d), U.to_dense()


# ------------------------------------------------------------------ 1. width reuse
@pytest.mark.parametrize("name", sorted(SOLVERS))
def test_a_cached_temporary_of_another_width_or_length_does_not_show(ctx, name):
    """On ONE context: 24 probe vectors, then 8 (narrower than the cached blocks), then 40 (wider: the blocks are regrown), then
    the same at N = 520 (another length: the blocks are replaced).  Every result equals, bit for bit, the same call on a context
    that has never held a temporary."""
    used = hf.Context(ctx.device)
    for N in (1000, 520):
        p_used = _Problem(N, used)
        for k in (24, 8, 40):
            d, U = _solve(name, p_used, N, k, used)
            fresh = hf.Context(ctx.device)
            d_ref, U_ref = _solve(name, _Problem(N, fresh), N, k, fresh)
            np.testing.assert_array_equal(d, d_ref, err_msg="%s N=%d k=%d" % (name, N, k))
            np.testing.assert_array_equal(U, U_ref, err_msg="%s N=%d k=%d" % (name, N, k))


# ------------------------------------------------------------------ 2. nesting
def test_nested_compositions_keep_their_temporaries_apart(ctx):
    """B^-1 of doublePassG is M (A^-1 M A^-1) M: a composition whose middle operator is a composition of two sparse solves (the
    BiLaplacianRsolver shape inside the KLE shape), so the solve's, the QR's, both compositions' and the Krylov solver's
    temporaries are live in one call.  The reference route applies the five stages one at a time through matMvMult to the
    identity and hands the product to the solve as a dense operator.

    The two routes are NOT the same arithmetic: the dense route multiplies Y by the stored matrix (one contraction per entry),
    the composed route runs the iterative solves on Y itself.  Both carry the solver's relative residual (rel_tol 1e-14 on a
    Jacobi-scaled spectrum of condition 2: D^-1 A with A = M + 1e-4 K), which reaches the eigenpairs amplified by cond(Q) ~ 10 of
    the 8-vector sketch and, for U, by the inverse relative gap ~ 5 of the 4 leading eigenvalues (decay 0.1 per index): about
    5e-14 expected, so the bound is 1e-12 relative (normwise, columns of U aligned in sign), not bit equality.  Aliased
    temporaries would show as O(1) differences."""
    N, k, r = 1000, 8, 4
    nx, ny = GRIDS[N]
    M = workloads.grid_mass_matrix(nx, ny).tocsr()
    Amat = (M + 1e-4 * workloads.grid_stiffness_matrix(nx, ny)).tocsr()
    A = hf.SnapshotGramOperator(hf.MultiVector.from_vectors(_snapshots(32, N, 0.1, 7)))
    Mop = hf.CsrOperator(M)
    S = hf.CsrPCGSolver(Amat, rel_tol=1e-14)
    inner = hf.ComposedOperator(S, Mop, S)
    outer = hf.ComposedOperator(Mop, inner, Mop)
    Omega = _omega(N, k, ctx)
    d, U = hf.doublePassG(A, Mop, outer, Omega, r)

    D = np.empty((N, N))
    for c0 in range(0, N, 200):                               # the identity in slabs of 200 columns
        X = hf.MultiVector.from_dense(np.eye(N)[:, c0:c0 + 200])
        for stage in (Mop, S, Mop, S, Mop):
            Y = hf.MultiVector(N, 200)
            stage.matMvMult(X, Y)
            X = Y
        D[:, c0:c0 + 200] = X.to_dense()
    d_ref, U_ref = hf.doublePassG(A, Mop, hf.npToDeviceOperator(D), Omega, r)

    U, U_ref = U.to_dense(), U_ref.to_dense()
    U_ref = U_ref * np.sign(np.sum(U * U_ref, axis=0))
    err_d = np.linalg.norm(d - d_ref) / np.linalg.norm(d_ref)
    err_U = np.linalg.norm(U - U_ref) / np.linalg.norm(U_ref)
    print("nested composition vs dense product: d %.3e, U %.3e" % (err_d, err_U))
    assert err_d <= 1e-12 and err_U <= 1e-12, (err_d, err_U)


# ------------------------------------------------------------------ 3. accumulate
def _accumulating_operator(kind):
    nx, ny = GRIDS[1000]
    M = workloads.grid_mass_matrix(nx, ny).tocsr()
    if kind == "csr_pcg":
        return hf.CsrPCGSolver(M)
    if kind == "csr_amg":
        return hf.CsrAMGSolver((M + 0.1 * workloads.grid_stiffness_matrix(nx, ny)).tocsr())
    if kind == "host_callback":
        return hf.HostCallbackOperator(lambda W: 2.0 * W + W[::-1], N=1000)
    Mop = hf.CsrOperator(M)
    return hf.ComposedOperator(Mop, hf.CsrPCGSolver(M), Mop)


@pytest.mark.parametrize("kind", ["csr_pcg", "csr_amg", "host_callback", "composed"])
def test_accumulate_equals_apply_then_axpy(ctx, kind):
    """matMvMult(X, Y, accumulate=True) of an operator that cannot add to its output goes through a temporary: Y <- Y + T.
    Bit-equal to T = op(X) into a block of its own followed by Y0.axpy(1, T)."""
    N, k = 1000, 5
    op = _accumulating_operator(kind)
    rng = np.random.default_rng(5)
    X = hf.MultiVector.from_dense(rng.standard_normal((N, k)))
    Y0 = rng.standard_normal((N, k))
    T = hf.MultiVector(N, k)
    op.matMvMult(X, T)
    want = hf.MultiVector.from_dense(Y0)
    want.axpy(1.0, T)
    got = hf.MultiVector.from_dense(Y0)
    op.matMvMult(X, got, accumulate=True)
    assert np.abs(T.to_dense()).max() > 0
    np.testing.assert_array_equal(got.to_dense(), want.to_dense())
