"""GPU suite: the one-workgroup LU solve (k_lu_solve, hfmi_lu.hip) and the one-sided Jacobi SVD (k_jacobi_svd,
hfmi_jacobi.hip) against exact references, at every boundary of their plans.

LU, through hfmi_test_lu_solve (X, the factored working copy, the status words, the T slot):
  1. a dyadic family on which the elimination is exact: X, L\\U and the pivots' extremes bit for bit, at both ends of every rung
     of the panel-width ladder;   2. pivots tied across the waves of the pivot search;   3. operands that need their row
     exchanges, against Higham's componentwise bounds (no fitted number);   4. exact scaling by 2^+-400;   5. every status;
  6. the T = (X + X^T) / 2 epilogue with its zero padding, on success and on every failure.
SVD:
  7. general, orthogonal, permuted-diagonal, clustered, identity and zero matrices at both sides of the LDS / global boundary
     and up to 256;   8. relative accuracy of every non-zero singular value of graded and rank-deficient matrices against a
     longdouble Jacobi (tests/helpers/jacobi_svd_ref.py), and what U holds for a zero singular value;   9. exact scaling by
     2^+-40 and 2^+-500;   10. non-finite input.
Eigensolver:
  11. the hard spectra of test_gpu_kernels.py through the Jacobi kernels.

Bit for bit means equal as IEEE numbers, -0.0 == +0.0 (the sign of a zero depends on whether a - b c is one fma or two
operations); where the sign matters -- the padding of T -- it is asserted separately."""
import os
import sys

import numpy as np
import pytest

import hippyflow_amd as hf
from hippyflow_amd import _lib as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import jacobi_svd_ref as jr  # noqa: E402
import lu_cases  # noqa: E402
from lu_small_twin import lu_panel_width, lu_solve_blocked  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64) + 0.0, np.asarray(b, dtype=np.float64) + 0.0      # -0.0 + 0.0 = +0.0
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


# ====================================================================== LU
def dev_lu(ctx, W, Z, want_T=False):
    W, Z = L.as_f64(W), L.as_f64(Z)
    m = W.shape[0]
    mp = min((m + 15) // 16 * 16, 256)
    X, LU, st, T = np.empty((m, m)), np.empty((m, m)), np.empty(3), np.full((mp, mp), np.nan)
    L.call("hfmi_test_lu_solve", ctx.handle, L.ptr(W), L.ptr(Z), m, int(want_T), L.ptr(X), L.ptr(LU), L.ptr(st), L.ptr(T) if want_T else None)
    return X, LU, {"pmin": st[0], "pmax": st[1], "failed": int(st[2])}, T


def _check_exact(ctx, m, ties):
    W, Z, X0, Lx, Ux, _ = lu_cases.exact_case(m, ties=ties)
    Xt, pmin, pmax, failed, LUt, piv = lu_solve_blocked(W, Z, full=True)
    assert failed == 0 and same_bits(Xt, X0)                      # the case is what it claims to be (CPU suite: at every blocking)
    X, LU, st, _ = dev_lu(ctx, W, Z)
    assert st["failed"] == 0
    assert same_bits(X, X0)
    assert same_bits(LU, LUt)
    d = np.abs(np.diag(Ux))
    assert st["pmin"] == d.min() == pmin and st["pmax"] == d.max() == pmax
    if m >= 3:
        assert st["pmin"] == 4.0 and st["pmax"] == 16.0


@pytest.mark.parametrize("m", lu_cases.SIZES)
def test_lu_exact_family_bit_for_bit(ctx, m):
    """W = P (L U) with dyadic factors: every pivot unique and a power of two, every intermediate exact.  X == X0,
    L\\U == the twin's, min / max |pivot| == 4 / 16."""
    _check_exact(ctx, m, ties=False)


@pytest.mark.parametrize("m", lu_cases.SIZES)
def test_lu_tied_pivots_take_the_first_row(ctx, m):
    """+-1 entries of L tie rows in seats of different waves (0 | 63 | 64 | 200; 104 | 170 | 240) for a pivot: only "first
    row of largest |entry|" reproduces the twin's L\\U and X0."""
    _check_exact(ctx, m, ties=True)


@pytest.mark.parametrize("m", lu_cases.SIZES)
@pytest.mark.parametrize("kind", ["tinydiag", "random", "graded"])
def test_lu_pivoting_within_higham_bounds(ctx, m, kind):
    """|L| <= 1, |P W - L U| <= gamma_m |L| |U| (Higham Thm 9.3), |W X - Z| <= gamma_3m P^T |L| |U| |X| (Thm 9.4),
    componentwise, with L, U, X from the device and P from the twin; the status words are min / max |diag U|."""
    W, Z = lu_cases.pivoting_case(m, kind)
    piv = lu_solve_blocked(W, Z, full=True)[5]
    X, LU, st, _ = dev_lu(ctx, W, Z)
    assert st["failed"] == 0
    r_fac, r_res, lmax = lu_cases.higham_ratios(W, Z, LU, piv, X)
    print("lu %-8s m=%3d nb=%3d: max |L| %.3f, factorisation at %.2e of its bound, residual at %.2e of its bound"
          % (kind, m, lu_panel_width(m), lmax, r_fac, r_res))
    assert lmax <= 1.0
    assert r_fac <= 1.0
    assert r_res <= 1.0
    d = np.abs(np.diag(LU))
    assert st["pmin"] == d.min() and st["pmax"] == d.max()


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_lu_scales_exactly(ctx, kind):
    m = 142
    W, Z = lu_cases.exact_case(m)[:2] if kind == "exact" else lu_cases.pivoting_case(m, "random")
    X, LU, st, _ = dev_lu(ctx, W, Z)
    Xs, LUs, sts, _ = dev_lu(ctx, np.ldexp(W, 400), np.ldexp(Z, -400))
    assert st["failed"] == 0 and sts["failed"] == 0
    assert same_bits(Xs, np.ldexp(X, -800))
    assert same_bits(np.triu(LUs), np.ldexp(np.triu(LU), 400)) and same_bits(np.tril(LUs, -1), np.tril(LU, -1))
    assert sts["pmin"] == np.ldexp(st["pmin"], 400) and sts["pmax"] == np.ldexp(st["pmax"], 400)


@pytest.mark.parametrize("m", [17, 142, 256])
def test_lu_status_duplicated_column(ctx, m):
    W, Z = lu_cases.exact_case(m)[:2]
    W[:, m - 2] = W[:, m // 3]
    _, LU, st, _ = dev_lu(ctx, W, Z)
    _, pmin, pmax, failed, LUt, _ = lu_solve_blocked(W, Z, full=True)       # still exact: the column cancels to zeros
    assert (pmin, failed) == (0.0, 2)
    assert st == {"pmin": 0.0, "pmax": pmax, "failed": 2}
    assert same_bits(LU, LUt)


@pytest.mark.parametrize("m", [2, 142])
def test_lu_status_singularity_threshold(ctx, m):
    """min |pivot| <= m eps max |pivot| is singular, the next number above is not"""
    d = np.ones(m)
    d[-1] = m * EPS
    assert dev_lu(ctx, np.diag(d), np.eye(m))[2] == {"pmin": m * EPS, "pmax": 1.0, "failed": 2}
    d[-1] = np.nextafter(m * EPS, 1.0)
    X, _, st, _ = dev_lu(ctx, np.diag(d), np.eye(m))
    assert st == {"pmin": d[-1], "pmax": 1.0, "failed": 0}
    assert same_bits(X, np.diag(1.0 / d))


def _failures(m):
    """(name, W, Z, failed) for every way the solve can fail"""
    W, Z = lu_cases.pivoting_case(m, "random")
    Wd = W.copy()
    Wd[:, m - 1] = Wd[:, 0]
    yield "singular", Wd, Z, 2
    for bad in (np.nan, np.inf, -np.inf):
        Wb = W.copy()
        Wb[m // 2, m - 1] = bad
        yield "non-finite W", Wb, Z, 1
        Zb = Z.copy()
        Zb[m - 1, m // 2] = bad
        yield "non-finite Z", W, Zb, 1
    Wo = np.eye(m)
    Wo[0, 0] = 1e-200
    yield "overflow", Wo, np.full((m, m), 1e200), 3


@pytest.mark.parametrize("m", [2, 17, 142])
def test_lu_status_nonfinite_and_overflow(ctx, m):
    for name, W, Z, failed in _failures(m):
        _, _, st, _ = dev_lu(ctx, W, Z)
        assert st["failed"] == failed, name
        if failed == 1:
            assert st["pmin"] == 0.0 and st["pmax"] == 0.0, name
    assert dev_lu(ctx, np.diag([1e-200, 1.0]), np.full((2, 2), 1e200))[2]["failed"] == 3        # test_small_solve_rejects_...'s case


@pytest.mark.parametrize("m", [17, 141, 142, 256])
def test_lu_T_epilogue(ctx, m):
    """T = (X + X^T) / 2 as the single pass has the kernel write it: the m x m part, +0.0 in the padding up to a multiple of
    16, nothing of the NaN fill left inside that square; all +0.0 on every failure."""
    mp = min((m + 15) // 16 * 16, 256)
    for W, Z in (lu_cases.exact_case(m)[:2], lu_cases.pivoting_case(m, "tinydiag")):
        X, _, st, T = dev_lu(ctx, W, Z, want_T=True)
        assert st["failed"] == 0 and T.shape == (mp, mp)
        assert not np.isnan(T).any()
        assert same_bits(T[:m, :m], 0.5 * (X + X.T))
        pad = np.ones((mp, mp), dtype=bool)
        pad[:m, :m] = False
        assert np.all(T[pad] == 0.0) and not np.signbit(T[pad]).any()
        assert same_bits(X, dev_lu(ctx, W, Z)[0])                  # the epilogue leaves X alone
    for name, W, Z, failed in _failures(m):
        _, _, st, T = dev_lu(ctx, W, Z, want_T=True)
        assert st["failed"] == failed, name
        assert np.all(T == 0.0) and not np.signbit(T).any(), name


# ====================================================================== SVD
SVD_SIZES = [1, 2, 3, 16, 17, 64, 65, 138, 139, 140, 141, 255, 256]      # 139 | 140: the matrix in LDS | in global memory


def check_svd(R, U, sv, V, ref=None):
    """the assertions of test_gpu_kernels.py::test_svd_small_matches_numpy, with the contract for zero singular values:
    their columns of U are exactly zero, the others orthonormal; V is orthogonal always"""
    k = R.shape[0]
    ref = np.linalg.svd(R, compute_uv=False) if ref is None else ref
    assert np.all(np.isfinite(sv)) and np.all(sv >= 0) and np.all(np.diff(sv) <= 0)
    np.testing.assert_allclose(sv, ref, rtol=1e-9, atol=1e-15 * ref[0])
    live = sv > 0
    assert np.all(U[:, ~live] == 0.0)
    assert np.linalg.norm(U[:, live].T @ U[:, live] - np.eye(int(live.sum()))) <= 1e-12 * k
    assert np.linalg.norm(V.T @ V - np.eye(k)) <= 1e-12 * k
    assert np.linalg.norm((U * sv) @ V.T - R) <= 1e-13 * k * np.linalg.norm(R)


def _general_families(k):
    rng = np.random.default_rng(1000 + k)
    G = rng.standard_normal((k, k))
    yield "gaussian", G, k
    Q = np.linalg.qr(G)[0]
    yield "orthogonal", Q, k
    d = rng.choice([0.25, 1.0, 1.0, 3.0], k) * rng.choice([-1.0, 1.0], k)
    yield "permuted diagonal", np.diag(d)[rng.permutation(k)], k
    Q2 = np.linalg.qr(rng.standard_normal((k, k)))[0]
    yield "clustered", (Q * (1.0 + 1e-10 * rng.integers(0, 3, k))) @ Q2.T, k
    yield "identity", np.eye(k), k
    yield "zero", np.zeros((k, k)), 0


@pytest.mark.parametrize("k", SVD_SIZES)
def test_svd_general_families(ctx, k):
    for name, R, rank in _general_families(k):
        U, sv, V = hf.svd_small(R, ctx)
        try:
            check_svd(R, U, sv, V)
            assert int((sv > 0).sum()) == rank
            if name == "permuted diagonal":                         # nothing to rotate: the values themselves
                assert same_bits(sv, np.sort(np.abs(R).sum(0))[::-1])
        except AssertionError as e:
            raise AssertionError("%s, k=%d: %s" % (name, k, e)) from e


_REF = {}


def _reference(family, k):
    if (family, k) not in _REF:
        R, rank = jr.accuracy_case(family, k)
        sig = jr.jacobi_svd(R, np.longdouble)[1]
        _REF[family, k] = (R, rank, sig, jr.accuracy_tolerance(R, rank, sig))
    return _REF[family, k]


@pytest.mark.parametrize("family,k", jr.accuracy_cases())
def test_svd_relative_accuracy(ctx, family, k):
    """Every non-zero singular value to 8 x the error of the fp64 restatement of the same algorithm (at least 8 k eps),
    relative to a longdouble Jacobi; and to 8 k eps sigma_1 absolutely, which is what holds the triangular family at
    k = 64, 65 (see jacobi_svd_ref.MEASURED).  A duplicated column leaves rounding noise, <= k eps sigma_1; exactly zero
    columns leave exact zeros and zero columns of U."""
    R, rank, ref, tol = _reference(family, k)
    U, sv, V = hf.svd_small(R, ctx)
    check_svd(R, U, sv, V, ref=ref.astype(np.float64))
    err = np.abs(sv[:rank].astype(np.longdouble) - ref[:rank])
    rel = float(np.max(err / ref[:rank]))
    print("svd %-12s k=%2d: worst relative error %.2e, allowed %.2e (ratio %.3f); absolute %.2e sigma_1"
          % (family, k, rel, tol, rel / tol, float(err.max() / ref[0])))
    assert rel <= tol
    assert float(err.max()) <= 8 * k * EPS * float(ref[0])
    if family == "duplicated":
        assert np.all(sv[rank:] <= k * EPS * sv[0])
    if family == "zero-columns":
        assert np.all(sv[rank:] == 0.0) and np.all(U[:, rank:] == 0.0)
        assert np.linalg.norm(U[:, :rank].T @ U[:, :rank] - np.eye(rank)) <= 1e-12 * k


_UNSCALED = {}


@pytest.mark.parametrize("e", [40, -40, 500, -500])
@pytest.mark.parametrize("k", [30, 140])
def test_svd_scales_exactly(ctx, k, e):
    """svd_small(2^e R) = (U, 2^e sigma, V) of svd_small(R), bit for bit: the orthogonality test and the rotations see
    ratios only.  At 2^+-500 the squared column norms' product leaves the exponent range unless the kernel scales."""
    R = np.random.default_rng(k).standard_normal((k, k))
    if k not in _UNSCALED:
        _UNSCALED[k] = hf.svd_small(R, ctx)
        check_svd(R, *_UNSCALED[k])
    U0, s0, V0 = _UNSCALED[k]
    U, sv, V = hf.svd_small(np.ldexp(R, e), ctx)
    assert same_bits(sv, np.ldexp(s0, e))
    assert same_bits(U, U0)
    assert same_bits(V, V0)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_svd_rejects_nonfinite(ctx, bad):
    R = np.random.default_rng(0).standard_normal((20, 20))
    R[7, 11] = bad
    with pytest.raises(hf.HfmiError, match="non-finite"):
        hf.svd_small(R, ctx)


# ====================================================================== Jacobi eigensolver
def _hard_spectra():
    from test_gpu_kernels import _hard_spectra as cases
    return list(cases())


@pytest.mark.parametrize("name,T", _hard_spectra(), ids=[n for n, _ in _hard_spectra()])
def test_sym_eig_small_jacobi_hard_spectra(ctx, name, T):
    """test_gpu_kernels.py::test_sym_eig_small_divide_and_conquer_hard_spectra's cases and assertions through
    method="jacobi" (no power-of-two scaling in front of it: "huge" and "tiny" are 1e+-150)."""
    k = T.shape[0]
    d, V = hf.sym_eig_small(T, method="jacobi")
    w = np.linalg.eigvalsh(T)[::-1]
    nrm = max(np.abs(w).max(), 1e-300)
    assert np.all(np.diff(d) <= 0)
    assert np.max(np.abs(d - w)) < 1e-14 * k * nrm
    assert np.linalg.norm(V.T @ V - np.eye(k)) < 1e-13 * k
    assert np.linalg.norm(T @ V - V * d) < 1e-13 * k * nrm
