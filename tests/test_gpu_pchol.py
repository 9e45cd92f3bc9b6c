"""GPU suite of the pivoted Cholesky factor of kernel covariances (hfmi_pchol_* / pivoted_cholesky, hfmi_pchol.hip): the order-free
properties of tests/helpers/pchol_checks.py on every case, pivot identity with the numpy twin where the twin's pivots are well separated, the
rel_tol stop, determinism, several row tiles per workgroup (a size beyond the default grid, and small sizes on a capped grid), the block
storage contract of the library-owned factor and its read-only Python face, the KLE route of KLEProjector (kernel_factor_rank), sampling,
and the argument checks."""
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
import fake_pde                                   # noqa: E402
import pchol_checks as pc                         # noqa: E402
import pchol_twin as twin                         # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib as L               # noqa: E402
from hippyflow_amd import projectors              # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
STOP = {name: value for value, name in enumerate(L.PCHOL_STOP_REASONS)}


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


def operator_of(case, ctx):
    N, d, family, ell, nugget, _ = case
    return hf.KernelCovarianceOperator(pc.case_points(case), family=family, sigma=pc.SIGMA, ell=ell, nugget=nugget, ctx=ctx)


_factors = {}


def device_factor(case, ctx, rel_tol=0.0):
    """one factorisation per (case, rel_tol) for the whole module: (PivotedCholesky, L on the host)"""
    key = (case, rel_tol)
    if key not in _factors:
        f = hf.pivoted_cholesky(operator_of(case, ctx), case[5], rel_tol)       # the operator is dropped: the factor outlives it
        _factors[key] = (f, f.L.to_dense())
    return _factors[key]


_twins = {}


def twin_factor(case, rel_tol=0.0):
    key = (case, rel_tol)
    if key not in _twins:
        N, d, family, ell, nugget, max_rank = case
        _twins[key] = twin.factor_kernel(pc.case_points(case), family, pc.SIGMA, ell, nugget, max_rank, rel_tol)
    return _twins[key]


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_properties(ctx, case):
    f, Lh = device_factor(case, ctx)
    assert f.L.size() == case[0] and f.L.nvec() == f.rank and f.residual_trace == f.trace[-1]
    assert f.pivots.dtype == np.int64 and f.stop_reason in STOP
    pc.check_properties(case, Lh, f.pivots, f.trace, f.rank, STOP[f.stop_reason], "device")


def test_default_grid_takes_a_second_tile(ctx):
    """the premise of SECOND_TILE_CASE in test_properties: more row tiles than workgroups this device can hold (8 waves per SIMD is the
    hardware's limit, a workgroup is one wave on each of a unit's four SIMDs)"""
    tiles = -(-pc.SECOND_TILE_CASE[0] // pc.ROWS_PER_TILE)
    assert tiles > 8 * ctx.device_info()["compute_units"]


# (case, most workgroups): 6 row tiles on 2 workgroups with the pivot's row restaged three times per tile; 4 tiles on 3 (one workgroup
# takes two); 79 tiles on 5
@pytest.mark.parametrize("case,cap", [(c, cap) for c in pc.CASES for cap in [{1500: 2, 1000: 3, 20000: 5}.get(c[0])] if cap],
                         ids=lambda v: pc.case_id(v) if isinstance(v, tuple) else "grid%d" % v)
def test_many_tiles_per_workgroup(ctx, case, cap):
    """a capped grid walks several row tiles per workgroup: the same L and pivots bit for bit (a row's chain and the arg-max do not depend
    on the grouping), traces within the worst case of regrouping a sum of N non-negative terms (2 N eps relative)"""
    f0, L0 = device_factor(case, ctx)
    L.call("hfmi_tuning_set", b"pchol_grid", cap)
    try:
        f = hf.pivoted_cholesky(operator_of(case, ctx), case[5])
        Lh = f.L.to_dense()
    finally:
        L.call("hfmi_tuning_set", b"pchol_grid", 0)
    pc.check_properties(case, Lh, f.pivots, f.trace, f.rank, STOP[f.stop_reason], "device, %d workgroups" % cap)
    assert f.rank == f0.rank and f.stop_reason == f0.stop_reason and np.array_equal(f.pivots, f0.pivots)
    assert np.array_equal(Lh, L0)
    terr = np.abs(f.trace - f0.trace)
    print("capped grid %s: max trace difference / (2 N eps trace) = %.3g" % (pc.case_id(case), float(np.max(terr / (2 * case[0] * EPS * f0.trace)))))
    assert np.all(terr <= 2 * case[0] * EPS * f0.trace)


@pytest.mark.parametrize("case", pc.PIVOTS_COMPARABLE, ids=pc.case_id)
def test_pivots_are_the_twins(ctx, case):
    t = twin_factor(case)
    gap = float(t.gaps[1:].min())
    print("pivots %s: twin's smallest gap after the first step %.3g" % (pc.case_id(case), gap))
    assert gap >= pc.MIN_GAP
    f, _ = device_factor(case, ctx)
    assert f.rank == t.rank and STOP[f.stop_reason] == t.stop_reason
    assert np.array_equal(f.pivots, t.pivots)


def test_rel_tol_stop(ctx):
    case, rel_tol = pc.REL_TOL_CASE, pc.REL_TOL_VALUE
    full, t = twin_factor(case), twin_factor(case, rel_tol)
    thr = rel_tol * full.trace[0]
    first = int(np.argmax(full.trace <= thr))
    assert t.stop_reason == twin.REL_TOL and t.rank == first and full.gaps[1:].min() >= pc.MIN_GAP
    assert np.abs(full.trace[first - 1:first + 1] - thr).min() > 1e-9 * thr        # the twin is not at the threshold
    f, _ = device_factor(case, ctx, rel_tol)
    print("rel_tol stop: device rank %d, twin rank %d, trace[rank-1], trace[rank] = %.6g, %.6g, threshold %.6g" % (
        f.rank, t.rank, f.trace[-2], f.trace[-1], rel_tol * f.trace[0]))
    assert f.stop_reason == "rel_tol" and f.rank == t.rank
    assert f.trace[-1] <= rel_tol * f.trace[0] < f.trace[-2]                       # the first j at or below the threshold


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[0] in (1000, 1500, 20000)], ids=pc.case_id)
def test_two_factorisations_are_bit_identical(ctx, case):
    f1, L1 = device_factor(case, ctx)
    f2 = hf.pivoted_cholesky(operator_of(case, ctx), case[5])
    assert f2.rank == f1.rank and f2.stop_reason == f1.stop_reason
    assert np.array_equal(f2.pivots, f1.pivots) and np.array_equal(f2.trace, f1.trace)
    assert np.array_equal(f2.L.to_dense(), L1)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[0] in (15, 63, 64, 65, 193, 257)], ids=pc.case_id)
def test_factor_block_contract(ctx, case):
    """the library-owned factor: allocated like hfmi_block_create (ld = round_up(N, 32), 128-byte aligned), rows N..ld-1 of every column
    +0.0 bit for bit, columns the factorisation did not reach untouched zeros"""
    f, Lh = device_factor(case, ctx)
    N, kmax = case[0], min(case[5], case[0])
    ld = f.L.leading_dimension()
    assert ld == ba.round_up(N, 32) and f.L.device_ptr() % 128 == 0
    # alias of the whole allocation as an ld x kmax block: N == ld, so the wrap zeroes nothing and a download sees the padding rows
    h = C.c_void_p()
    L.call("hfmi_block_wrap", ctx.handle, C.c_void_p(f.L.device_ptr()), ld, kmax, ld, C.byref(h))
    alias = hf.MultiVector(ctx=ctx, _handle=h, _parent=f)
    raw = np.ascontiguousarray(alias.to_vectors()).view(np.uint64).reshape(kmax, ld)
    ba.assert_contract(raw, raw, N, [(0, f.rank)], [(0, f.rank)], what="hfmi_pchol_create")
    assert not raw[f.rank:].any()
    assert np.array_equal(raw[:f.rank, :N].view(np.float64).T, Lh)


class _Prior:
    pass


@pytest.fixture(scope="module")
def kle_problem():
    N, r = 1500, 20
    rng = np.random.default_rng(21)
    pts = pc.scattered(N, 2, seed=21)
    family, sigma, ell = "matern52", 1.0, 1.0
    Cm = hf.kernel_cov_host(pts, family, sigma, ell)
    mdiag = (0.5 + rng.random(N)) / N
    return dict(N=N, r=r, pts=pts, family=family, sigma=sigma, ell=ell, Cm=Cm, mdiag=mdiag, M=sp.diags(mdiag).tocsr())


def kle_projector(p, ctx, M=None, factor_rank=60):
    prior = _Prior()
    prior.M = p["M"] if M is None else M
    prior.C = hf.KernelCovarianceOperator(p["pts"], family=p["family"], sigma=p["sigma"], ell=p["ell"], ctx=ctx)
    params = hf.KLEParameterList()
    params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = p["r"], 10, False, False
    kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)
    kle.kernel_factor_rank = factor_rank
    return kle


@pytest.mark.parametrize("mode", ["mass", "identity"])
def test_kle_route(ctx, kle_problem, mode):
    p = kle_problem
    N, r, Cm = p["N"], p["r"], p["Cm"]
    kle = kle_projector(p, ctx)
    d, dec, enc = kle.construct_input_subspace(mode)
    d, V, E = np.asarray(d), dec.to_dense(), enc.to_dense()
    assert d.shape == (r,) and V.shape == (N, r) and kle.kle_factor.rank == 60
    if mode == "mass":
        Mm = p["M"]
        A = p["mdiag"][:, None] * Cm * p["mdiag"][None, :]
        d_exact = sla.eigh(A, np.diag(p["mdiag"]), eigvals_only=True)[::-1][:r]
    else:
        Mm = sp.identity(N, format="csr")
        A = Cm
        d_exact = np.linalg.eigvalsh(Cm)[::-1][:r]
    orth = np.abs(V.T @ (Mm @ V) - np.eye(r)).max()
    enc_err = np.linalg.norm(E - Mm @ V) / np.linalg.norm(Mm @ V)
    res = np.linalg.norm(A @ V - (Mm @ V) * d) / np.linalg.norm(A @ V)
    gap = d_exact - d
    print("kle route [%s]: |V^T M V - I| %.3g, encoder %.3g, residual %.3g, d_exact - d in [%.3g, %.3g], bound %.3g" % (
        mode, orth, enc_err, res, gap.min(), gap.max(), kle.kle_eigenvalue_error_bound))
    assert orth < 1e-10
    assert enc_err < 1e-10
    assert res < 1e-4
    assert np.all(gap >= -1e-12) and np.all(gap <= kle.kle_eigenvalue_error_bound)
    assert kle.M_orthogonal == (mode == "mass")


def test_kle_route_refusals(ctx, kle_problem):
    kle = kle_projector(kle_problem, ctx)
    with pytest.raises(ValueError):
        kle.construct_input_subspace("prior")
    host_M = fake_pde.MatrixOperator(kle_problem["M"])             # mult / init_vector only: a host operator on the device side
    kle = kle_projector(kle_problem, ctx, M=host_M)
    assert not isinstance(kle.M, hf.CsrOperator)
    with pytest.raises(ValueError):
        kle.construct_input_subspace("mass")


def test_kle_default_is_unchanged(ctx, kle_problem):
    """kernel_factor_rank left None: the projector makes the calls it made before the attribute existed -- the probe draw, then the fused
    generalized double pass -- and returns their result bit for bit"""
    p = kle_problem
    kle = kle_projector(p, ctx, factor_rank=None)
    assert hf.KLEProjector.kernel_factor_rank is None
    kle.construct_input_subspace("mass")          # the mass matrix' lazy spectrum estimate is made here, before both compared runs
    hf.parRandom.reseed(7)
    d, dec, enc = kle.construct_input_subspace("mass")
    assert not hasattr(kle, "kle_eigenvalue_error_bound") and not hasattr(kle, "kle_factor")
    hf.parRandom.reseed(7)
    A = hf.MassPreconditionedCovarianceOperator(kle.C, kle.M)
    Omega = projectors._draw_omega(p["N"], p["r"] + 10, kle.collective, ctx)
    d2, V2 = hf.doublePassG(A, kle.M, kle._Msolver(), Omega, p["r"], s=1)
    E2 = hf.MultiVector(V2)
    hf.MatMvMult(kle.M, V2, E2)
    assert np.array_equal(np.asarray(d), np.asarray(d2))
    assert np.array_equal(dec.to_dense(), V2.to_dense()) and np.array_equal(enc.to_dense(), E2.to_dense())


def test_sampling(ctx):
    case = (1000, 2, "matern32", 0.3, 0.0, 138)
    f, Lh = device_factor(case, ctx)
    X, xi = f.sample(7, seed=123)
    Xh, xih = X.to_dense(), xi.to_dense()
    assert Xh.shape == (1000, 7) and xih.shape == (f.rank, 7)
    assert abs(xih.mean()) < 0.2 and 0.8 < xih.std() < 1.2                      # a standard normal block, not zeros
    err, bound = np.abs(Xh - Lh @ xih), 8 * f.rank * EPS * (np.abs(Lh) @ np.abs(xih))
    print("sampling: max err/bound = %.3g" % float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound) and np.abs(Xh).max() > 0 and bound.min() > 0
    X2, xi2 = f.sample(7, seed=123)
    assert np.array_equal(xi2.to_dense(), xih) and np.array_equal(X2.to_dense(), Xh)
    _, xi3 = f.sample(7, seed=124)
    assert not np.array_equal(xi3.to_dense(), xih)


def test_factor_is_read_only(ctx):
    f, Lh = device_factor((64, 2, "matern32", 0.3, 0.3, 64), ctx)
    other = hf.MultiVector(64, f.rank, ctx=ctx)
    for write in (f.L.zero, lambda: f.L.scale(2.0), lambda: f.L.axpy(1.0, other), lambda: f.L.copy_from(other), lambda: f.L.swap(other),
                  lambda: other.swap(f.L), f.L.orthogonalize, f.L.view(1, 2).zero, f.L[0].zero):
        with pytest.raises(ValueError):
            write()
    assert np.array_equal(f.L.to_dense(), Lh)
    copy = hf.MultiVector(f.L)                                                  # the way to a writable block
    copy.scale(2.0)
    assert np.array_equal(copy.to_dense(), 2.0 * Lh) and np.array_equal(f.L.to_dense(), Lh)


def test_invalid_arguments(ctx):
    lib = L.load()
    op = hf.KernelCovarianceOperator(pc.scattered(10, 2, seed=1), ctx=ctx)
    other = hf.CsrOperator(sp.identity(10, format="csr"), ctx=ctx)

    def create(op_handle, max_rank, rel_tol, want_out=True):
        out = C.c_void_p()
        rc = lib.hfmi_pchol_create(op_handle, max_rank, rel_tol, C.byref(out) if want_out else None)
        return rc, out

    bad = {"not a kernel covariance": (other._op, 4, 0.0), "max_rank = 0": (op._op, 0, 0.0), "max_rank < 0": (op._op, -3, 0.0),
           "max_rank = 16385": (op._op, 16385, 0.0), "rel_tol < 0": (op._op, 4, -1e-3), "rel_tol = nan": (op._op, 4, float("nan")),
           "rel_tol = inf": (op._op, 4, float("inf")), "no operator": (None, 4, 0.0)}
    for what, args in bad.items():
        rc, out = create(*args)
        assert rc == -1 and not out.value, what                                  # HFMI_ERR_INVALID, nothing created
        assert lib.hfmi_last_error().decode(), what
    assert create(op._op, 4, 0.0, want_out=False)[0] == -1
    with pytest.raises(ValueError):
        hf.pivoted_cholesky(other, 4)
    with pytest.raises(hf.HfmiError) as e:
        hf.pivoted_cholesky(op, 0)
    assert e.value.code == -1 and "max_rank" in str(e.value)
    # the largest max_rank is accepted (kmax = min(max_rank, N)); the handle reads back and is destroyed through the ABI
    rc, out = create(op._op, 16384, 0.0)
    assert rc == 0 and out.value
    rank, reason, trace0 = C.c_int(), C.c_int(), C.c_double()
    assert lib.hfmi_pchol_info(out, C.byref(rank), C.byref(reason), C.byref(trace0)) == 0
    assert 1 <= rank.value <= 10 and trace0.value == 10.0
    assert lib.hfmi_pchol_info(None, C.byref(rank), None, None) == -1 and lib.hfmi_pchol_factor(out, None) == -1
    assert lib.hfmi_pchol_destroy(out) == 0 and lib.hfmi_pchol_destroy(None) == 0
