"""CPU checks of the smoothed-aggregation hierarchy (hippyflow_amd/amg.py) and of the numpy twin of the device V-cycle
(tests/helpers/amg_vcycle_twin.py): coarsening rate, Galerkin coarse operators, operator complexity, the twin as a CG
preconditioner on structured grids and on an unstructured mesh with a coefficient jump, its symmetry, input validation."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import amg_vcycle_twin as twin                     # noqa: E402
from hippyflow_amd import workloads                # noqa: E402
from hippyflow_amd.amg import AMGHierarchy         # noqa: E402


def grid_operator(nx):
    return (workloads.grid_mass_matrix(nx, nx) + 0.1 * workloads.grid_stiffness_matrix(nx, nx)).tocsr()


def p1_mesh_operator(m=60, jump=1e3, seed=0):
    """A = M + 0.1 K_kappa on a Delaunay triangulation of seeded random points in the unit square: an m x m grid, every
    interior point moved at random by up to 0.35 of the spacing (no slivers), kappa = jump on the triangles with centroid
    x > 0.5, 1 elsewhere."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, m)
    pts = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    inner = np.all((pts > 0) & (pts < 1), axis=1)
    pts[inner] += rng.uniform(-0.35, 0.35, (int(inner.sum()), 2)) / (m - 1)
    tri = Delaunay(pts).simplices
    X = pts[tri]                                                   # (nt, 3, 2)
    d1, d2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    det = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    area = 0.5 * np.abs(det)
    keep = area > 1e-14
    tri, X, area, det = tri[keep], X[keep], area[keep], det[keep]
    # gradients of the barycentric functions
    G = np.empty((len(tri), 3, 2))
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        e = X[:, c] - X[:, b]
        G[:, a, 0], G[:, a, 1] = -e[:, 1] / det, e[:, 0] / det
    kappa = np.where(X.mean(axis=1)[:, 0] > 0.5, jump, 1.0)
    rows, cols, kv, mv = [], [], [], []
    for a in range(3):
        for b in range(3):
            rows.append(tri[:, a])
            cols.append(tri[:, b])
            kv.append(kappa * area * np.einsum("ti,ti->t", G[:, a], G[:, b]))
            mv.append(area * (1.0 / 6.0 if a == b else 1.0 / 12.0))
    n = len(pts)
    r, c = np.concatenate(rows), np.concatenate(cols)
    K = sp.csr_matrix((np.concatenate(kv), (r, c)), shape=(n, n))
    M = sp.csr_matrix((np.concatenate(mv), (r, c)), shape=(n, n))
    A = (M + 0.1 * K).tocsr()
    return ((A + A.T) * 0.5).tocsr()


def is_spd(A):
    """LDL^T pivots of a symmetric permutation all positive (sparse LU without row pivoting, symmetric mode)."""
    A = sp.csc_matrix(A)
    if A.shape[0] <= 2000:
        return bool(np.linalg.eigvalsh(A.toarray()).min() > 0)
    lu = spla.splu(A, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options={"SymmetricMode": True})
    return bool(np.array_equal(lu.perm_r, lu.perm_c) and np.all(lu.U.diagonal() > 0))


def pcg_iterations(A, h, seed=0):
    b = np.random.default_rng(seed).standard_normal(A.shape[0])
    its = [0]

    def count(_):
        its[0] += 1

    x, info = spla.cg(A, b, rtol=1e-12, atol=0.0, M=twin.as_linear_operator(h), callback=count, maxiter=200)
    return its[0], info, np.linalg.norm(b - A @ x) / np.linalg.norm(b)


@pytest.fixture(scope="module", params=[64, 128, 256])
def grid(request):
    A = grid_operator(request.param)
    return request.param, A, AMGHierarchy(A)


def test_hierarchy_coarsening_galerkin_and_complexity(grid):
    nx, A, h = grid
    sizes = h.sizes()
    assert sizes[0] == nx * nx and len(sizes) >= 2 and sizes[-1] <= 500
    for a, b in zip(sizes, sizes[1:]):
        assert 3 * b <= a, sizes
    for lv, nxt in zip(h.levels, h.levels[1:]):
        G = (lv.P.T @ lv.A @ lv.P).tocsr()
        assert spla.norm(nxt.A - G) <= 1e-14 * spla.norm(G)
        assert abs(lv.R - lv.P.T).max() == 0.0
        assert is_spd(nxt.A)
    assert 1.0 < h.operator_complexity() <= 2.0
    info = h.info()
    assert info["rows"] == sizes and info["nnz"] == h.nnz() and info["levels"] == len(sizes)
    # the coarse inverse is the inverse of the coarsest matrix
    Ac = h.levels[-1].A.toarray()
    assert np.abs(h.coarse_inv @ Ac - np.eye(len(Ac))).max() < 1e-9


def test_twin_vcycle_preconditions_cg_on_grids(grid):
    nx, A, h = grid
    its, info, res = pcg_iterations(A, h)
    assert info == 0 and its <= 20 and res <= 1e-12 * 1.01, (nx, its, res)


def test_twin_vcycle_on_unstructured_mesh_with_coefficient_jump():
    A = p1_mesh_operator()
    h = AMGHierarchy(A)
    assert len(h.sizes()) >= 2
    its, info, res = pcg_iterations(A, h)
    assert info == 0 and its <= 20, (its, res, h.sizes())
    # Jacobi-CG needs far more: the multigrid is doing the work
    jits = [0]
    spla.cg(A, np.random.default_rng(0).standard_normal(A.shape[0]), rtol=1e-12, atol=0.0, M=sp.diags(1.0 / A.diagonal()),
            callback=lambda _: jits.__setitem__(0, jits[0] + 1), maxiter=5000)
    assert jits[0] > 3 * its


def test_twin_vcycle_is_symmetric(grid):
    nx, A, h = grid
    rng = np.random.default_rng(1)
    n = A.shape[0]
    Vn = max(np.linalg.norm(twin.vcycle(h, v)) / np.linalg.norm(v) for v in rng.standard_normal((3, n)))
    for _ in range(3):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        asym = abs(x @ twin.vcycle(h, y) - y @ twin.vcycle(h, x))
        assert asym <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y) * Vn
    # positive definite on random vectors (a CG preconditioner must be)
    X = rng.standard_normal((n, 4))
    assert np.all(np.einsum("ij,ij->j", X, twin.vcycle(h, X)) > 0)


def test_block_twin_equals_columnwise():
    A = grid_operator(40)
    h = AMGHierarchy(A, max_coarse=100)
    B = np.random.default_rng(2).standard_normal((A.shape[0], 3))
    V = twin.vcycle(h, B)
    for j in range(3):
        np.testing.assert_allclose(V[:, j], twin.vcycle(h, B[:, j]), rtol=1e-13, atol=1e-13 * np.abs(V).max())


def test_small_matrix_is_one_dense_level():
    A = grid_operator(12)
    h = AMGHierarchy(A)
    assert h.sizes() == [144]
    b = np.random.default_rng(0).standard_normal(144)
    np.testing.assert_allclose(A @ twin.vcycle(h, b), b, rtol=0, atol=1e-10 * np.linalg.norm(b))


@pytest.mark.parametrize("case", ["non_square", "non_symmetric", "non_positive_diagonal", "nan_entry"])
def test_invalid_matrices_raise_value_error(case):
    A = grid_operator(20).tolil()
    if case == "non_square":
        A = sp.csr_matrix(np.ones((5, 4)))
    elif case == "non_symmetric":
        A[0, 1] = A[0, 1] + 1e-3
    elif case == "non_positive_diagonal":
        A[3, 3] = 0.0
    elif case == "nan_entry":
        A[2, 2] = np.nan
    with pytest.raises(ValueError):
        AMGHierarchy(sp.csr_matrix(A))
