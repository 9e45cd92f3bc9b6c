"""CPU suite of the matrix-free kernel covariance (hfmi_op_kernel_cov, hippyflow_amd/csrc/hfmi_kcov.hip): the dense host evaluation
``operators.kernel_cov_host`` the device operator is compared with, the numpy twin of the kernel's slab / panel / summation order
(tests/helpers/kernel_cov_twin.py), and the C-ABI bookkeeping of the new entry point."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kernel_cov_twin as twin                       # noqa: E402

from hippyflow_amd import _lib, operators, workloads   # noqa: E402

FAMILIES = ("matern12", "matern32", "matern52", "sqexp")
EPS = np.finfo(np.float64).eps


def scattered(N, d, seed=0):
    """seeded points in the unit cube, two of them coincident"""
    pts = np.random.default_rng(seed).random((N, d))
    if N > 3:
        pts[N - 1] = pts[1]
    return pts


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_host_evaluation(family, d):
    N, sigma, ell, nugget = 90, 1.7, 0.3, 0.25
    pts = scattered(N, d, seed=d)
    C = operators.kernel_cov_host(pts, family, sigma, ell, nugget)
    assert C.shape == (N, N) and np.array_equal(C, C.T)
    np.testing.assert_allclose(np.diag(C), sigma ** 2 + nugget, rtol=1e-15)
    C0 = operators.kernel_cov_host(pts, family, sigma, ell)
    np.testing.assert_allclose(np.diag(C0), sigma ** 2, rtol=1e-15)
    assert C0[1, N - 1] == sigma ** 2                              # coincident points, no nugget off the diagonal
    assert C[1, N - 1] == C0[1, N - 1]
    for M in (C, C0):
        assert np.linalg.eigvalsh(M).min() >= -1e-12 * sigma ** 2 * N
    rows = [5, 0, N - 1, 17]
    assert np.array_equal(operators.kernel_cov_host(pts, family, sigma, ell, nugget, rows=rows), C[rows])
    # the formula itself, one entry by hand
    r = np.linalg.norm(pts[3] - pts[40]) / ell
    want = {"matern12": np.exp(-r), "matern32": (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r),
            "matern52": (1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r), "sqexp": np.exp(-r * r / 2)}[family]
    np.testing.assert_allclose(C[3, 40], sigma ** 2 * want, rtol=1e-13)


def test_host_evaluation_rejects_what_the_device_rejects():
    with pytest.raises(ValueError):
        operators.kernel_cov_host(np.zeros((4, 2)), "matern72", 1.0, 0.1)
    with pytest.raises(ValueError):
        operators.kernel_cov_host(np.zeros((4, 2, 2)), "matern32", 1.0, 0.1)


def test_same_numbers_as_the_grid_formula():
    nx, ny, N = 10, 8, 60
    pts = workloads.grid_points(N, nx, ny)
    C = operators.kernel_cov_host(pts, "matern32", 2.0, 0.3)
    np.testing.assert_allclose(C, workloads.matern32_host(N, nx, ny, sigma=2.0, ell=0.3), rtol=1e-14)
    g = np.load(os.path.join(ROOT, "tests", "golden", "independent_eig.npz"))
    nx, ny, N = int(g["matern_nx"]), int(g["matern_ny"]), int(g["matern_N"])
    head = operators.kernel_cov_host(workloads.grid_points(N, nx, ny), "matern32", float(g["matern_sigma"]), float(g["matern_ell"]),
                                     rows=np.arange(5))
    np.testing.assert_allclose(head[:, :5], g["matern_C_corner"], rtol=1e-14)


# N: below one slab, one row tile + a ragged slab, several row tiles and chunks with a ragged tail; k: one tile, ragged, two panels
@pytest.mark.parametrize("N,k,d,family,nugget,accumulate", [
    (3, 1, 1, "matern12", 0.0, False),
    (21, 5, 2, "matern32", 0.3, True),
    (70, 17, 3, "matern52", 0.0, False),
    (131, 3, 2, "sqexp", 0.3, False),
    (37, 150, 2, "matern32", 0.0, True),
])
def test_twin_against_host(N, k, d, family, nugget, accumulate):
    rng = np.random.default_rng(N + k)
    pts, W, Y0 = scattered(N, d, seed=N), rng.standard_normal((N, k)), rng.standard_normal((N, k))
    sigma, ell = 1.3, 0.2
    C = operators.kernel_cov_host(pts, family, sigma, ell, nugget)
    got = twin.apply(pts, W, family, sigma, ell, nugget, Y=Y0, accumulate=accumulate)
    ref = C @ W + (Y0 if accumulate else 0.0)
    bound = 8 * N * EPS * (np.abs(C) @ np.abs(W) + (np.abs(Y0) if accumulate else 0.0))
    assert np.all(np.abs(got - ref) <= bound), np.max(np.abs(got - ref) / bound)
    # the twin's entries are the host's: both round the exponent g a few times (relative error <= 4 eps each), and exp turns an
    # error dg of its argument into a relative error dg, so the two agree to 8 eps (1 + g) with g at the cube's diagonal
    ca, _, _, g1, g2 = twin.COEFFS[family]
    a = ca * np.sqrt(d) / ell
    np.testing.assert_allclose(twin.entries(pts, np.arange(N), np.arange(N), family, sigma, ell, nugget), C,
                               rtol=8 * EPS * (1 + a * (g1 + g2 * a)))


def test_twin_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "hippyflow_amd", "csrc", "hfmi_kcov.hip")).read()
    assert int(re.search(r"#define KC_JC (\d+)", src).group(1)) == twin.JC
    assert 16 * int(re.search(r"#define KC_MAXT (\d+)", src).group(1)) == twin.PANEL and twin.PANEL >= 138
    for name, (ca, p1, p2, g1, g2) in twin.COEFFS.items():
        assert _lib.KERNEL_FAMILIES[name] in range(4)
    assert "%.16g" % twin.COEFFS["matern32"][0] in src and "%.15g" % twin.COEFFS["matern52"][0] in src


def test_abi_bookkeeping():
    header = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    proto = re.search(r"HFMI_API int hfmi_op_kernel_cov\(([^;]*)\);", header)
    assert proto and "hfmi_block" not in proto.group(1)            # no block parameter: no row in the contract tables
    for name, value in _lib.KERNEL_FAMILIES.items():
        assert re.search(r"#define HFMI_KERNEL_%s %d\b" % (name.upper(), value), header)
    sig = _lib.SIGNATURES["hfmi_op_kernel_cov"]
    assert len(sig) == 9 and sig[2] is ctypes.c_int64 and sig[5:8] == [ctypes.c_double] * 3
    # the export list is a pattern over the prefix every declared entry point carries
    assert "hfmi_*" in open(os.path.join(ROOT, "hippyflow_amd", "libhfmi.map")).read()
    lib_path = os.path.join(ROOT, "hippyflow_amd", "libhfmi.so")
    if not os.path.exists(lib_path):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(lib_path), "hfmi_op_kernel_cov")
    assert "hfmi_kcov.hip" in __import__("hippyflow_amd._build", fromlist=["SOURCES"]).SOURCES


def test_public_names():
    import hippyflow_amd as hf
    assert issubclass(hf.KernelCovarianceOperator, hf.DeviceOperator) and hf.kernel_cov_host is operators.kernel_cov_host
    assert callable(workloads.kle_kernel_workload)
