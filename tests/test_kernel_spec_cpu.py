"""Host side of the Matern-1 family and of the metric of the kernel covariances (no GPU): the numpy twin of the device's a K_1(a) against
40-digit values, the host matrices with a metric, the BiLaplacian's kernel against the Fourier integral of its precision, the signed-offset
column of the grid operator, the host Cholesky factor of a metric, and the ABI's bookkeeping."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_metric_twin as gt                     # noqa: E402
import matern1_twin as m1                         # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib                    # noqa: E402

EPS = np.finfo(np.float64).eps
FAMILIES = ["matern12", "matern32", "matern52", "sqexp", "matern1"]
HFMI_ERR_INVALID = -1


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "matern1_phi.npz"))
    return z["a"], z["phi"]


# ---------------------------------------------------------------------------------------------------------------- 1. a K_1(a)
def test_twin_against_forty_digits(golden):
    """E_phi = max relative error of the twin over 0 < a <= 700 against the correctly rounded a K_1(a): at most 16 eps.
    Measured: 2.62 eps (series side 2.62 at a = 1.6125, Chebyshev side 1.78)."""
    a, ref = golden
    assert a.size == 1604 and a[0] == 0.0 and a[-2] == 750.0 and a[-1] == 1e4
    got = m1.phi(a)
    m = (a > 0.0) & (a <= 700.0)
    rel = np.abs(got[m] - ref[m]) / ref[m]
    worst = int(np.argmax(rel))
    print("matern1 twin: E_phi = %.3f eps at a = %.6g (series side %.3f eps, Chebyshev side %.3f eps)"
          % (rel.max() / EPS, a[m][worst], rel[a[m] <= 2.0].max() / EPS, rel[a[m] > 2.0].max() / EPS))
    assert rel.max() <= 16.0 * EPS
    assert got[0] == 1.0 and ref[0] == 1.0
    for v in got[-2:]:
        assert np.isfinite(v) and 0.0 <= v <= 1e-300


def test_twin_tables_are_the_headers():
    """the literals of the header and of the twin are the same strings, in the same order"""
    src = open(os.path.join(ROOT, "hippyflow_amd", "csrc", "hfmi_kcov_k1.h")).read()
    src = re.sub(r"//[^\n]*", "", src)
    for name, table in (("S1", m1.K1_S1), ("S2", m1.K1_S2), ("CH", m1.K1_CHEB)):
        body = re.search(r"constexpr double %s\[\w+\] = \{([^}]*)\}" % name, src).group(1)
        values = [float(v) for v in body.replace("\n", " ").split(",") if v.strip()]
        assert values == list(table), name
    assert int(re.search(r"#define K1_NSER (\d+)", src).group(1)) == len(m1.K1_S1)
    assert int(re.search(r"#define K1_NCHEB (\d+)", src).group(1)) == len(m1.K1_CHEB)


def test_host_matern1_is_the_twin(golden):
    """kernel_cov_host('matern1') goes through scipy.special.k1e (4 eps of its own): within 16 + 8 eps of the 40-digit values"""
    a, ref = golden
    m = a <= 600.0
    x = a[m] / np.sqrt(2.0)
    row = hf.kernel_cov_host(np.concatenate([[0.0], x]), "matern1", 1.0, 1.0)[0, 1:]
    rel = np.abs(row - ref[m]) / ref[m]
    # the host's a = sqrt(2) (a / sqrt(2)) is two roundings away from the fixture's, and d(ln phi) / d(ln a) = -a K_0 / K_1 is at most a in
    # magnitude: the abscissa moves phi by up to 2 a eps; 16 eps for the evaluation's condition and 8 for k1e's own 4
    tol = (24.0 + 2.0 * a[m]) * EPS
    assert np.all(rel <= tol), float((rel / tol).max())
    assert row[0] == 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. host matrices
def scattered(N, d, seed):
    pts = np.random.default_rng(seed).random((N, d))
    pts[N - 1] = pts[1]
    return pts


def spd(d, seed):
    A = np.random.default_rng(seed).standard_normal((d, d))
    return A @ A.T + 0.5 * np.eye(d)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_metric_is_the_isotropic_kernel_on_transformed_points(family, d):
    N, sigma, ell, nugget = 37, 1.3, 0.4, 0.25
    pts = scattered(N, d, seed=10 + d)
    G = spd(d, seed=d)
    Lf = np.linalg.cholesky(G)
    full = hf.kernel_cov_host(pts, family, sigma, ell, nugget, metric=G)
    iso = hf.kernel_cov_host(pts @ Lf, family, sigma, ell, nugget)
    assert np.allclose(full, iso, rtol=64 * EPS, atol=0.0)
    # and it is the quadratic form: r^2 = delta^T G delta
    delta = pts[:, None, :] - pts[None, :, :]
    r = np.sqrt(np.einsum("ijc,ce,ije->ij", delta, G, delta))
    direct = sigma ** 2 * gt.phi(family, r / ell)
    direct[np.arange(N), np.arange(N)] += nugget
    assert np.allclose(full, direct, rtol=1e-9, atol=1e-13)
    # the cross form still slices the square form bit for bit
    for r0, r1 in ((0, N), (7, 30), (N - 1, N)):
        K = hf.kernel_cross_cov_host(pts[r0:r1], pts, family, sigma, ell, nugget, diag_offset=r0, metric=G)
        assert np.array_equal(K, full[r0:r1])
        assert np.array_equal(K, hf.kernel_cov_host(pts, family, sigma, ell, nugget, rows=range(r0, r1), metric=G))
    if d == 1:      # a scalar is a 1 x 1 metric
        assert np.array_equal(hf.kernel_cov_host(pts, family, sigma, ell, nugget, metric=float(G[0, 0])), full)


@pytest.mark.parametrize("d", [1, 2, 3])
def test_matern1_slices_and_identity_metric(d):
    N, sigma, ell, nugget = 29, 0.9, 0.3, 0.1
    pts = scattered(N, d, seed=d)
    full = hf.kernel_cov_host(pts, "matern1", sigma, ell, nugget)
    assert np.all(np.isfinite(full)) and np.array_equal(full, full.T)
    assert full[1, N - 1] == sigma ** 2 and full[1, 1] == sigma ** 2 + nugget       # coincident points: phi(0) = 1, no nugget
    K = hf.kernel_cross_cov_host(pts[3:11], pts, "matern1", sigma, ell, nugget, diag_offset=3)
    assert np.array_equal(K, full[3:11])
    assert np.array_equal(hf.kernel_cov_host(pts, "matern1", sigma, ell, nugget, metric=np.eye(d)), full)


@pytest.mark.parametrize("bad", ["nonsymmetric", "indefinite", "nan", "shape"])
def test_metric_rejections_in_python(bad):
    G = {"nonsymmetric": [[2.0, 0.5], [0.5 + 1e-12, 1.0]], "indefinite": [[1.0, 2.0], [2.0, 1.0]], "nan": [[1.0, 0.0], [0.0, np.nan]],
         "shape": np.eye(3)}[bad]
    pts = scattered(9, 2, seed=0)
    with pytest.raises(ValueError):
        hf.kernel_cov_host(pts, "matern32", 1.0, 0.2, metric=G)
    with pytest.raises(ValueError):
        hf.kernel_cross_cov_host(pts[:3], pts, "matern1", 1.0, 0.2, metric=G)
    with pytest.raises(ValueError):
        hf.kernel_cov_host(pts, "matern72", 1.0, 0.2)


# ---------------------------------------------------------------------------------------------------------------- 3. the BiLaplacian's kernel
def test_anisotropy_2d():
    T = hf.anisotropy_2d(2.0, 0.5, np.pi / 4)
    assert np.allclose(T, [[1.25, 0.75], [0.75, 1.25]], rtol=4 * EPS)
    assert np.allclose(np.linalg.eigvalsh(T), [0.5, 2.0], rtol=8 * EPS)
    T = hf.anisotropy_2d(3.0, 0.25, 0.3)
    s, c = np.sin(0.3), np.cos(0.3)
    assert T[0, 0] == 3.0 * s * s + 0.25 * c * c and T[0, 1] == T[1, 0] == (3.0 - 0.25) * s * c and T[1, 1] == 3.0 * c * c + 0.25 * s * s
    assert np.array_equal(hf.anisotropy_2d(1.0, 1.0, 0.7).round(15), np.eye(2))
    with pytest.raises(ValueError):
        hf.anisotropy_2d(0.0, 1.0, 0.1)


def test_bilaplacian_kernel_against_the_fourier_integral():
    """c(x) = (1 / |box|) sum_k exp(i k x) / (delta + gamma k^T Theta k)^2 on a periodic box of side 40 with n = 4096 cells per side, at
    six offsets, against kernel_cov_host(**bilaplacian_kernel_2d(gamma, delta)): rtol 1e-6.  Periodic images sit 40 kappa = 126 away
    (e^-126) and the truncation of the sum at |k| = pi n / 40 decays with the distance from 0."""
    gamma, delta, side, n = 0.1, 1.0, 40.0, 4096
    kw = hf.bilaplacian_kernel_2d(gamma, delta)
    assert kw["family"] == "matern1" and set(kw) == {"family", "sigma", "ell", "metric"}
    Theta = hf.anisotropy_2d(2.0, 0.5, np.pi / 4)
    assert np.allclose(kw["metric"] @ Theta, np.eye(2), atol=8 * EPS)
    assert kw["ell"] == np.sqrt(2.0 * gamma / delta)
    assert np.isclose(kw["sigma"] ** 2, 1.0 / (4.0 * np.pi * delta * gamma * np.sqrt(np.linalg.det(Theta))), rtol=8 * EPS)
    k = 2.0 * np.pi * np.fft.fftfreq(n, d=side / n)
    k0, k1 = k[:, None], k[None, :]
    q = Theta[0, 0] * k0 * k0 + 2.0 * Theta[0, 1] * k0 * k1 + Theta[1, 1] * k1 * k1
    c = np.fft.ifft2(1.0 / (delta + gamma * q) ** 2).real * (n / side) ** 2
    h = side / n
    offsets = [(30, 0), (0, 30), (30, 30), (30, -30), (100, 40), (-60, 80)]
    pts = np.array([(0.0, 0.0)] + [(i * h, j * h) for i, j in offsets])
    row = hf.kernel_cov_host(pts, **kw)[0]
    worst = 0.0
    for t, (i, j) in enumerate(offsets):
        ref = c[i % n, j % n]
        worst = max(worst, abs(row[1 + t] - ref) / abs(ref))
    print("bilaplacian_kernel_2d against the Fourier integral (n = %d): worst relative error %.3g" % (n, worst))
    assert worst <= 1e-6
    assert abs(row[3] - row[4]) > 0.1 * max(row[3], row[4])      # (30, 30) against (30, -30): a transposed or unrotated Theta fails here
    # splats into the device classes' argument lists
    import inspect
    for cls in (hf.KernelCovarianceOperator, hf.KernelCrossCovarianceOperator, hf.KernelCovarianceRowsOperator, hf.GridKernelCovarianceOperator):
        params = inspect.signature(cls.__init__).parameters
        assert set(kw) <= set(params) and list(params)[-1] == "metric"


# ---------------------------------------------------------------------------------------------------------------- 4. the grid's signed column
GRID_FAMILIES = ["matern1", "matern32"]


@pytest.mark.parametrize("cid,shape,spacing,G,subset", gt.GRID_CASES, ids=[c[0] for c in gt.GRID_CASES])
@pytest.mark.parametrize("family", GRID_FAMILIES)
def test_grid_twin(cid, shape, spacing, G, subset, family):
    sigma, ell, nugget, k = 1.3, 0.45, 0.2, 5
    lam = gt.spectrum(shape, spacing, family, sigma, ell, nugget, G)
    P = lam.size
    assert np.abs(lam.imag).max() <= 64.0 * EPS * np.log2(P) * np.abs(lam.real).max()
    nodes = gt.case_nodes(shape, subset)
    pts = gt.points(shape, spacing, nodes)
    W = np.random.default_rng(P).standard_normal((pts.shape[0], k))
    Cm = hf.kernel_cov_host(pts, family, sigma, ell, nugget, metric=G)
    bound = gt.column_bounds(shape, spacing, family, sigma, ell, nugget, W, np.abs(Cm) @ np.abs(W), G)
    Y = gt.apply(shape, spacing, family, sigma, ell, nugget, W, nodes, G)
    ratio = np.linalg.norm(Y - Cm @ W, axis=0) / bound
    print("grid metric twin %s %s: worst err/bound = %.3g" % (cid, family, ratio.max()))
    assert ratio.max() <= 1.0
    # the even column of fftcov_twin is NOT this matrix: the metric's off-diagonal entries are what the signs carry
    wrong = gt.base.apply(shape, spacing, "matern32", sigma, ell, nugget, W, nodes)
    assert np.linalg.norm(wrong - Cm @ W) > 1e-3 * np.linalg.norm(Cm @ W)


def test_grid_twin_without_a_metric_is_the_even_column():
    """identity metric, one of the four first families: the signed rule gives the column fftcov_twin states, to rounding"""
    for shape, spacing in (((6, 5), (0.2, 0.25)), ((4, 3, 3), (0.2, 0.25, 0.3)), ((1, 7), (0.1, 0.3)), ((5,), (0.3,))):
        a = gt.first_column(shape, spacing, "matern52", 1.1, 0.4, 0.3, None)
        b = gt.base.first_column(shape, spacing, "matern52", 1.1, 0.4, 0.3)
        assert np.allclose(a, b, rtol=16 * EPS, atol=0.0)
    one = gt.first_column((5,), (0.3,), "matern1", 1.0, 0.4, 0.0, np.array([[2.5]]))      # a scalar metric in one dimension
    assert one.shape == (16,) and one[0] == 1.0 and np.allclose(one[1:8], one[:8:-1], rtol=4 * EPS)


# ---------------------------------------------------------------------------------------------------------------- 5. the metric's factor
def factor(G, d):
    G = np.ascontiguousarray(G, dtype=np.float64)
    out = np.full((d, d), np.nan)
    status = _lib.load().hfmi_kernel_metric_factor(_lib.ptr(G), d, _lib.ptr(out))
    return status, out


@pytest.mark.parametrize("d", [1, 2, 3])
def test_metric_factor_against_numpy(d):
    for seed in range(4):
        G = spd(d, seed)
        status, Lf = factor(G, d)
        assert status == 0
        assert np.array_equal(np.triu(Lf, 1), np.zeros((d, d)))
        assert np.allclose(Lf, np.linalg.cholesky(G), rtol=16 * EPS, atol=16 * EPS * np.abs(G).max())
    status, Lf = factor(np.diag([4.0, 0.25, 9.0][:d]), d)
    assert status == 0 and np.array_equal(Lf, np.diag([2.0, 0.5, 3.0][:d]))


def test_metric_factor_rejections():
    assert factor(np.eye(2), 0)[0] == HFMI_ERR_INVALID and factor(np.eye(4), 4)[0] == HFMI_ERR_INVALID
    assert factor([[2.0, 0.5], [0.5 + 1e-12, 1.0]], 2)[0] == HFMI_ERR_INVALID            # not symmetric
    assert factor([[2.0, 0.5], [0.5 * (1.0 + EPS), 1.0]], 2)[0] == 0                       # within 4 eps max |G|
    assert factor([[1.0, 2.0], [2.0, 1.0]], 2)[0] == HFMI_ERR_INVALID                      # indefinite: the second pivot is -3
    assert factor([[0.0]], 1)[0] == HFMI_ERR_INVALID and factor([[-1.0]], 1)[0] == HFMI_ERR_INVALID
    assert factor([[1.0, 1.0], [1.0, 1.0]], 2)[0] == HFMI_ERR_INVALID                      # singular: pivot 0
    for bad in (np.nan, np.inf):
        assert factor([[1.0, 0.0], [0.0, bad]], 2)[0] == HFMI_ERR_INVALID
        assert factor([[1.0, bad], [bad, 1.0]], 2)[0] == HFMI_ERR_INVALID
    assert "metric" in _lib.load().hfmi_last_error().decode()
    lib = _lib.load()
    assert lib.hfmi_kernel_metric_factor(None, 2, None) == HFMI_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- 6. ABI bookkeeping
def test_abi_bookkeeping():
    header = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    assert re.search(r"#define HFMI_KERNEL_MATERN1 4\b", header) and _lib.KERNEL_FAMILIES["matern1"] == 4
    assert int(re.search(r"HFMI_ERR_INVALID = (-?\d+),", header).group(1)) == HFMI_ERR_INVALID
    struct = re.search(r"typedef struct hfmi_kernel_spec \{(.*?)\} hfmi_kernel_spec;", header, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert [s.strip() for s in struct.split(";") if s.strip()] == ["int family", "int d", "double sigma, ell, nugget", "double metric[9]"]
    assert [(n, t) for n, t in _lib.KernelSpec._fields_] == [("family", ctypes.c_int), ("d", ctypes.c_int), ("sigma", ctypes.c_double),
                                                             ("ell", ctypes.c_double), ("nugget", ctypes.c_double), ("metric", ctypes.c_double * 9)]
    assert ctypes.sizeof(_lib.KernelSpec) == 8 + 3 * 8 + 9 * 8
    # each descriptor creator: the old argument list with (family, sigma, ell, nugget) replaced by one pointer
    for old in ("hfmi_op_kernel_cov", "hfmi_op_kernel_cross_cov", "hfmi_op_kernel_cov_rows", "hfmi_op_kernel_cov_grid"):
        new = old + "_spec"
        proto_old = re.search(r"HFMI_API int %s\(([^;]*)\);" % old, header).group(1)
        proto_new = re.search(r"HFMI_API int %s\(([^;]*)\);" % new, header).group(1)
        squeeze = lambda s: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", s, flags=re.S)).strip()
        expect = squeeze(proto_old).replace("int family, double sigma, double ell, double nugget", "const hfmi_kernel_spec* spec")
        assert squeeze(proto_new) == expect, new
        so, sn = _lib.SIGNATURES[old], _lib.SIGNATURES[new]
        i = so.index(ctypes.c_double) - 1               # the family's position
        assert so[i:i + 4] == [ctypes.c_int] + [ctypes.c_double] * 3
        assert sn == so[:i] + [ctypes.POINTER(_lib.KernelSpec)] + so[i + 4:], new
        assert hasattr(_lib.load(), new)
    assert len(_lib.SIGNATURES["hfmi_kernel_metric_factor"]) == 3
    # the creators with a bare family stop at HFMI_KERNEL_SQEXP (the GPU suite asks them with family = 4)
    src = open(os.path.join(ROOT, "hippyflow_amd", "csrc", "hfmi_op.hip")).read()
    for old in ("hfmi_op_kernel_cov", "hfmi_op_kernel_cross_cov", "hfmi_op_kernel_cov_rows", "hfmi_op_kernel_cov_grid"):
        body = re.search(r'extern "C" int %s\(.*?\n\}' % old, src, flags=re.S).group(0)
        assert "HFMI_KERNEL_SQEXP, nullptr, out" in body and "MATERN1" not in body, old
    # without a context they answer INVALID before anything else
    spec = _lib.KernelSpec(4, 2, 1.0, 0.1, 0.0)
    pts = np.zeros((3, 2))
    out = ctypes.c_void_p()
    assert _lib.load().hfmi_op_kernel_cov_spec(None, _lib.ptr(pts), 3, 2, ctypes.byref(spec), ctypes.byref(out)) == HFMI_ERR_INVALID
    assert _lib.load().hfmi_op_kernel_cov(None, _lib.ptr(pts), 3, 2, 4, 1.0, 0.1, 0.0, ctypes.byref(out)) == HFMI_ERR_INVALID
