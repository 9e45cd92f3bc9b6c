"""Host side of the Matern family of any smoothness, family "matern" with nu (no GPU): the numpy twin of the device's phi_nu with the
LIBRARY's tables against 40-digit values, the library's tables against mpmath's, the host matrices (scipy's K_nu) against the same
values and against the named families, whittle_matern_kernel against closed forms and the radial Fourier integral of its precision,
and the ABI's bookkeeping."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import matern_nu_twin as tw                       # noqa: E402

hf = pytest.importorskip("hippyflow_amd")
from hippyflow_amd import _lib                    # noqa: E402

EPS = np.finfo(np.float64).eps
HFMI_ERR_INVALID = -1
E_ASSERT = 64.0          # eps: twice the measured worst of the twin (23.75), rounded up to a power of two; the cap is 128
NUS = (0.125, 0.3, 0.5, 0.75, 1.0, 1.0 + 2.0 ** -30, 1.25, 1.4999, 1.5, 2.0, 2.000001, 2.5, 3.2, 4.5, 6.0, 7.49, 8.0)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "matern_nu_phi.npz"))
    return z["nu"], z["a"], z["phi"], z["tables"]


def library_tables(nu):
    T = np.full(tw.WORDS, np.nan)
    status = _lib.load().hfmi_kernel_matern_tables(float(nu), _lib.ptr(T))
    return status, T


# ---------------------------------------------------------------------------------------------------------------- 1. the twin
def test_fixture_contents(golden):
    nus, a, phi, tables = golden
    assert tuple(nus) == NUS
    assert a[0] == 0.0 and a[-2] == 750.0 and a[-1] == 1e4 and 380 <= a.size <= 420
    near = [2.0]
    lo = hi = 2.0
    for _ in range(3):
        lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 3.0)
        near += [lo, hi]
    assert set(near) <= set(a) and a[1] == 1e-9 and 700.0 in a
    assert phi.shape == (len(NUS), a.size) and tables.shape == (len(NUS), tw.WORDS)
    assert np.all(phi[:, 0] == 1.0) and np.all(np.isfinite(phi)) and np.all(phi >= 0.0)


def test_twin_with_the_library_tables_against_forty_digits(golden):
    """E = max relative error of the twin, run with the tables of hfmi_kernel_matern_tables, over 0 < a <= 700 and the 17 values of nu,
    against the correctly rounded phi_nu(a): at most E_ASSERT = 64 eps (the cap of the scheme is 128).
    Measured: 23.75 eps (nu = 1.4999 at a = 1.98333, on the series side just below the split; series side 5.9 to 23.8 eps over the
    values of nu, Chebyshev side 1.8 to 3.9 eps)."""
    nus, a, ref, _ = golden
    assert E_ASSERT <= 128.0
    m = (a > 0.0) & (a <= 700.0)
    worst = 0.0
    for i, nu in enumerate(nus):
        status, T = library_tables(nu)
        assert status == 0
        got = tw.phi(T, a)
        rel = np.abs(got[m] - ref[i][m]) / ref[i][m] / EPS
        lo = a[m] <= 2.0
        print("matern nu = %.10g twin: E = %.2f eps at a = %.6g (series side %.2f, Chebyshev side %.2f)"
              % (nu, rel.max(), a[m][int(np.argmax(rel))], rel[lo].max(), rel[~lo].max()))
        worst = max(worst, rel.max())
        assert got[0] == 1.0
        for v in got[-2:]:
            assert np.isfinite(v) and 0.0 <= v <= 1e-300
    print("matern nu twin: E = %.2f eps" % worst)
    assert worst <= E_ASSERT


def test_twin_far_out_is_zero_not_nan():
    """a beyond every exponent the recurrence could survive: the clamp at 1e5 keeps a^(2 n) finite and e^(-a) is +0"""
    for nu in (0.125, 1.0, 8.0):
        _, T = library_tables(nu)
        got = tw.phi(T, np.array([1e5, 1e30, 1e300, np.finfo(np.float64).max]))
        assert np.array_equal(got, np.zeros(4)) and not np.any(np.signbit(got))


# ---------------------------------------------------------------------------------------------------------------- 2. the tables
def test_library_tables_are_mpmaths(golden):
    """Each word of hfmi_kernel_matern_tables (long double) against the same word from mpmath at 50 digits (the fixture).  The tolerance
    of a word is what it may move phi by, and the words together stay under 1 eps:
      * header words (mu, the Gamma constants, the two normalisers, sqrt(2 nu)) multiply phi or one of its three terms: eps / 4 relative,
        and n, mu, nu exactly (mu = nu - n is exact in fp64);
      * a coefficient of one of the six series polynomials enters p(y) = sum c_k y^k with 0 <= y <= 1, so it moves p by at most its own
        error; p is of the size of its largest coefficient (PA, PB, PC and QB start with it, QA and QC have c_0 = 0), so every
        coefficient may be off by (eps / 64) max_k |c_k| and the 16 of them move p by at most eps / 4 of its size;
      * a Chebyshev coefficient moves g(t) = sum c_j T_j by at most its own error, |T_j| <= 1, and g is within a factor 2 of c_0
        (sqrt(pi / 2) at t = 0, decreasing in t for order <= 1/2 and increasing beyond): (eps / 128) |c_0| each, 25 of them eps / 5 of g.
    The recurrences in the order that follow only add positive multiples of these terms from j = 1 on."""
    nus, _, _, ref = golden
    for i, nu in enumerate(nus):
        status, T = library_tables(nu)
        assert status == 0 and np.all(np.isfinite(T)), nu
        R = ref[i]
        for w in (tw.W_N, tw.W_MU, tw.W_NU):
            assert T[w] == R[w], (nu, w)
        assert T[tw.W_N] == np.floor(nu + 0.5) and T[tw.W_MU] == nu - T[tw.W_N] and -0.5 <= T[tw.W_MU] < 0.5
        for w in (tw.W_HP, tw.W_HQ, tw.W_G1, tw.W_G2, tw.W_CS, tw.W_CC, tw.W_CA):
            assert abs(T[w] - R[w]) <= 0.25 * EPS * abs(R[w]), (nu, w, T[w], R[w])
        assert np.array_equal(T[10:16], np.zeros(6))
        for off in (tw.W_PA, tw.W_PB, tw.W_PC, tw.W_QA, tw.W_QB, tw.W_QC):
            c, r = T[off:off + tw.NSER], R[off:off + tw.NSER]
            assert np.abs(c - r).max() <= EPS / 64.0 * np.abs(r).max(), (nu, off)
        for off in (tw.W_CH0, tw.W_CH1):
            c, r = T[off:off + tw.NCHEB], R[off:off + tw.NCHEB]
            assert np.abs(c - r).max() <= EPS / 128.0 * abs(r[0]), (nu, off)
        again = library_tables(nu)[1]
        assert np.array_equal(again, T)          # two calls, the same bits
    assert tw.WORDS == _lib.MATERN_TABLE_WORDS == 162


def test_table_rejections():
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0, np.nextafter(0.125, 0.0), np.nextafter(8.0, 9.0), 8.5, 1e300):
        status, T = library_tables(bad)
        assert status == HFMI_ERR_INVALID and np.all(np.isnan(T)), bad          # nothing is written
    assert "nu" in _lib.load().hfmi_last_error().decode()
    assert library_tables(0.125)[0] == 0 and library_tables(8.0)[0] == 0
    assert _lib.load().hfmi_kernel_matern_tables(1.0, None) == HFMI_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- 3. the host
def line(a):
    return np.concatenate([[0.0], a])[:, None]


def test_host_against_forty_digits(golden):
    """kernel_cov_host(family="matern", nu=...) goes through scipy.special.kve: within 1024 eps of the 40-digit values, plus the abscissa
    term 2 a eps (the host's a = sqrt(2 nu) (a / sqrt(2 nu)) is two roundings away from the fixture's and |d ln phi / d ln a| <= a, as in
    the Matern-1 host test).  Measured: 465.8 eps beyond the abscissa term (nu = 0.125 at a = 2, kve's own error for orders that are not
    half-integers; 2 to 17 eps for nu = 0.5, 1 and everything from 1.5 on)."""
    nus, a, ref, _ = golden
    m = (a > 0.0) & (a <= 700.0)
    worst = 0.0
    for i, nu in enumerate(nus):
        x = a / np.sqrt(2.0 * nu)
        row = hf.kernel_cov_host(line(x), "matern", 1.0, 1.0, nu=float(nu))[0, 1:]
        rel = np.abs(row[m] - ref[i][m]) / ref[i][m] / EPS
        over = (rel - 2.0 * a[m]).max()
        print("matern nu = %.10g host: %.1f eps beyond 2 a eps" % (nu, over))
        worst = max(worst, over)
        assert np.all(rel <= 1024.0 + 2.0 * a[m]), nu
        assert row[0] == 1.0 and np.all(np.isfinite(row)) and np.all(row[-2:] >= 0.0) and np.all(row[-2:] <= 1e-300)
    print("matern nu host: worst %.1f eps" % worst)


@pytest.mark.parametrize("nu,named", [(0.5, "matern12"), (1.5, "matern32"), (2.5, "matern52"), (1.0, "matern1")])
def test_host_agrees_with_the_named_families(golden, nu, named):
    """no dispatch: the general evaluation, held to the named family's closed form by the same bound"""
    a = golden[1]
    a = a[a <= 700.0]
    x = a / np.sqrt(2.0 * nu)
    got = hf.kernel_cov_host(line(x), "matern", 1.3, 1.0, nu=nu)[0, 1:]
    ref = hf.kernel_cov_host(line(x), named, 1.3, 1.0)[0, 1:]
    assert np.all(np.abs(got - ref) <= (1024.0 + 2.0 * a) * EPS * ref)
    assert got[0] == ref[0] == 1.3 ** 2


def scattered(N, d, seed):
    pts = np.random.default_rng(seed).random((N, d))
    pts[N - 1] = pts[1]
    return pts


@pytest.mark.parametrize("d", [1, 2, 3])
def test_host_metric_rows_and_cross_form(d):
    N, sigma, ell, nugget, nu = 31, 1.3, 0.4, 0.25, 0.75
    pts = scattered(N, d, seed=20 + d)
    A = np.random.default_rng(d).standard_normal((d, d))
    G = A @ A.T + 0.5 * np.eye(d)
    full = hf.kernel_cov_host(pts, "matern", sigma, ell, nugget, nu=nu, metric=G)
    assert np.all(np.isfinite(full)) and np.array_equal(full, full.T)
    assert full[1, N - 1] == sigma ** 2 and full[1, 1] == sigma ** 2 + nugget       # coincident points: phi(0) = 1, no nugget
    iso = hf.kernel_cov_host(pts @ np.linalg.cholesky(G), "matern", sigma, ell, nugget, nu=nu)
    assert np.allclose(full, iso, rtol=64 * EPS, atol=0.0)
    for r0, r1 in ((0, N), (7, 30), (N - 1, N)):
        K = hf.kernel_cross_cov_host(pts[r0:r1], pts, "matern", sigma, ell, nugget, diag_offset=r0, nu=nu, metric=G)
        assert np.array_equal(K, full[r0:r1])
        assert np.array_equal(K, hf.kernel_cov_host(pts, "matern", sigma, ell, nugget, rows=range(r0, r1), nu=nu, metric=G))
    assert np.array_equal(hf.kernel_cov_host(pts, "matern", sigma, ell, nugget, nu=nu, metric=np.eye(d)),
                          hf.kernel_cov_host(pts, "matern", sigma, ell, nugget, nu=nu))


def test_argument_rules_on_the_host():
    pts = scattered(9, 2, seed=0)
    with pytest.raises(ValueError):
        hf.kernel_cov_host(pts, "matern", 1.0, 0.2)                      # the family needs its smoothness
    for family in ("matern12", "matern32", "matern52", "sqexp", "matern1"):
        with pytest.raises(ValueError):
            hf.kernel_cov_host(pts, family, 1.0, 0.2, nu=1.5)            # and no other family takes one
        with pytest.raises(ValueError):
            hf.kernel_cross_cov_host(pts[:3], pts, family, 1.0, 0.2, nu=1.5)
    for bad in (0.0, 0.1, 8.5, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            hf.kernel_cov_host(pts, "matern", 1.0, 0.2, nu=bad)
        with pytest.raises(ValueError):
            hf.kernel_cross_cov_host(pts[:3], pts, "matern", 1.0, 0.2, nu=bad)
    with pytest.raises(ValueError):
        hf.kernel_cov_host(pts, "matern72", 1.0, 0.2)
    with pytest.raises(TypeError):
        hf.kernel_cov_host(pts, "matern", 1.0, 0.2, 0.0, None, 1.5)     # nu is keyword only
    # nu sits before metric and metric stays last: what splats of bilaplacian_kernel_2d and whittle_matern_kernel rely on
    kw = hf.whittle_matern_kernel(0.1, 1.0, 2.0, 2)
    for cls in (hf.KernelCovarianceOperator, hf.KernelCrossCovarianceOperator, hf.KernelCovarianceRowsOperator, hf.GridKernelCovarianceOperator):
        params = inspect.signature(cls.__init__).parameters
        assert set(kw) <= set(params) and list(params)[-2:] == ["nu", "metric"]
        assert params["nu"].kind is inspect.Parameter.KEYWORD_ONLY and params["nu"].default is None
    for fn in (hf.kernel_cov_host, hf.kernel_cross_cov_host):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["nu", "metric"] and params["nu"].kind is inspect.Parameter.KEYWORD_ONLY


# ---------------------------------------------------------------------------------------------------------------- 4. whittle_matern_kernel
def test_whittle_matern_is_the_bilaplacian_at_alpha_2_d_2():
    gamma, delta = 0.1, 1.0
    Theta = hf.anisotropy_2d(2.0, 0.5, np.pi / 4)
    kw, bl = hf.whittle_matern_kernel(gamma, delta, 2, 2, Theta), hf.bilaplacian_kernel_2d(gamma, delta)
    assert kw["family"] == "matern" and kw["nu"] == 1.0 and set(kw) == {"family", "sigma", "ell", "nu", "metric"}
    assert bl["family"] == "matern1" and "nu" not in bl
    assert np.isclose(kw["sigma"], bl["sigma"], rtol=8 * EPS) and np.isclose(kw["ell"], bl["ell"], rtol=4 * EPS)
    assert np.allclose(kw["metric"], bl["metric"], rtol=16 * EPS, atol=0.0)
    pts = scattered(12, 2, seed=3)
    assert np.allclose(hf.kernel_cov_host(pts, **kw), hf.kernel_cov_host(pts, **bl), rtol=1100 * EPS, atol=0.0)


def test_whittle_matern_closed_forms():
    gamma, delta = 0.3, 1.7
    kappa = np.sqrt(delta / gamma)
    x = np.array([0.0, 0.05, 0.4, 1.3, 5.0])
    # alpha = 1, d = 1: (delta - gamma d^2/dx^2)^-1 has the kernel exp(-kappa |x|) / (2 kappa gamma)
    kw = hf.whittle_matern_kernel(gamma, delta, 1, 1)
    assert kw["nu"] == 0.5 and np.array_equal(kw["metric"], np.eye(1))
    row = hf.kernel_cov_host(x[:, None], **kw)[0]
    assert np.allclose(row, np.exp(-kappa * x) / (2.0 * kappa * gamma), rtol=1100 * EPS, atol=0.0)
    # alpha = 2, d = 3: nu = 1/2 again, exp(-kappa r) / (8 pi kappa gamma^2)
    kw = hf.whittle_matern_kernel(gamma, delta, 2, 3)
    assert kw["nu"] == 0.5 and kw["metric"].shape == (3, 3)
    pts = np.zeros((x.size, 3))
    pts[:, 1] = x
    row = hf.kernel_cov_host(pts, **kw)[0]
    assert np.allclose(row, np.exp(-kappa * x) / (8.0 * np.pi * kappa * gamma ** 2), rtol=1100 * EPS, atol=0.0)
    # Theta = t I is the same operator as gamma -> t gamma: the same kernel, distance and variance together
    a, b = hf.whittle_matern_kernel(gamma, delta, 1.75, 2, 4.0 * np.eye(2)), hf.whittle_matern_kernel(4.0 * gamma, delta, 1.75, 2)
    q = np.array([[0.0, 0.0], [0.3, -0.2]])
    assert np.allclose(hf.kernel_cov_host(q, **a), hf.kernel_cov_host(q, **b), rtol=64 * EPS)


def test_whittle_matern_against_the_radial_fourier_integral():
    """alpha = 1.75, d = 2 (nu = 0.75): c(r) = (1 / 2 pi) int_0^inf J_0(xi r) xi / (gamma^alpha (kappa^2 + xi^2)^alpha) d xi, integrated
    between consecutive zeros of J_0 (2000 of them).  The pieces alternate in sign and decrease, so the mean of the last two partial
    sums is off by less than the last piece, ~ (2000 pi)^(1 - 2 alpha - 1/2) relative = 4e-12; each piece is integrated to 1e-13
    absolute.  rtol 1e-8 leaves room for 2000 of those."""
    from scipy.integrate import quad
    from scipy.special import j0, jn_zeros
    gamma, delta, alpha = 0.1, 1.0, 1.75
    kappa2 = delta / gamma
    kw = hf.whittle_matern_kernel(gamma, delta, alpha, 2)
    assert kw["nu"] == 0.75 and kw["ell"] == np.sqrt(2.0 * 0.75 * gamma / delta)
    zeros = np.concatenate([[0.0], jn_zeros(0, 2000)])
    worst = 0.0
    for r in (0.1, 0.35, 1.0, 2.5):
        f = lambda xi: j0(xi * r) * xi / (gamma ** alpha * (kappa2 + xi * xi) ** alpha)      # noqa: E731
        pieces = np.array([quad(f, zeros[i] / r, zeros[i + 1] / r, epsabs=1e-13, epsrel=1e-13)[0] for i in range(zeros.size - 1)])
        ref = (pieces[:-1].sum() + 0.5 * pieces[-1]) / (2.0 * np.pi)
        got = hf.kernel_cov_host(np.array([[0.0, 0.0], [0.6 * r, 0.8 * r]]), **kw)[0, 1]
        worst = max(worst, abs(got - ref) / ref)
    print("whittle_matern_kernel(alpha = 1.75, d = 2) against the radial Fourier integral: worst relative error %.3g" % worst)
    assert worst <= 1e-8


def test_whittle_matern_rejections():
    for alpha, d in ((1.0, 2), (0.5, 1), (1.5, 3), (9.5, 2), (np.nan, 2)):      # nu = 0, 0, 0, 8.5, nan
        with pytest.raises(ValueError):
            hf.whittle_matern_kernel(0.1, 1.0, alpha, d)
    for bad in (dict(gamma=0.0), dict(delta=-1.0), dict(d=4), dict(Theta=[[1.0, 2.0], [2.0, 1.0]])):
        args = dict(gamma=0.1, delta=1.0, alpha=2.0, d=2)
        args.update(bad)
        with pytest.raises(ValueError):
            hf.whittle_matern_kernel(**args)
    assert hf.whittle_matern_kernel(0.1, 1.0, 1.125, 2)["nu"] == 0.125 and hf.whittle_matern_kernel(0.1, 1.0, 9.5, 3)["nu"] == 8.0


# ---------------------------------------------------------------------------------------------------------------- 5. ABI bookkeeping
PAIRS = (("hfmi_op_kernel_cov_spec", "hfmi_op_kernel_cov_spec2"), ("hfmi_op_kernel_cross_cov_spec", "hfmi_op_kernel_cross_cov_spec2"),
         ("hfmi_op_kernel_cov_rows_spec", "hfmi_op_kernel_cov_rows_spec2"), ("hfmi_op_kernel_cov_grid_spec", "hfmi_op_kernel_cov_grid_spec2"),
         ("hfmi_op_kernel_cov_grid_long", "hfmi_op_kernel_cov_grid_long_spec2"))


def test_abi_bookkeeping():
    header = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    assert re.search(r"#define HFMI_KERNEL_MATERN 5\b", header) and _lib.KERNEL_FAMILIES["matern"] == 5
    assert sorted(_lib.KERNEL_FAMILIES.values()) == list(range(6)) and "matern72" not in _lib.KERNEL_FAMILIES
    assert float(re.search(r"#define HFMI_MATERN_NU_MIN (\S+)", header).group(1)) == _lib.MATERN_NU_MIN == 0.125
    assert float(re.search(r"#define HFMI_MATERN_NU_MAX (\S+)", header).group(1)) == _lib.MATERN_NU_MAX == 8.0
    assert int(re.search(r"#define HFMI_MATERN_TABLE_WORDS (\d+)", header).group(1)) == _lib.MATERN_TABLE_WORDS
    struct = re.search(r"typedef struct hfmi_kernel_spec2 \{(.*?)\} hfmi_kernel_spec2;", header, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert [s.strip() for s in struct.split(";") if s.strip()] == ["int family", "int d", "double sigma, ell, nugget", "double metric[9]",
                                                                   "double nu"]
    assert list(_lib.KernelSpec2._fields_) == list(_lib.KernelSpec._fields_) + [("nu", ctypes.c_double)]
    assert ctypes.sizeof(_lib.KernelSpec2) == ctypes.sizeof(_lib.KernelSpec) + 8 == 8 + 3 * 8 + 9 * 8 + 8
    assert _lib.KernelSpec2.nu.offset == ctypes.sizeof(_lib.KernelSpec)
    squeeze = lambda s: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", s, flags=re.S)).strip()      # noqa: E731
    for old, new in PAIRS:
        proto_old = re.search(r"HFMI_API int %s\(([^;]*)\);" % old, header).group(1)
        proto_new = re.search(r"HFMI_API int %s\(([^;]*)\);" % new, header).group(1)
        assert squeeze(proto_new) == squeeze(proto_old).replace("const hfmi_kernel_spec* spec", "const hfmi_kernel_spec2* spec"), new
        so, sn = _lib.SIGNATURES[old], _lib.SIGNATURES[new]
        i = so.index(ctypes.POINTER(_lib.KernelSpec))
        assert sn == so[:i] + [ctypes.POINTER(_lib.KernelSpec2)] + so[i + 1:], new
        assert hasattr(_lib.load(), new)
    assert _lib.SIGNATURES["hfmi_kernel_matern_tables"] == [ctypes.c_double, ctypes.c_void_p]
    # the old descriptor's creators stop at HFMI_KERNEL_MATERN1, the bare ones at HFMI_KERNEL_SQEXP (the GPU suite asks them with family 5)
    src = open(os.path.join(ROOT, "hippyflow_amd", "csrc", "hfmi_op.hip")).read()
    for old, _ in PAIRS:
        body = re.search(r'extern "C" int %s\(.*?\n\}' % old, src, flags=re.S).group(0)
        assert "HFMI_KERNEL_MATERN1, mL, out" in body and "spec2" not in body, old


def test_entry_points_without_a_context():
    lib = _lib.load()
    pts, n, h = np.zeros((3, 2)), np.array([3, 1], dtype=np.int64), np.array([0.5, 0.5])
    out = ctypes.c_void_p()
    for family, nu in ((5, 1.25), (1, 0.0)):
        spec = _lib.KernelSpec2(family, 2, 1.0, 0.1, 0.0)
        spec.nu = nu
        sp, o = ctypes.byref(spec), ctypes.byref(out)
        assert lib.hfmi_op_kernel_cov_spec2(None, _lib.ptr(pts), 3, 2, sp, o) == HFMI_ERR_INVALID
        assert lib.hfmi_op_kernel_cross_cov_spec2(None, _lib.ptr(pts), 3, _lib.ptr(pts), 3, 2, sp, 0, o) == HFMI_ERR_INVALID
        assert lib.hfmi_op_kernel_cov_rows_spec2(None, _lib.ptr(pts), 3, 2, sp, 0, 2, o) == HFMI_ERR_INVALID
        assert lib.hfmi_op_kernel_cov_grid_spec2(None, 2, _lib.ptr(n), _lib.ptr(h), None, 3, sp, o) == HFMI_ERR_INVALID
        assert lib.hfmi_op_kernel_cov_grid_long_spec2(None, 2, _lib.ptr(n), _lib.ptr(h), None, 3, sp, o) == HFMI_ERR_INVALID
        assert out.value is None
    assert lib.hfmi_op_kernel_cov_spec2(None, _lib.ptr(pts), 3, 2, None, ctypes.byref(out)) == HFMI_ERR_INVALID
    # the old descriptor with family 5: refused by the descriptor's own range, context or not
    old = _lib.KernelSpec(5, 2, 1.0, 0.1, 0.0)
    assert lib.hfmi_op_kernel_cov_spec(None, _lib.ptr(pts), 3, 2, ctypes.byref(old), ctypes.byref(out)) == HFMI_ERR_INVALID
