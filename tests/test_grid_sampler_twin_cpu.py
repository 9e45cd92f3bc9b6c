"""The numpy twin of the grid sampler (tests/helpers/grid_sampler_twin.py) held to what it must be before the device is held to it:
the growth it takes on the seven embeddings whose definiteness is tabulated, the clip's bound against the dense host covariance, the
exactness of the covariance where nothing is clipped, and the statistics of its draws at the seed the GPU suite uses.  No device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_twin as ft                          # noqa: E402
import grid_sampler_twin as tw                    # noqa: E402

hf = pytest.importorskip("hippyflow_amd")

EPS = tw.EPS
STAT_SEED, STAT_DRAWS = tw.STAT_SEED, tw.STAT_DRAWS   # the GPU suite's statistics case: the twin passes it here first


def dense_C(shape, spacing, family, ell, sigma=1.0, nugget=0.0, nodes=None):
    return hf.kernel_cov_host(ft.points(shape, spacing, nodes), family, sigma, ell, nugget)


@pytest.mark.parametrize("shape,spacing,family,ell,growth", tw.TABLE)
def test_growth_of_the_tabulated_embeddings(shape, spacing, family, ell, growth):
    """the sign pattern of lambda_min / lambda_max over g = 0..3 and the growth the rule takes; what is negative by rounding only
    (the squared exponential's rows) sits at least a factor 16 inside the floor, what is genuinely negative a factor 1e6 outside"""
    rec = tw.info(shape, spacing, family, 1.0, ell, 0.0, max_growth=3)
    assert rec["growth"] == growth and rec["n_clipped"] == 0 and rec["cov_error_bound"] == 0.0
    assert rec["embedding"] == [ft.embed_len(n) << growth for n in shape]
    for g in range(4):
        lam = tw.spectrum(shape, spacing, family, 1.0, ell, 0.0, g)
        rel_floor = tw.floor(lam.size, lam.max()) / lam.max()
        ratio = lam.min() / lam.max()
        if g < growth:
            assert ratio < -1e6 * rel_floor, (g, ratio)
        elif ratio < 0.0:
            assert -ratio * 16.0 < rel_floor, (g, ratio, rel_floor)
    for g in range(growth):                              # a smaller max_growth cannot be definite
        with pytest.raises(ValueError, match="lambda_min / lambda_max = -"):
            tw.info(shape, spacing, family, 1.0, ell, 0.0, max_growth=g)


@pytest.mark.parametrize("shape,spacing,family,ell,max_growth", [((8, 8), (0.125, 0.125), "matern52", 1.0, 1),
                                                                 ((13, 5), (0.1, 0.25), "sqexp", 1.0, 0)])
def test_clip_bound_holds(shape, spacing, family, ell, max_growth):
    """every entry of Cov(draw) - C is within cov_error_bound"""
    rec = tw.info(shape, spacing, family, 1.0, ell, 0.0, max_growth=max_growth, clip=True)
    assert rec["growth"] == max_growth and rec["n_clipped"] > 0 and rec["cov_error_bound"] > 0.0
    err = np.abs(tw.dense_cov(shape, spacing, family, 1.0, ell, 0.0, rec["growth"]) - dense_C(shape, spacing, family, ell)).max()
    print("clip %s %s: max |Cov - C| = %.3e, bound %.3e" % (shape, family, err, rec["cov_error_bound"]))
    # on the diagonal the error IS the bound (the clipped circulant's constant diagonal), computed here by two routes that agree to
    # rounding only (measured: 2.1e-17 apart for the first case): the allowance is the one the unclipped comparison below has
    P = int(np.prod(rec["embedding"]))
    assert 0.0 < err <= rec["cov_error_bound"] + 64 * EPS * np.log2(P)


@pytest.mark.parametrize("shape,spacing,family,ell,growth", tw.TABLE)
def test_covariance_is_exact_where_nothing_is_clipped(shape, spacing, family, ell, growth):
    sigma, nugget = 1.3, 0.05
    nodes = ft.case_nodes(shape, len(shape) == 2, 5)
    g = tw.info(shape, spacing, family, sigma, ell, nugget, max_growth=3)["growth"]
    cov = tw.dense_cov(shape, spacing, family, sigma, ell, nugget, g, nodes)
    P = int(np.prod(tw.embedding(shape, g)))
    assert np.abs(cov - dense_C(shape, spacing, family, ell, sigma, nugget, nodes)).max() <= 64 * EPS * np.log2(P) * sigma ** 2


def test_noise_map():
    """entries 2 q, 2 q + 1 share one Philox output; pairs and seeds are separate streams; a prefix of a longer array is the same"""
    a, b = tw.noise(40, 3, 11), tw.noise(17, 3, 11)
    assert np.array_equal(a[:17], b) and not np.array_equal(tw.noise(40, 4, 11), a) and not np.array_equal(tw.noise(40, 3, 12), a)
    x = tw.philox.philox4x32_10(2, 0, 3, tw.STREAM, 11, 0)
    u = [(float(v) + 0.5) * 2.0 ** -32 for v in x]
    r = np.sqrt(-2.0 * np.log(u[2]))
    assert a[5] == r * np.cos(2.0 * np.pi * u[3]) + 1j * (r * np.sin(2.0 * np.pi * u[3]))
    z = np.concatenate([tw.noise(4096, p, 7) for p in range(8)])
    assert abs(z.real.mean()) < 0.03 and abs(z.real.var() - 1.0) < 0.03 and abs((z.real * z.imag).mean()) < 0.03


def test_twin_transform_against_extended_precision():
    """the parity bound of the GPU suite, 64 eps log2(P) sqrt(sigma^2 + nugget) 8, leaves the fp64 twin itself this margin"""
    for shape, spacing, family, ell, _ in tw.TABLE[:2] + tw.TABLE[5:]:
        g = 2 if len(shape) < 3 else 1
        a = tw.draws(shape, spacing, family, 1.0, ell, 0.0, g, 2, 5)
        b = tw.draws(shape, spacing, family, 1.0, ell, 0.0, g, 2, 5, dtype=np.clongdouble)
        P = int(np.prod(tw.embedding(shape, g)))
        bound = 64 * EPS * np.log2(P) * 8.0
        print("%s: twin against long double %.2e, bound %.2e" % (shape, np.abs(a - b).max(), bound))
        assert np.abs(a - b).max() <= bound / 16


def test_parity_cases_are_well_conditioned():
    """The GPU suite holds the device's draws to this twin within ``parity_bound``, which counts the rounding of the transforms.  The
    device and numpy also round Lambda differently, and sqrt(Lambda) turns a perturbation eps lambda_max of an eigenvalue lambda into
    eps lambda_max / (2 sqrt(lambda)): for spectra that reach zero to rounding (the squared exponential without a nugget: measured here
    4e-8 between this twin and the same twin on the extended-precision spectrum, 33 nodes, ell 0.4, growth 2) NO two implementations agree
    to the bound, so the parity cases give the two smoothest families a nugget.  Measured for the 40 cases as they are: at most 0.052
    of the bound (33 nodes, matern32, growth 2); asserted: 1 / 8."""
    worst = 0.0
    for shape, spacing, subset in tw.PARITY_SHAPES:
        for family, (ell, nugget) in tw.PARITY_KERNELS.items():
            for g in tw.PARITY_GROWTHS:
                args = (shape, spacing, family, tw.PARITY_SIGMA, ell, nugget, g)
                a = tw.draws(*args, 8, 5)
                b = tw.draws(*args, 8, 5, lam=tw.spectrum_extended(*args))
                ratio = np.abs(a - b).max() / tw.parity_bound(int(np.prod(tw.embedding(shape, g))), tw.PARITY_SIGMA, nugget)
                worst = max(worst, ratio)
                assert ratio <= 0.125, (shape, family, g, ratio)
    print("parity cases: the spectrum's rounding moves the draws by at most %.3f of the parity bound" % worst)


def test_statistics_of_the_twin_at_the_committed_seed():
    shape, spacing, family, ell = tw.TABLE[0][:4]
    X = tw.draws(shape, spacing, family, 1.0, ell, 0.0, 0, STAT_DRAWS, STAT_SEED)
    Cm = dense_C(shape, spacing, family, ell)
    tol = tw.cov_tolerance(Cm, STAT_DRAWS)
    emp = X @ X.T / STAT_DRAWS
    assert np.all(np.abs(emp - Cm) <= tol), np.abs((emp - Cm) / tol).max()
    re, im = X[:, 0::2], X[:, 1::2]
    cross = re @ im.T / (STAT_DRAWS // 2)
    assert np.all(np.abs(cross) <= tol), np.abs(cross / tol).max()


def test_projection_error_of_the_twin_draws():
    """the consumer check of the GPU suite on the twin: the mean relative projection error of 256 draws on the exact KLE basis is
    non-increasing in the rank and below 1.5 sqrt(sum_{i > r} d_i / sum d_i) at r = 20 (measured: see the print)"""
    shape, spacing, family, ell = tw.TABLE[0][:4]
    Cm = dense_C(shape, spacing, family, ell)
    d, U = np.linalg.eigh(Cm)
    d, U = d[::-1], U[:, ::-1]
    X = tw.draws(shape, spacing, family, 1.0, ell, 0.0, 0, tw.KLE_DRAWS, tw.KLE_SEED)
    errs = []
    for r in tw.KLE_RANKS:
        E = X - U[:, :r] @ (U[:, :r].T @ X)
        errs.append(np.mean(np.linalg.norm(E, axis=0) / np.linalg.norm(X, axis=0)))
    expect = np.sqrt(d[20:].sum() / d.sum())
    print("twin projection errors %s, sqrt(tail / trace) at 20 = %.4f" % (np.round(errs, 4), expect))
    assert all(b <= a for a, b in zip(errs, errs[1:])) and errs[-1] <= 1.5 * expect
