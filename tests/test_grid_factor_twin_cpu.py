"""The numpy twin of the factor C = S S^T of a grid sampler's embedding (tests/helpers/grid_factor_twin.py) against the dense host
covariance: S S^T = C to rounding on definite embeddings, C + E with E on the bound on clipped ones, S^T is the transpose of S, and
what the rounding of the spectrum does to the GPU suite's cases.  No device: the GPU suite holds the device to this twin."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fftcov_twin as ft                          # noqa: E402
import grid_sampler_twin as gs                    # noqa: E402
import grid_factor_twin as tw                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")

EPS = tw.EPS


def dense_case(case):
    shape, spacing, family, ell, nugget, growth = case
    spacing = tw.unit_spacing(shape) if spacing is None else spacing
    lam = gs.spectrum(shape, spacing, family, 1.0, ell, nugget, growth)
    S = tw.dense_S(tw.root_spectrum(shape, spacing, family, 1.0, ell, nugget, growth, lam=lam), shape)
    Cm = hf.kernel_cov_host(ft.points(shape, spacing), family, 1.0, ell, nugget)
    return lam, S, Cm


@pytest.mark.parametrize("case", tw.DEFINITE, ids=["%s-%s-g%d" % ("x".join(map(str, c[0])), c[2], c[5]) for c in tw.DEFINITE])
def test_definite_embeddings_factor_the_covariance(case):
    """max |S S^T - C| <= 64 eps log2(Ptot) (sigma^2 + nugget); measured 8.9e-16, 1.3e-15, 4.4e-16 and 2.4e-15 on the four cases"""
    lam, S, Cm = dense_case(case)
    assert lam.min() > 0.0 and S.shape == (Cm.shape[0], lam.size)
    err = np.abs(S @ S.T - Cm).max()
    tol = tw.twin_tolerance(lam.size, 1.0, case[4])
    print("S S^T - C %s: %.3g (tolerance %.3g)" % (case[:3], err, tol))
    assert err <= tol


@pytest.mark.parametrize("case,ratio,bound", [(tw.CLIPPED[0], -5.1e-3, 1.04e-3), (tw.CLIPPED[1], -1.5e-2, 4.44e-2)], ids=["4x3x3", "9x8"])
def test_clipped_embeddings_miss_by_the_reported_bound(case, ratio, bound):
    """S S^T = C + E with E the restriction of the clipped part: its largest entry is its constant diagonal, which is cov_error_bound.
    max |E| <= bound (1 + 64 eps log2 Ptot) and the diagonal equals the bound to that rounding -- PLUS the rounding of forming S S^T - C
    at all, the definite cases' 64 eps log2(Ptot) (sigma^2 + nugget): the entries of C are O(sigma^2) = 1 and the relative slack alone,
    1.3e-13 of a bound of 1.04e-3, is 1.3e-16, less than one ulp (2.2e-16) of the numbers subtracted.  Measured excess over the bound:
    1.7e-15 at (4, 3, 3), i.e. 8 ulp of C's entries."""
    shape, spacing, family, ell, nugget, growth = case
    spacing = tw.unit_spacing(shape) if spacing is None else spacing
    lam, S, Cm = dense_case(case)
    info = gs.info(shape, spacing, family, 1.0, ell, nugget, max_growth=growth, clip=True)
    assert info["growth"] == growth and info["n_clipped"] > 0
    assert abs(lam.min() / lam.max() / ratio - 1.0) < 0.05 and abs(info["cov_error_bound"] / bound - 1.0) < 0.01
    E = S @ S.T - Cm
    slack = 64.0 * EPS * np.log2(lam.size)
    print("clipped %s: max |S S^T - C| %.4g, bound %.4g" % (shape, np.abs(E).max(), info["cov_error_bound"]))
    rounding = tw.twin_tolerance(lam.size, 1.0, nugget)
    print("  excess over the bound %.3g, rounding allowed %.3g" % (np.abs(E).max() - info["cov_error_bound"], rounding))
    assert np.abs(E).max() <= info["cov_error_bound"] * (1.0 + slack) + rounding
    assert np.abs(np.diag(E) - info["cov_error_bound"]).max() <= info["cov_error_bound"] * slack + rounding


@pytest.mark.parametrize("shape,subset,growth", [((7,), True, 1), ((6, 5), False, 0), ((5, 4), True, 1), ((4, 3, 3), True, 0)])
def test_the_transpose_twin_is_the_transpose(shape, subset, growth):
    """apply_St against dense_S^T, odd and even numbers of columns, with and without a node map; S of a unit padded vector restricted
    to the nodes is a column of Chat^(1/2)"""
    spacing = tw.unit_spacing(shape)
    nodes = ft.case_nodes(shape, subset, 5)
    root = tw.root_spectrum(shape, spacing, "matern32", 1.0, 0.3, 0.0, growth)
    S = tw.dense_S(root, shape, nodes)
    rng = np.random.default_rng(1)
    for k in (1, 2, 3):
        X = rng.standard_normal((S.shape[0], k))
        Xi = rng.standard_normal((S.shape[1], k))
        scale = np.linalg.norm(root) * EPS * 64
        assert np.abs(tw.apply_St(root, shape, X, nodes) - S.T @ X).max() <= scale * np.linalg.norm(X, axis=0).max()
        assert np.abs(tw.apply_S(root, shape, Xi, nodes) - S @ Xi).max() <= scale * np.linalg.norm(Xi, axis=0).max()


@pytest.mark.parametrize("case", [c for c in tw.GPU_CASES if int(np.prod(tw.plan_embedding(c[1], max(c[7])))) <= 1 << 15], ids=lambda c: c[0])
def test_the_spectrums_rounding_stays_inside_the_gpu_bound(case):
    """The device computes Lambda with its own transform.  Replace numpy's spectrum by the extended-precision one (both are within
    rounding of the exact spectrum, as the device's is) and see what that alone does to S Xi and S^T X: at most a quarter of the bound
    the GPU suite allows, for every case of that suite small enough for a dense extended-precision DFT."""
    name, shape, spacing, subset, family, ell, nugget, growths = case
    nodes = tw.gpu_case_nodes(shape, subset)
    rng = np.random.default_rng(2)
    worst = 0.0
    for g in growths:
        lam = gs.spectrum(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, g)
        if lam.size > 1 << 15:
            continue
        lam_x = gs.spectrum_extended(shape, spacing, family, tw.GPU_SIGMA, ell, nugget, g)
        root, root_x = np.sqrt(np.maximum(lam, 0.0)), np.sqrt(np.maximum(lam_x, 0.0))
        N = int(np.prod(shape)) if nodes is None else nodes.size
        Xi, X = rng.standard_normal((lam.size, 3)), rng.standard_normal((N, 3))
        worst = max(worst, (np.abs(tw.apply_S(root, shape, Xi, nodes) - tw.apply_S(root_x, shape, Xi, nodes)).max(axis=0) / tw.column_bounds(root, Xi)).max())
        worst = max(worst, (np.abs(tw.apply_St(root, shape, X, nodes) - tw.apply_St(root_x, shape, X, nodes)).max(axis=0) / tw.column_bounds(root, X)).max())
    print("spectrum rounding %s: worst |delta| / bound = %.3g" % (name, worst))
    assert worst <= 0.25
