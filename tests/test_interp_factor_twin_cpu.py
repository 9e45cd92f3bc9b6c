"""The numpy twin of the factor K = F F^T, F = [W S | diag(sqrt(delta))], of the interpolated grid covariance
(tests/helpers/interp_factor_twin.py) against the dense K of ``interp_twin.dense_K``: F F^T = K to rounding on definite embeddings,
K + W E W^T with |W E W^T| <= 1.25^(2 d) cov_error_bound on a clipped one, and F^T is the transpose of F.  No device: the GPU suite
(tests/test_gpu_interp_factor.py) holds the device to the public steps and to this twin."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_factor_twin as gf                     # noqa: E402
import grid_sampler_twin as gs                    # noqa: E402
import interp_factor_twin as tw                   # noqa: E402

EPS = tw.EPS
CASES = [(c, nug) for c in tw.CPU_CASES for nug in tw.NUGGETS]
IDS = ["%s-nugget%g" % (c[0], nug) for c, nug in CASES]


@pytest.mark.parametrize("case,nugget", CASES, ids=IDS)
def test_definite_embeddings_factor_K(case, nugget):
    """max |F F^T - K| <= 64 eps log2(Ptot) sigma^2 1.25^(2 d) + 4 eps (sigma^2 + nugget): the grid twin's tolerance for S S^T - Cg passed
    through two rows of W (1-norm at most 1.25^d each), and the rounding of adding delta to a diagonal of that size."""
    name, grid, family, ell, growth, ratio = case
    t = tw.build(grid, family, ell, growth, nugget=nugget)
    lam = t["lam"]
    assert lam.min() > 0.0 and abs(lam.min() / lam.max() / ratio - 1.0) < 0.05
    F = tw.dense_F(t)
    assert F.shape == (t["N"], t["Ptot"] + t["N"])
    err = np.abs(F @ F.T - t["K"]).max()
    tol = gf.twin_tolerance(t["Ptot"], tw.SIGMA, 0.0) * 1.25 ** (2 * t["d"]) + 4.0 * EPS * (tw.SIGMA ** 2 + nugget)
    print("F F^T - K %s nugget %g (Ptot = %d): %.3g (tolerance %.3g), lambda_min / lambda_max = %.3g" % (name, nugget, t["Ptot"], err, tol, lam.min() / lam.max()))
    assert err <= tol
    # the tail block of F is diag(sqrt(delta)) in point order, the head is W S
    assert np.array_equal(F[:, t["Ptot"]:], np.diag(np.sqrt(t["delta"])))


@pytest.mark.parametrize("case,nugget", CASES, ids=IDS)
def test_the_transpose_twin_is_adjoint(case, nugget):
    """<F xi, x> = <xi, F^T x> to 64 eps relative to |F xi| |x|, for 1, 2, 3 and 5 columns; F^T X against dense_F^T X"""
    name, grid, family, ell, growth, _ = case
    t = tw.build(grid, family, ell, growth, nugget=nugget)
    F = tw.dense_F(t)
    rng = np.random.default_rng(t["Ptot"])
    worst = 0.0
    for k in (1, 2, 3, 5):
        Xi, X = rng.standard_normal((t["Ptot"] + t["N"], k)), rng.standard_normal((t["N"], k))
        worst = max(worst, tw.adjoint_defect(t, Xi, X).max())
        scale = 64.0 * EPS * np.linalg.norm(F, 2)
        assert np.abs(tw.apply_Ft(t, X) - F.T @ X).max() <= scale * np.linalg.norm(X, axis=0).max()
        assert np.abs(tw.apply_F(t, Xi) - F @ Xi).max() <= scale * np.linalg.norm(Xi, axis=0).max()
    print("adjointness %s nugget %g: worst defect %.3g (allowed %.3g)" % (name, nugget, worst, 64.0 * EPS))
    assert worst <= 64.0 * EPS


@pytest.mark.parametrize("nugget", tw.NUGGETS)
def test_a_clipped_embedding_misses_K_by_the_reported_bound(nugget):
    """d2, matern52, ell 0.45 at growth 0: S S^T = Cg + E with |E_ij| <= bound, the grid twin's clip bound, so F F^T - K = W E W^T and
    max |F F^T - K| <= 1.25^(2 d) bound; the defect is far above rounding level, so the inequality says something."""
    grid, family, ell, growth, ratio = tw.CLIPPED_CASE
    t = tw.build(grid, family, ell, growth, nugget=nugget)
    lam = t["lam"]
    info = gs.info(t["shape"], t["h"], family, tw.SIGMA, ell, 0.0, max_growth=growth, clip=True)
    assert info["growth"] == growth and info["n_clipped"] > 0 and abs(lam.min() / lam.max() / ratio - 1.0) < 0.05
    bound = info["cov_error_bound"]
    F = tw.dense_F(t)
    err = np.abs(F @ F.T - t["K"]).max()
    rounding = gf.twin_tolerance(t["Ptot"], tw.SIGMA, 0.0) * 1.25 ** (2 * t["d"]) + 4.0 * EPS * (tw.SIGMA ** 2 + nugget)
    print("clipped %s nugget %g: max |F F^T - K| %.4g, 1.25^(2d) bound %.4g (bound %.4g), rounding level %.3g" % (grid, nugget, err, 1.25 ** (2 * t["d"]) * bound, bound, rounding))
    assert err <= 1.25 ** (2 * t["d"]) * bound
    assert err > 1000.0 * rounding
