"""numpy twin of the factor  K = F F^T,  F = [ W S | diag(sqrt(delta)) ]  of the interpolated grid covariance (hfmi_op_interp_factor,
hippyflow_amd/csrc/hfmi_interp.hip; include/hfmi.h states the contract), put together from the twins of its parts: ``interp_twin``
(``cell_and_weights``, ``gather``, ``spread``, ``dense_K``, ``delta_of``) and ``grid_factor_twin`` (``root_spectrum``, ``apply_S``,
``apply_St``).  numpy only.

Noise layout: rows 0 .. Ptot - 1 the padded-grid noise in the grid factor's natural order, rows Ptot .. Ptot + N - 1 one entry per point
in point order.  ``apply_F`` is W (S Xi_top) + sqrt(delta) Xi_tail, ``apply_Ft`` stacks S^T (W^T X) on sqrt(delta) X, ``dense_F`` applies F
to the identity for Ptot + N <= 8192.

The grids and point sets are those of tests/test_gpu_grid_interp.py::_points, restated in ``points``."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grid_factor_twin as gf                     # noqa: E402
import grid_sampler_twin as gs                    # noqa: E402
import interp_twin as it                          # noqa: E402

EPS = np.finfo(np.float64).eps
SIGMA = 1.3
NUGGETS = (0.0, 0.01)
DENSE_MAX = 8192

# (id, grid and points, family, ell, growth, lambda_min / lambda_max of the embedding): definite and bounded away from rounding, which
# the square root needs (the note above GPU_CASES in grid_factor_twin.py)
CPU_CASES = [("d1", "d1", "matern32", 1.0, 0, 5.5e-4),
             ("d2m", "d2", "matern32", 0.3, 1, 2.6e-4)]
# d2 with matern52, ell 0.45 at growth 0: indefinite, lambda_min / lambda_max = -4.2e-3
CLIPPED_CASE = ("d2", "matern52", 0.45, 0, -4.2e-3)


def points(name):
    """(shape, h, o, pts) of a case of tests/test_gpu_grid_interp.py::_points"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "d1":        # n = 9, N = 7: both edge points, two points in one cell, a node
        shape, h, o = (9,), (0.25,), (1.0,)
        u = np.array([[1.0], [7.0], [3.25], [3.75], [5.0], [2.6], [6.1]])
    elif name == "d2":      # 9 x 6, N = 23, 12 of the points in the cell (4, 2)
        shape, h, o = (9, 6), (0.1, 0.13), (0.3, -0.2)
        u = np.concatenate([np.array([4.0, 2.0]) + rng.random((12, 2)), 1.0 + rng.random((11, 2)) * (np.array(shape) - 3)])
        u = u[rng.permutation(23)]
    elif name == "d3":      # 6 x 5 x 7, N = 40
        shape, h, o = (6, 5, 7), (0.07, 0.1, 0.09), (-1.0, 0.25, 2.0)
        u = 1.0 + rng.random((40, 3)) * (np.array(shape) - 3)
    else:                   # 70 x 67, N = 5000 in no order
        shape, h, o = (70, 67), (1.0 / 64, 1.0 / 60), (-0.02, 0.1)
        u = 1.0 + rng.random((5000, 2)) * (np.array(shape) - 3)
    return shape, h, o, np.ascontiguousarray(np.asarray(o) + u * np.asarray(h))


def build(name, family, ell, growth, nugget=0.0, sigma=SIGMA, diag_correction=True, dense=True):
    """everything the applies need of a case: the grid, the points' weights, the root spectrum of the embedding at ``growth`` (negative
    eigenvalues clipped) and delta; ``dense``: delta (and K) from ``interp_twin.dense_K``, otherwise from ``interp_twin.diagonal``"""
    shape, h, o, pts = points(name)
    base, w, _ = it.cell_and_weights(shape, h, o, pts)
    lam = gs.spectrum(shape, h, family, sigma, ell, 0.0, growth)
    t = dict(name=name, shape=shape, h=h, o=o, pts=pts, base=base, w=w, lam=lam, root=gf.root_spectrum(shape, h, family, sigma, ell, 0.0, growth, lam=lam),
             Ptot=int(lam.size), N=pts.shape[0], d=len(shape), sigma=sigma, nugget=nugget)
    if dense:
        t["K"], _, _, t["delta"] = it.dense_K(shape, h, o, pts, family, sigma, ell, nugget, diag_correction)
    else:
        t["delta"] = it.delta_of(it.diagonal(shape, h, family, sigma, ell, w)[0], sigma, nugget, diag_correction)
    return t


def apply_F(t, Xi):
    """(N, k) = F Xi for Xi of Ptot + N rows"""
    P = t["Ptot"]
    g = it.gather(t["shape"], t["base"], t["w"], gf.apply_S(t["root"], t["shape"], Xi[:P]))[0]
    return g + np.sqrt(t["delta"])[:, None] * Xi[P:]


def apply_Ft(t, X):
    """(Ptot + N, k) = F^T X"""
    G = it.spread(t["shape"], t["base"], t["w"], X)[0]
    return np.concatenate([gf.apply_St(t["root"], t["shape"], G), np.sqrt(t["delta"])[:, None] * X])


def dense_F(t):
    n = t["Ptot"] + t["N"]
    assert n <= DENSE_MAX
    return apply_F(t, np.eye(n))


def adjoint_defect(t, Xi, X):
    """per column |<F Xi, X> - <Xi, F^T X>| / (|F Xi| |X|) of the twin itself"""
    FX, FtX = apply_F(t, Xi), apply_Ft(t, X)
    return np.abs(np.sum(FX * X, axis=0) - np.sum(Xi * FtX, axis=0)) / (np.linalg.norm(FX, axis=0) * np.linalg.norm(X, axis=0))
