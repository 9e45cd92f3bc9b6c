"""CPU twin of the device V-cycle of hfmi_amg.hip: the same recurrences in the same order, in numpy, on a hierarchy
from hippyflow_amd.amg.  B and the result are (N, k) arrays.

Per level l (all but the coarsest), with the Chebyshev interval [lmin, lmax] of D^-1 A:
  theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta
  smooth(x0, b):  x1 = x0 + D^-1 (b - A x0) / theta;  rho = 1 / sigma
                  x_{n+1} = x_n + rho' rho (x_n - x_{n-1}) + (2 rho' / delta) D^-1 (b - A x_n),  rho' = 1 / (2 sigma - rho)
  x = smooth(0, b);  r = b - A x;  x += P V_{l+1}(R r);  x = smooth(x, b)
Coarsest level: x = A_L^-1 b (the dense inverse)."""
import numpy as np


def chebyshev(level, b, x0, degree):
    A, dinv = level.A, level.inv_diag[:, None]
    theta = 0.5 * (level.lmax + level.lmin)
    delta = 0.5 * (level.lmax - level.lmin)
    sigma = theta / delta
    xp = x0
    x = x0 + dinv * (b - A @ x0) / theta
    rho = 1.0 / sigma
    for _ in range(degree - 1):
        rho_new = 1.0 / (2.0 * sigma - rho)
        x, xp = x + rho_new * rho * (x - xp) + (2.0 * rho_new / delta) * dinv * (b - A @ x), x
        rho = rho_new
    return x


def vcycle(h, B, level=0):
    B = np.asarray(B, dtype=np.float64)
    squeeze = B.ndim == 1
    if squeeze:
        B = B[:, None]
    lv = h.levels[level]
    if level == len(h.levels) - 1:
        X = h.coarse_inv @ B
    else:
        X = chebyshev(lv, B, np.zeros_like(B), h.degree)
        r = B - lv.A @ X
        X = X + lv.P @ vcycle(h, lv.R @ r, level + 1)
        X = chebyshev(lv, B, X, h.degree)
    return X[:, 0] if squeeze else X


def as_linear_operator(h):
    import scipy.sparse.linalg as spla
    n = h.levels[0].A.shape[0]
    return spla.LinearOperator((n, n), matvec=lambda v: vcycle(h, v), matmat=lambda V: vcycle(h, V), dtype=np.float64)
