"""A numpy statement of the grid kernel covariance with a METRIC and of Matern-1 on a grid (hfmi_op_kernel_cov_grid_spec,
k_fftcov_column_signed of hfmi_fftcov.hip): the signed-offset rule of the circulant's first column.  Everything after the column -- the
embedding lengths, the node map, the pairing of columns -- is tests/helpers/fftcov_twin.py's, which this file leaves alone and reuses.

The rule.  With a metric G the kernel is even in the whole offset vector only, so storage position s_c of axis c stands for the signed
offset  o_c = s_c  if s_c < P_c / 2,  o_c = s_c - P_c  if s_c > P_c / 2.  At s_c = P_c / 2 (P_c >= 2) the entry is the mean of the kernel
over both signs of that offset -- over every axis that sits at its half, in the fixed order b = 0 .. 7 where bit c of b chooses the + sign
on axis c (combinations that flip an axis not at its half are skipped).  An apply never reads a half position (P_c >= 2 n_c wherever
n_c > 1); the mean keeps the column jointly even, so its transform is real.

The distance.  G = L L^T (lower Cholesky factor),  u = diag(h) o,  w = L^T u with w_c = sum_{e >= c} L[e, c] u_e (e ascending),
r^2 = w_0^2 + w_1^2 + w_2^2 in that order,  entry = sigma^2 phi(sqrt(r^2) / ell), the nugget added to entry 0 after the mean.  The device
does the same with fused multiply-adds.
"""
import numpy as np

import fftcov_twin as base
import matern1_twin as m1

EPS = base.EPS
embed_len = base.embed_len
points = base.points


def phi(family, r):
    if family == "matern1":
        return m1.phi(np.sqrt(2.0) * r)
    return base.phi(family, r)


def first_column(shape, spacing, family, sigma, ell, nugget, G=None, growth=0):
    """the circulant's first column as an array of shape (P_{d-1}, ..., P_0) (axis 0 of the grid is the LAST numpy axis); ``growth``: a
    sampler's embedding, every axis of more than one node doubled that many times"""
    d = len(shape)
    P = [(embed_len(n) << growth) if n > 1 else 1 for n in shape]
    Lf = np.eye(d) if G is None else np.linalg.cholesky(np.asarray(G, dtype=np.float64).reshape(d, d))
    view = lambda c: [-1 if a == c else 1 for a in range(d)][::-1]
    o, half = [], []
    for c in range(d):
        s = np.arange(P[c])
        o.append((np.where(2 * s < P[c], s, s - P[c]) * float(spacing[c])).reshape(view(c)))     # at the half: -P_c / 2
        half.append(((P[c] > 1) & (2 * s == P[c])).reshape(view(c)))
    total = np.zeros(P[::-1])
    count = np.zeros(P[::-1])
    for b in range(8):
        if b >> d:
            continue
        valid = np.ones(P[::-1], dtype=bool)
        u = []
        for c in range(d):
            plus = bool(b & (1 << c))
            if plus:
                valid = valid & half[c]
            u.append(-o[c] if plus else o[c])
        r2 = 0.0
        for c in range(d):
            w = Lf[c, c] * u[c]
            for e in range(c + 1, d):
                w = w + Lf[e, c] * u[e]
            r2 = r2 + w * w
        r2 = np.broadcast_to(r2, total.shape)
        total = total + np.where(valid, phi(family, np.sqrt(r2) / ell), 0.0)
        count = count + valid
    col = sigma ** 2 * (total / count)
    col[(0,) * d] += nugget
    return col


def spectrum(shape, spacing, family, sigma, ell, nugget, G=None, growth=0):
    """the complex transform of the column: its imaginary part is rounding"""
    return np.fft.fftn(first_column(shape, spacing, family, sigma, ell, nugget, G, growth))


def apply(shape, spacing, family, sigma, ell, nugget, W, nodes=None, G=None):
    """Y = C W as fftcov_twin.apply has it, with the signed column's real spectrum"""
    shape = tuple(int(n) for n in shape)
    lam = spectrum(shape, spacing, family, sigma, ell, nugget, G).real
    N, k = W.shape
    g = np.arange(int(np.prod(shape))) if nodes is None else np.asarray(nodes, dtype=np.int64)
    assert g.size == N
    idx, rest = [], g
    for n in shape:
        idx.append(rest % n)
        rest = rest // n
    idx = tuple(idx[::-1])
    Y = np.empty((N, k))
    for j in range(0, k, 2):
        z = np.zeros(lam.shape, dtype=np.complex128)
        z[idx] = W[:, j] + (1j * W[:, j + 1] if j + 1 < k else 0.0)
        y = np.fft.ifftn(lam * np.fft.fftn(z))[idx]
        Y[:, j] = y.real
        if j + 1 < k:
            Y[:, j + 1] = y.imag
    return Y


def column_bounds(shape, spacing, family, sigma, ell, nugget, W, absCW, G=None):
    """fftcov_twin.column_bounds with this file's column: per column j
    32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W[:, j]||_2  +  8 N eps || |C| |W[:, j]| ||_2"""
    col = first_column(shape, spacing, family, sigma, ell, nugget, G)
    P = col.size
    fft_term = 32.0 * max(1.0, np.log2(P)) * EPS * np.sqrt(P) * np.linalg.norm(col) * np.linalg.norm(W, axis=0)
    return fft_term + 8.0 * W.shape[0] * EPS * np.linalg.norm(absCW, axis=0)


def rotated_metric():
    """inv(Theta) of the BiLaplacian defaults theta0 = 2, theta1 = 0.5, alpha = pi / 4 (hf.anisotropy_2d, restated)"""
    s, c = np.sin(np.pi / 4), np.cos(np.pi / 4)
    off = (2.0 - 0.5) * s * c
    return np.linalg.inv(np.array([[2.0 * s * s + 0.5 * c * c, off], [off, 2.0 * c * c + 0.5 * s * s]]))


FULL_3D = np.array([[2.0, 0.6, -0.3], [0.6, 1.5, 0.4], [-0.3, 0.4, 0.8]])      # symmetric positive definite, every entry non-zero

# (id, shape, spacing, metric, subset of the nodes): the shapes the CPU and GPU tests share
GRID_CASES = [
    ("6x5", (6, 5), (0.2, 0.25), rotated_metric(), False),
    ("4x3x3", (4, 3, 3), (0.2, 0.25, 0.3), FULL_3D, False),
    ("6x5-subset", (6, 5), (0.2, 0.25), rotated_metric(), True),
]


def case_nodes(shape, subset):
    return base.case_nodes(shape, subset, 7)
