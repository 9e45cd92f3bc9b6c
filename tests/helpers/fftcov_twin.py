"""A numpy statement of the FFT apply of a kernel covariance on a regular grid (hfmi_op_kernel_cov_grid, hfmi_fftcov.hip): the
embedding rule, the node map, the pairing of columns and the nugget, with ``numpy.fft`` for the transforms.  It says WHAT the operator
computes, not in which order the device's passes run; tests/test_fftcov_twin_cpu.py holds it to the dense host covariance, and the GPU
suite shares its case table and its bound."""
import numpy as np

EPS = np.finfo(np.float64).eps
FAMILIES = ("matern12", "matern32", "matern52", "sqexp")


def embed_len(n):
    """the smallest power of two >= 2 n - 1 (1 for n = 1)"""
    P = 1
    while P < 2 * n - 1:
        P *= 2
    return P


def phi(family, r):
    if family == "matern12":
        return np.exp(-r)
    if family == "matern32":
        a = np.sqrt(3.0) * r
        return (1.0 + a) * np.exp(-a)
    if family == "matern52":
        a = np.sqrt(5.0) * r
        return (1.0 + a + a * a / 3.0) * np.exp(-a)
    if family == "sqexp":
        return np.exp(-0.5 * r * r)
    raise ValueError(family)


def first_column(shape, spacing, family, sigma, ell, nugget):
    """the circulant's first column as an array of shape (P_{d-1}, ..., P_0) (axis 0 of the grid is the LAST numpy axis: it varies fastest)"""
    P = [embed_len(n) for n in shape]
    r2 = np.zeros(P[::-1])
    for c, (Pc, h) in enumerate(zip(P, spacing)):
        j = np.arange(Pc)
        off = np.minimum(j, Pc - j) * h
        r2 = r2 + (off ** 2).reshape([-1 if a == c else 1 for a in range(len(P))][::-1])
    col = sigma ** 2 * phi(family, np.sqrt(r2) / ell)
    col[(0,) * len(P)] += nugget
    return col


def points(shape, spacing, nodes=None, origin=None):
    """(N, d) coordinates origin + index * spacing of the nodes, node g = i0 + n0 (i1 + n1 i2)"""
    g = np.arange(int(np.prod(shape))) if nodes is None else np.asarray(nodes, dtype=np.int64)
    out = np.empty((g.size, len(shape)))
    for c, n in enumerate(shape):
        out[:, c] = (0.0 if origin is None else origin[c]) + (g % n) * spacing[c]
        g = g // n
    return out


def apply(shape, spacing, family, sigma, ell, nugget, W, nodes=None):
    """Y = C W: columns paired from the first (z = w_j + i w_{j+1}, a last odd column with zeros), scattered into the zero-padded grid,
    transformed, multiplied by the real spectrum, transformed back, gathered."""
    shape = tuple(int(n) for n in shape)
    col = first_column(shape, spacing, family, sigma, ell, nugget)
    lam = np.fft.fftn(col).real
    N, k = W.shape
    g = np.arange(int(np.prod(shape))) if nodes is None else np.asarray(nodes, dtype=np.int64)
    assert g.size == N
    idx = []
    rest = g
    for n in shape:
        idx.append(rest % n)
        rest = rest // n
    idx = tuple(idx[::-1])
    Y = np.empty((N, k))
    for j in range(0, k, 2):
        z = np.zeros(col.shape, dtype=np.complex128)
        z[idx] = W[:, j] + (1j * W[:, j + 1] if j + 1 < k else 0.0)
        y = np.fft.ifftn(lam * np.fft.fftn(z))[idx]
        Y[:, j] = y.real
        if j + 1 < k:
            Y[:, j + 1] = y.imag
    return Y


def column_bounds(shape, spacing, family, sigma, ell, nugget, W, absCW):
    """per column j:  32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W[:, j]||_2  +  8 N eps || |C| |W[:, j]| ||_2   (P = prod P_c, c the first
    column with the nugget): Higham's bound for two transforms and the spectrum's own, and the dense reference's summation"""
    col = first_column(shape, spacing, family, sigma, ell, nugget)
    P = col.size
    fft_term = 32.0 * max(1.0, np.log2(P)) * EPS * np.sqrt(P) * np.linalg.norm(col) * np.linalg.norm(W, axis=0)
    return fft_term + 8.0 * W.shape[0] * EPS * np.linalg.norm(absCW, axis=0)


def case_nodes(shape, subset, seed):
    """None (all nodes in order) or a seeded random 3/4 of the nodes in shuffled order"""
    total = int(np.prod(shape))
    if not subset:
        return None
    rng = np.random.default_rng(seed)
    return rng.permutation(total)[:max(1, (3 * total) // 4)].astype(np.int64)


SHAPES = [(1,), (2,), (3,), (16,), (17,), (33,), (2048,),
          (5, 3), (1, 9), (17, 9), (32, 33), (64, 40), (300, 200),
          (7, 5, 3), (9, 8, 5), (33, 2, 17),
          (3, 1)]      # a strided line of one entry
NVECS = (1, 2, 5, 17, 74)
SPACINGS = (0.013, 0.021, 0.017)      # unequal between the axes


def cases():
    """(id, shape, spacing, nodes_kind, nvec, family, ell, nugget, accumulate): every shape with all nodes and with a seeded 3/4 subset,
    (300, 200) also with its first 50000 nodes; family, ell, nugget, accumulate and nvec rotate; one case of 290 columns"""
    out = []
    t = 0
    for shape in SHAPES:
        kinds = ["all", "subset"] + (["first50000"] if shape == (300, 200) else [])
        for kind in kinds:
            nvec = NVECS[t % len(NVECS)]
            if shape == (64, 40) and kind == "all":
                nvec = 290
            out.append(("%s-%s" % ("x".join(map(str, shape)), kind), shape, SPACINGS[:len(shape)], kind, nvec, FAMILIES[t % 4],
                        (0.05, 1.0)[(t // 2) % 2], (0.0, 0.3)[(t // 3) % 2], (t // 5) % 2))
            t += 1
    return out


def nodes_of(shape, kind, seed=0):
    if kind == "all":
        return None
    if kind == "subset":
        return case_nodes(shape, True, seed + int(np.prod(shape)))
    return np.arange(50000, dtype=np.int64)


DENSE_MAX_N = 4096      # up to here the reference is the whole dense product; beyond it, SAMPLE_ROWS seeded rows of it
SAMPLE_ROWS = 512


def reference_rows(N, seed=0):
    """None (all rows) up to DENSE_MAX_N points; beyond, the first and the last row and SAMPLE_ROWS seeded ones, sorted"""
    if N <= DENSE_MAX_N:
        return None
    rng = np.random.default_rng(seed + N)
    return np.unique(np.concatenate([[0, N - 1], rng.choice(N, SAMPLE_ROWS, replace=False)]))


def host_products(hf, pts, family, sigma, ell, nugget, W, rows=None):
    """(C W, |C| |W|) on the rows ``rows`` (None: all) with C = hf.kernel_cov_host(pts, ...)"""
    Cm = hf.kernel_cov_host(pts, family, sigma, ell, nugget, rows=rows)
    return Cm @ W, np.abs(Cm) @ np.abs(W)
