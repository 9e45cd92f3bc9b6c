"""numpy twin of hippyflow_amd/csrc/hfmi_chol_wide.hip: right-looking blocked Cholesky G = R^T R with blocks of 64 columns, the
inverse by block back-substitution from the inverses of the diagonal blocks, and the library's shift / breakdown rule (a pivot
<= pivot_tol * (G_jj + shift) ends the attempt; the second attempt adds shift_rel * trace(G) to the diagonal; a second breakdown
is a failure).  Same block order as the kernels, fp64 throughout.  Test infrastructure only."""
import numpy as np

NB = 64
EPS = 2.220446049250313e-16


def diag_block(s, ref, pivot_tol):
    """S_pp = R_pp^T R_pp column by column (k_cw_diag): returns (R_pp, W_pp = R_pp^-1, min pivot ratio) or None on breakdown"""
    n = s.shape[0]
    m = np.triu(s).copy()
    ratio = 1e300
    for j in range(n):
        piv = m[j, j]
        if not (piv > pivot_tol * ref[j]) or not (ref[j] > 0.0):
            return None
        ratio = min(ratio, piv / ref[j])
        rjj = np.sqrt(piv)
        m[j, j + 1:] *= 1.0 / rjj
        m[j, j] = rjj
        row = m[j, j + 1:]
        m[j + 1:, j + 1:] -= np.triu(np.outer(row, row))
    r = np.triu(m)
    x = np.zeros((n, n))
    for i in range(n - 1, -1, -1):                 # row by row, bottom up
        x[i, i] = 1.0 / r[i, i]
        if i + 1 < n:
            x[i, i + 1:] = -(r[i, i + 1:] @ x[i + 1:, i + 1:]) / r[i, i]
    return r, x, ratio


def _attempt(a, diag0, shift, pivot_tol):
    k = a.shape[0]
    w = np.triu(a).copy()
    w[np.diag_indices(k)] += shift
    ref = diag0 + shift
    r, x = np.zeros((k, k)), np.zeros((k, k))
    nblk = (k + NB - 1) // NB
    ratio = 1e300
    for p in range(nblk):
        j0, j1 = p * NB, min(p * NB + NB, k)
        out = diag_block(w[j0:j1, j0:j1], ref[j0:j1], pivot_tol)
        if out is None:
            return None
        r[j0:j1, j0:j1], x[j0:j1, j0:j1], rt = out
        ratio = min(ratio, rt)
        if j1 < k:
            r[j0:j1, j1:] = x[j0:j1, j0:j1].T @ w[j0:j1, j1:]                   # row panel
            w[j1:, j1:] -= np.triu(r[j0:j1, j1:].T @ r[j0:j1, j1:])              # trailing update, upper tiles
    for p in range(nblk - 2, -1, -1):                                           # R^-1, bottom up
        j0, j1 = p * NB, p * NB + NB
        t = r[j0:j1, j1:] @ x[j1:, j1:]
        x[j0:j1, j1:] = -(x[j0:j1, j0:j1] @ t)
    return r, x, ratio


def chol_wide(g, shift_rel, pivot_tol=0.0):
    """returns (R, R^-1, status) with status = dict(min_pivot_ratio, gram_dev, shifted, failed) -- hfmi_test_chol_wide's words"""
    g = np.asarray(g, dtype=np.float64)
    k = g.shape[0]
    if pivot_tol <= 0.0:
        pivot_tol = 64.0 * k * EPS
    a = 0.5 * (g + g.T)
    diag0 = np.diag(a).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        ivd = np.where(diag0 > 0.0, 1.0 / np.sqrt(np.where(diag0 > 0.0, diag0, 1.0)), 0.0)
        dev = np.sqrt(np.sum((a * ivd[:, None] * ivd[None, :] - np.eye(k)) ** 2))
    tr = np.sum(diag0)
    status = {"min_pivot_ratio": 0.0, "gram_dev": float(dev), "shifted": 0, "failed": 0}
    for attempt in range(2):
        with np.errstate(invalid="ignore", over="ignore"):
            out = _attempt(a, diag0, shift_rel * tr if attempt else 0.0, pivot_tol)
        if out is not None:
            status["min_pivot_ratio"] = float(out[2])
            return out[0], out[1], status
        if attempt == 0:
            status["shifted"] = 1
        else:
            status["failed"] = 1
    return np.zeros((k, k)), np.zeros((k, k)), status


def gram_with_condition(k, cond, seed):
    """G = Z^T Z, Z Gaussian 2k x k with singular values spread so that cond(G) ~ cond"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((2 * k, k))
    u, _, vt = np.linalg.svd(z, full_matrices=False)
    z = (u * np.logspace(0.0, -0.5 * np.log10(cond), k)) @ vt
    return z.T @ z


def qr_shift_rel(n_rows, k):
    """the relative shift the Cholesky-QR passes use (hfmi_qr.hip)"""
    return 11.0 * (n_rows * k + k * (k + 1.0)) * 0.5 * EPS
