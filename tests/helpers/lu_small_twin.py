"""numpy twin of k_lu_solve (hippyflow_amd/csrc/hfmi_lu.hip): X = W^-1 Z by right-looking blocked LU with partial
pivoting, the right-hand sides carried as extra columns right of W, then back substitution.  Test infrastructure only
(the CPU suite checks the recurrences here against LAPACK; the GPU suite checks the kernel)."""
import numpy as np

LU_LDS_BYTES = 163840
LU_BOOK_BYTES = (64 + 64 + 256 + 128) * 8
EPS = np.finfo(np.float64).eps


def lu_panel_width(m):
    """the launcher's choice: one panel (the whole matrix in LDS) while m x (m|1) doubles fit beside the bookkeeping,
    otherwise the widest multiple of 16 whose m x (nb|1) panel fits"""
    avail = (LU_LDS_BYTES - LU_BOOK_BYTES - 64) // 8
    if m * (m | 1) <= avail:
        return m
    return ((avail // m) - 1) & ~15


def lu_solve_blocked(W, Z, nb=None, full=False):
    """returns (X, min |pivot|, max |pivot|, failed) with the kernel's status rule; full=True appends (LU, piv): the
    factored working copy as the kernel leaves it (L below the diagonal, U on and above; a panel's row swaps reach the
    columns to its RIGHT only, so the L columns of earlier panels keep the rows they had -- lu_factors() sorts that
    out) and piv[j] = the row swapped with row j at step j.  Non-finite input (failed == 1) has neither: zeros."""
    W = np.asarray(W, dtype=np.float64)
    m = W.shape[0]
    nb = lu_panel_width(m) if nb is None else nb
    ipiv = np.arange(m)
    if not (np.isfinite(W).all() and np.isfinite(Z).all()):
        return (np.zeros((m, m)), 0.0, 0.0, 1) + ((np.zeros((m, m)), ipiv) if full else ())
    A = np.hstack([W.copy(), np.asarray(Z, dtype=np.float64).copy()])   # [W | Z]: columns >= m are the right-hand sides
    invd = np.zeros(m)
    pmin, pmax = np.inf, 0.0
    for j0 in range(0, m, nb):
        nbc = min(nb, m - j0)
        pn = A[j0:, j0:j0 + nbc].copy()                                  # 1. the panel (LDS)
        piv = np.zeros(nbc, dtype=int)
        for jj in range(nbc):
            p = jj + int(np.argmax(np.abs(pn[jj:, jj])))                  # first row of largest |entry|
            piv[jj] = p
            if p != jj:
                pn[[jj, p]] = pn[[p, jj]]
            pv = pn[jj, jj]
            inv = 1.0 / pv if pv != 0.0 else 0.0
            invd[j0 + jj] = inv
            pmin, pmax = min(pmin, abs(pv)), max(pmax, abs(pv))
            l = pn[jj + 1:, jj] * inv
            pn[jj + 1:, jj + 1:] -= np.outer(l, pn[jj, jj + 1:])
            pn[jj + 1:, jj] = l
        A[j0:, j0:j0 + nbc] = pn                                         # 2. back, swaps on the columns to the right
        ipiv[j0:j0 + nbc] = j0 + piv
        right = slice(j0 + nbc, 2 * m)
        for jj in range(nbc):
            p = j0 + piv[jj]
            if p != j0 + jj:
                A[[j0 + jj, p], right] = A[[p, j0 + jj], right]
        for t in range(nbc - 1):                                         # 3. U12 = L11^-1 A12, row by row
            A[j0 + t + 1:j0 + nbc, right] -= np.outer(pn[t + 1:nbc, t], A[j0 + t, right])
        if m - j0 > nbc:                                                 # 4. A22 -= L21 U12
            A[j0 + nbc:, right] -= pn[nbc:, :nbc] @ A[j0:j0 + nbc, right]
    X = A[:, m:]
    extra = (A[:, :m].copy(), ipiv) if full else ()
    for t in range(m - 1, 0, -1):                                        # back substitution, rows scaled at the end
        X[:t] -= np.outer(A[:t, t], X[t] * invd[t])
    X *= invd[:, None]
    if not (np.isfinite(X).all() and np.isfinite(pmin) and np.isfinite(pmax)):
        return (np.zeros((m, m)), pmin, pmax, 3) + extra                 # overflow during the elimination
    failed = 0 if pmin > m * EPS * pmax else 2
    return (X.copy(), pmin, pmax, failed) + extra


def lu_factors(LU, piv, nb=None):
    """(L, U, perm) with W[perm] = L U from the working copy and the swaps of lu_solve_blocked(full=True) or of the
    kernel: the swaps of the panels after a column's own are applied to that column of L, which the elimination
    leaves undone because nobody reads it again."""
    LU = np.asarray(LU)
    m = LU.shape[0]
    nb = lu_panel_width(m) if nb is None else nb
    L = np.tril(LU, -1)
    perm = np.arange(m)
    for j in range(m):
        p = int(piv[j])
        if p != j:
            perm[[j, p]] = perm[[p, j]]
            done = (j // nb) * nb                                         # columns of the panels before step j's
            L[[j, p], :done] = L[[p, j], :done]
    return L + np.eye(m, dtype=LU.dtype), np.triu(LU), perm
