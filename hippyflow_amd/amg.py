"""Smoothed-aggregation algebraic multigrid: the host-side hierarchy setup behind ``CsrAMGSolver``.

hippylib solves the elliptic systems of its bi-Laplacian prior, A = delta M + gamma K, with PETSc CG preconditioned by
algebraic multigrid (``BiLaplacianPrior.Asolver``, ``amg_method()``; every ``prior.Rsolver`` apply, R^-1 = A^-1 M A^-1,
costs two such solves).  This module builds the multigrid hierarchy once per matrix, on the host (numpy / scipy);
``hfmi_amg.hip`` runs the V-cycle and the preconditioned block CG on the device.

Setup (smoothed aggregation, Vanek-Mandel-Brezina):

* strength of connection: j is a strong neighbour of i when |a_ij| >= theta sqrt(a_ii a_jj);
* greedy aggregation in three passes: (1) a node whose strong neighbours are all free seeds an aggregate with them,
  (2) a free node joins the aggregate of a strong neighbour, (3) what is left seeds aggregates with its free neighbours;
* tentative prolongator T from the constant vector, columns normalised;
* prolongator smoothing P = (I - 4 / (3 lmax) D^-1 A) T, lmax an upper bound of the spectrum of D^-1 A;
* Galerkin coarse operator A_c = P^T A P (symmetrised to round-off), until at most ``max_coarse`` rows remain;
* the coarsest matrix is inverted densely (explicit symmetric inverse: one small product on the device).

The smoother of every level but the coarsest is a Chebyshev polynomial of degree ``degree`` in D^-1 A on the interval
[lmax / ``cheb_ratio``, lmax]: the same polynomial before and after the coarse correction, so the V-cycle is a
symmetric operator and a valid CG preconditioner.
"""
import numpy as np
import scipy.sparse as sp


class AMGLevel:
    """One level: its matrix ``A`` (CSR), the inverse diagonal, the Chebyshev interval ``(lmin, lmax)`` of D^-1 A, and --
    for all but the coarsest level -- the prolongator ``P`` to it from the next coarser level and ``R = P^T``."""

    def __init__(self, A, lmin, lmax, P=None, R=None):
        self.A = A
        self.inv_diag = 1.0 / A.diagonal()
        self.lmin, self.lmax = float(lmin), float(lmax)
        self.P, self.R = P, R


def validate_spd_candidate(A):
    """scipy CSR of A, or ValueError when A cannot be an SPD matrix of this solver: not square, not symmetric to
    round-off, a diagonal entry <= 0, a non-finite entry."""
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    A = sp.csr_matrix(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("AMG: matrix must be square, got shape %s" % (A.shape,))
    A.sum_duplicates()
    A.sort_indices()
    if not np.all(np.isfinite(A.data)):
        raise ValueError("AMG: matrix has non-finite entries")
    d = A.diagonal()
    if not np.all(d > 0):
        raise ValueError("AMG: diagonal entry %d is %r, not positive" % (int(np.argmin(d > 0)), float(d[np.argmin(d > 0)])))
    asym = abs(A - A.T)
    scale = abs(A).max() if A.nnz else 1.0
    if asym.nnz and asym.max() > 1e-12 * scale:
        raise ValueError("AMG: matrix is not symmetric (max |A - A^T| = %.3e, max |A| = %.3e)" % (asym.max(), scale))
    return A


def strength(A, theta):
    """Symmetric strength-of-connection graph (CSR pattern, no diagonal)."""
    C = A.tocoo()
    d = np.abs(A.diagonal())
    keep = (C.row != C.col) & (np.abs(C.data) >= theta * np.sqrt(d[C.row] * d[C.col]))
    S = sp.csr_matrix((np.ones(int(keep.sum())), (C.row[keep], C.col[keep])), shape=A.shape)
    S.sort_indices()
    return S


def aggregate(S):
    """Greedy (standard) aggregation of the graph S: an aggregate number per node.  Pass 1 runs over the nodes in
    order; passes 2 and 3 are vectorised over the nodes left free."""
    n = S.shape[0]
    indptr, indices = S.indptr, S.indices
    agg = np.full(n, -1, dtype=np.int64)
    nagg = 0
    ip = indptr.tolist()
    ix = indices.tolist()
    a = agg.tolist()
    for i in range(n):                          # pass 1: seeds whose whole strong neighbourhood is free
        if a[i] >= 0:
            continue
        b, e = ip[i], ip[i + 1]
        if b == e:
            continue                            # isolated node: pass 3
        nb = ix[b:e]
        if all(a[j] < 0 for j in nb):
            a[i] = nagg
            for j in nb:
                a[j] = nagg
            nagg += 1
    agg = np.asarray(a, dtype=np.int64)
    # pass 2: a free node joins the aggregate of its first aggregated strong neighbour
    free = np.flatnonzero(agg < 0)
    if len(free):
        rows = np.repeat(free, np.diff(indptr)[free])
        cols = np.concatenate([indices[indptr[i]:indptr[i + 1]] for i in free]) if len(rows) else np.zeros(0, np.int64)
        tgt = agg[cols] if len(cols) else np.zeros(0, np.int64)
        ok = tgt >= 0
        rows, tgt = rows[ok], tgt[ok]
        first = np.unique(rows, return_index=True)
        agg[first[0]] = tgt[first[1]]
    # pass 3: what is still free seeds new aggregates with its free neighbours
    for i in np.flatnonzero(agg < 0).tolist():
        if agg[i] >= 0:
            continue
        agg[i] = nagg
        nb = indices[indptr[i]:indptr[i + 1]]
        nb = nb[agg[nb] < 0]
        agg[nb] = nagg
        nagg += 1
    return agg, nagg


def tentative_prolongator(agg, nagg):
    """T with T[i, agg[i]] = 1 / sqrt(|aggregate|): the constant vector, column-normalised."""
    n = len(agg)
    counts = np.bincount(agg, minlength=nagg).astype(np.float64)
    return sp.csr_matrix((1.0 / np.sqrt(counts[agg]), (np.arange(n), agg)), shape=(n, nagg))


def spectral_bound(A, inv_diag, steps=20, seed=0):
    """Upper bound of the spectrum of D^-1 A: 1.1 x a power-iteration estimate on D^-1/2 A D^-1/2, capped by
    Gershgorin's bound max_i sum_j |a_ij| / a_ii (a true bound)."""
    n = A.shape[0]
    gersh = float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() * inv_diag))
    s = np.sqrt(inv_diag)
    x = np.random.default_rng(seed).standard_normal(n)
    lam = 0.0
    for _ in range(steps):
        x /= np.linalg.norm(x)
        y = s * (A @ (s * x))
        lam = float(x @ y)
        x = y
    return min(1.1 * abs(lam), gersh) if lam != 0.0 else gersh


class AMGHierarchy:
    """Smoothed-aggregation hierarchy of an SPD matrix (see the module docstring).  ``levels[0].A`` is the input;
    ``coarse_inv`` is the dense symmetric inverse of ``levels[-1].A``."""

    def __init__(self, A, theta=0.08, max_coarse=500, max_levels=12, degree=2, cheb_ratio=4.0, power_steps=20):
        if degree < 1:
            raise ValueError("AMG: Chebyshev degree must be >= 1")
        A = validate_spd_candidate(A)
        self.theta, self.max_coarse, self.degree, self.cheb_ratio = float(theta), int(max_coarse), int(degree), float(cheb_ratio)
        self.levels = []
        while A.shape[0] > self.max_coarse and len(self.levels) + 1 < max_levels:
            inv_diag = 1.0 / A.diagonal()
            lmax = spectral_bound(A, inv_diag, steps=power_steps)
            agg, nagg = aggregate(strength(A, self.theta))
            if nagg >= A.shape[0] or nagg == 0:
                break                                   # no coarsening possible: this is the coarsest level
            T = tentative_prolongator(agg, nagg)
            P = (T - sp.diags((4.0 / (3.0 * lmax)) * inv_diag) @ (A @ T)).tocsr()
            P.eliminate_zeros()
            P.sort_indices()
            R = P.T.tocsr()
            R.sort_indices()
            Ac = (R @ A @ P).tocsr()
            Ac = ((Ac + Ac.T) * 0.5).tocsr()
            Ac.sum_duplicates()
            Ac.sort_indices()
            self.levels.append(AMGLevel(A, lmax / self.cheb_ratio, lmax, P, R))
            A = Ac
        self.levels.append(AMGLevel(A, 0.0, 0.0))
        Ad = A.toarray()
        inv = np.linalg.inv(Ad)
        self.coarse_inv = np.ascontiguousarray(0.5 * (inv + inv.T))

    # ---- inspection -------------------------------------------------------------------------------------------------
    def sizes(self):
        return [lv.A.shape[0] for lv in self.levels]

    def nnz(self):
        return [int(lv.A.nnz) for lv in self.levels]

    def operator_complexity(self):
        """sum of nnz(A_l) over nnz(A_0)."""
        z = self.nnz()
        return float(sum(z)) / z[0]

    def info(self):
        return {"levels": len(self.levels), "rows": self.sizes(), "nnz": self.nnz(),
                "operator_complexity": self.operator_complexity(),
                "prolongator_nnz": [int(lv.P.nnz) for lv in self.levels[:-1]],
                "chebyshev": [(lv.lmin, lv.lmax) for lv in self.levels[:-1]], "degree": self.degree}
