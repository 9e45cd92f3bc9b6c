"""Plain-numpy twin of the general fp64 MFMA product (hippyflow_amd/csrc/hfmi_dgemm.hip, descriptor ``gemm_desc`` and route
``dgemm_route_make`` of hfmi_dgemm.h).  No library is imported here.

(a) ``route``: which kernel a descriptor runs, its load path and grid, or the refusal -- the rule of dgemm_route_make restated.
(b) ``reference``: the values a descriptor must leave in the WHOLE C allocation and the mask of the doubles it writes; everything
    outside the mask (pad rows of ldc, gaps between batch members, guards, skipped tiles) must come back bit for bit.
(c) ``exact_amplitude``: integer operands for which every summation order is exact, so that the comparison is equality.
The case lists of tests/test_gpu_dgemm_descriptor.py stand here as well, so that tests/test_dgemm_route_cpu.py can show on a machine
without a GPU that they reach every kernel instance."""
import numpy as np

NONE, K64, K64_CUT, P128, P64 = -1, 0, 1, 2, 3            # HFMI_DGEMM_* of include/hfmi.h
ERR_NONE, ERR_K2_BATCH, ERR_CUT = 0, 1, 2                 # HFMI_DGEMM_ERR_*
KERNEL_NAMES = {NONE: "none", K64: "k_dgemm", K64_CUT: "k_dgemm<CUT>", P128: "k_dgemm_p<128>", P64: "k_dgemm_p<64>"}
SKIP_NONE, SKIP_DOWN, SKIP_UP = 0, 1, 2
SENTINEL = np.array([0x7FF8C0DEFACE0001], dtype=np.uint64).view(np.float64)[0]     # a NaN with a payload: compared as bits
C0_AMP = 1 << 19                                          # |C0| <= 2^19 where beta != 0


def cdiv(a, b):
    return -(-a // b)


def even_up(v):
    return v + (v & 1)


# ------------------------------------------------------------------ descriptors
def make(name, M, N, K, ta=0, tb=0, K2=0, batch=1, alpha=1.0, beta=0.0, lda=None, ldb=None, ldc=None, lda_odd=0, ldb_odd=0, sA_odd=0,
         sB_odd=0, sC_gap=7, off_A=0, off_B=0, off_A2=0, off_B2=0, off_C=6, lower=0, cut=0, skip=SKIP_NONE, poison=0, lower_sym=0):
    """a descriptor as a dict: natural leading dimensions rounded up to even (so that vec = 1 unless a case asks otherwise),
    ldc = M + 3, batch strides with a gap behind every member, a guard of off_C doubles before C"""
    Km = max(K, K2, 1)
    ra, ca = (Km, M) if ta else (M, Km)               # A and A2 share lda and sA, B and B2 share ldb and sB
    rb, cb = (N, Km) if tb else (Km, N)
    d = dict(name=name, ta=int(ta), tb=int(tb), M=M, N=N, K=K, K2=K2, batch=batch, alpha=float(alpha), beta=float(beta), lower=lower, cut=cut,
             skip=skip, off_A=off_A, off_B=off_B, off_A2=off_A2, off_B2=off_B2, off_C=off_C, poison=poison, lower_sym=lower_sym)
    d["lda"] = (even_up(max(ra, 1)) if lda is None else lda) + lda_odd
    d["ldb"] = (even_up(max(rb, 1)) if ldb is None else ldb) + ldb_odd
    d["ldc"] = M + 3 if ldc is None else ldc
    d["sA"] = even_up(d["lda"] * max(ca, 1)) + 2 + sA_odd if batch > 1 else 0
    d["sB"] = even_up(d["ldb"] * max(cb, 1)) + 2 + sB_odd if batch > 1 else 0
    d["sC"] = d["ldc"] * N + sC_gap if batch > 1 else 0
    return d


def operand_shape(d, which):
    """(rows, columns, leading dimension, batch stride, offset) of A, B, A2, B2 or C as stored (column-major)"""
    k = d["K2"] if which in ("A2", "B2") else d["K"]
    if which in ("A", "A2"):
        r, c = (k, d["M"]) if d["ta"] else (d["M"], k)
        return r, c, d["lda"], d["sA"], d["off_" + which]
    if which in ("B", "B2"):
        r, c = (d["N"], k) if d["tb"] else (k, d["N"])
        return r, c, d["ldb"], d["sB"], d["off_" + which]
    return d["M"], d["N"], d["ldc"], d["sC"], d["off_C"]


def alloc_size(d, which, tail=5):
    """doubles of the allocation of an operand: everything up to its last element, and `tail` guard doubles behind"""
    r, c, ld, s, off = operand_shape(d, which)
    last = off + (d["batch"] - 1) * s + (max(c, 1) - 1) * ld + max(r, 1)
    return last + tail


def view(alloc, d, which, b=0):
    """the (rows x columns) matrix of batch member b inside a flat allocation, as a writable strided view"""
    r, c, ld, s, off = operand_shape(d, which)
    start = off + b * s
    if r == 0 or c == 0:
        return np.zeros((r, c), dtype=alloc.dtype)
    assert start + (c - 1) * ld + r <= alloc.size
    return np.lib.stride_tricks.as_strided(alloc[start:], shape=(r, c), strides=(alloc.itemsize, ld * alloc.itemsize))


def op(mat, trans):
    return mat.T if trans else mat


# ------------------------------------------------------------------ (a) the route
def route(d, pipelined=1):
    """dgemm_route_make restated.  The pipelined kernel runs iff no cut and no skip flag, the switch is on, t128 >= 192 or
    t64 >= 192 (tiles counted with batch), and K + K2 >= 32; BM = 128 iff t128 >= 192.  vec (pipelined kernels only): every
    leading dimension and batch stride even, A and B 16-byte aligned, and A2 and B2 as well when there is a second product."""
    r = dict(kernel=NONE, vec=0, gx=0, gy=0, gz=0, error=ERR_NONE)
    M, N, K, K2, batch = d["M"], d["N"], d["K"], d.get("K2", 0), d.get("batch", 1)
    if M <= 0 or N <= 0:
        return r
    if K2 > 0 and batch > 1:
        return dict(r, error=ERR_K2_BATCH)
    cut = d.get("cut", 0) != 0 or bool(d.get("has_skip", d.get("skip", 0) != 0))
    if cut and (K2 > 0 or d["ta"]):
        return dict(r, error=ERR_CUT)
    t128 = cdiv(M, 128) * cdiv(N, 128) * batch
    t64 = cdiv(M, 64) * cdiv(N, 128) * batch
    if not cut and pipelined and (t128 >= 192 or t64 >= 192) and K + K2 >= 32:
        al = lambda x: d.get("align_" + x, 8 * (d.get("off_" + x, 0) & 1)) % 16 == 0
        even = all(d.get(key, 0) % 2 == 0 for key in ("lda", "ldb", "sA", "sB"))
        vec = int(even and al("A") and al("B") and (K2 == 0 or (al("A2") and al("B2"))))
        bm = 128 if t128 >= 192 else 64
        return dict(r, kernel=P128 if bm == 128 else P64, vec=vec, gx=cdiv(M, bm), gy=cdiv(N, 128), gz=batch)
    return dict(r, kernel=K64_CUT if cut else K64, gx=cdiv(M, 64), gy=cdiv(N, 64), gz=batch)


def instance(d, pipelined=1):
    """(kernel, ta, tb, vec) of the compiled instance and load path a descriptor reaches; None for a refusal or a no-op"""
    r = route(d, pipelined)
    return None if r["kernel"] == NONE else (r["kernel"], d["ta"], d["tb"], r["vec"])


# ------------------------------------------------------------------ (b) values and what is not written
def written_tiles(d, r):
    """mask (M x N) of the entries of one batch member that the kernel of route r writes.
    lower (pipelined kernels only; the 64 x 64 kernel does not look at it): a BM x 128 tile is skipped iff the 128-block of its last
    row is less than the 128-block of its first column, `lower - 1` added to both indices.
    cut bit 0 (64 x 64 tiles bx, by): tiles with by > bx are left untouched."""
    M, N = d["M"], d["N"]
    mask = np.ones((M, N), dtype=bool)
    if r["kernel"] in (P128, P64) and d["lower"]:
        bm, sh = (128 if r["kernel"] == P128 else 64), d["lower"] - 1
        for bx in range(cdiv(M, bm)):
            for by in range(cdiv(N, 128)):
                if (bx * bm + bm - 1 + sh) // 128 < (by * 128 + sh) // 128:
                    mask[bx * bm:(bx + 1) * bm, by * 128:(by + 1) * 128] = False
    if r["kernel"] == K64_CUT and d["cut"] & 1:
        for bx in range(cdiv(M, 64)):
            for by in range(bx + 1, cdiv(N, 64)):
                mask[bx * 64:(bx + 1) * 64, by * 64:(by + 1) * 64] = False
    return mask


def cut_range(d, bx, by):
    """reduction range [klo, khi) of the 64 x 64 tile (bx, by): bit 1 ends it at min(K, (bx + 1) 64), bit 2 starts it at min(K, by 64)"""
    K = d["K"]
    klo = min(K, by * 64) if d["cut"] & 4 else 0
    khi = min(K, (bx + 1) * 64) if d["cut"] & 2 else K
    return klo, khi


def product(d, r, A, B, A2, B2, b, dtype=np.float64):
    """op(A) op(B) + op(A2) op(B2) of batch member b in `dtype`, tile by tile with the ranges of the cuts on the CUT kernel (the
    operand entries outside a tile's range are never touched: they may be NaN)"""
    M, N = d["M"], d["N"]
    # (row-major op(A) against column-major op(B): numpy's long-double product, which has no BLAS behind it, is four times faster so)
    mat = lambda X, which, trans, order: np.asarray(op(view(X, d, which, b), trans), dtype=dtype, order=order)
    oa, ob = mat(A, "A", d["ta"], "C"), mat(B, "B", d["tb"], "F")
    if r["kernel"] == K64_CUT and d["cut"] & 6:
        P = np.zeros((M, N), dtype=dtype)
        for bx in range(cdiv(M, 64)):
            for by in range(cdiv(N, 64)):
                klo, khi = cut_range(d, bx, by)
                if khi > klo:            # an empty range still writes alpha 0 + beta C
                    P[bx * 64:(bx + 1) * 64, by * 64:(by + 1) * 64] = oa[bx * 64:(bx + 1) * 64, klo:khi] @ ob[klo:khi, by * 64:(by + 1) * 64]
        return P
    P = oa @ ob if d["K"] > 0 else np.zeros((M, N), dtype=dtype)
    if d["K2"] > 0:
        P = P + mat(A2, "A2", d["ta"], "C") @ mat(B2, "B2", d["tb"], "F")
    return P


def reference(d, r, A, B, A2, B2, C0, dtype=np.float64):
    """(expected C allocation, mask of the doubles written) for the flat allocations A, B, A2, B2, C0 and the route r.  A refusal, a
    no-op and a raised skip flag write nothing.  beta == 0 does not read C (C0 may be NaN there)."""
    expect = np.array(C0, dtype=dtype)
    written = np.zeros(C0.shape, dtype=bool)
    if r["kernel"] == NONE or d["skip"] == SKIP_UP:
        return expect, written
    mask = written_tiles(d, r)
    for b in range(d["batch"]):
        P = product(d, r, A, B, A2, B2, b, dtype)
        val = dtype(d["alpha"]) * P
        if d["beta"] != 0.0:
            val = val + dtype(d["beta"]) * view(C0, d, "C", b).astype(dtype)
        Cv, Wv = view(expect, d, "C", b), view(written, d, "C", b)
        Cv[mask] = val[mask]
        Wv[mask] = True
    return expect, written


# ------------------------------------------------------------------ (c) exact amplitude
def is_pow2_or_zero(x):
    x = abs(float(x))
    return x == 0.0 or np.frexp(x)[0] == 0.5


def exact_amplitude(d, cmax=C0_AMP, cap=1 << 20):
    """largest power of two a <= cap with (K + K2) a^2 |alpha| + |beta| max|C0| < 2^53 u, u = the smallest of 1, |alpha|, |beta| (the
    nonzero ones): with integer operands in [-a, a], integer C0 and alpha, beta = +-powers of two or 0, every partial sum in any
    order, alpha acc and beta C0 are multiples of u below 2^53 u -- all exactly representable, so every summation order and every
    fused or unfused evaluation gives the same bits and the float64 BLAS product of the integer arrays is the reference."""
    alpha, beta = abs(d["alpha"]), abs(d["beta"])
    assert is_pow2_or_zero(alpha) and is_pow2_or_zero(beta)
    u = min([1.0] + [x for x in (alpha, beta) if x != 0.0])
    kk = max(d["K"] + d["K2"], 1)
    a = cap
    while a > 1 and kk * a * a * max(alpha, 1.0) + beta * cmax >= 2.0 ** 53 * u:
        a //= 2
    assert kk * a * a * max(alpha, 1.0) + beta * cmax < 2.0 ** 53 * u
    return a


def rounding_bound(d, r, A, B, A2, B2, C0):
    """(K + K2 + 2) 2^-53 (|alpha| (|op A||op B| + |op A2||op B2|) + |beta C0|) per entry of batch member 0: it holds for any
    summation order of correctly rounded or fused operations.  The products of the absolute values are float64 BLAS ones -- sums of
    positive terms, relative error below (K + K2 + 2) 2^-53 < 1e-13 -- and the result is scaled by 1 - 1e-12, so that what is
    returned is never above the bound itself."""
    P = product(d, r, np.abs(A), np.abs(B), None if A2 is None else np.abs(A2), None if B2 is None else np.abs(B2), 0)
    mag = abs(d["alpha"]) * P + abs(d["beta"]) * np.abs(view(C0, d, "C", 0))
    return (1.0 - 1e-12) * (d["K"] + d["K2"] + 2) * 2.0 ** -53 * mag


# ------------------------------------------------------------------ the case lists of tests/test_gpu_dgemm_descriptor.py
TT = [(0, 0), (1, 0), (0, 1), (1, 1)]
AB = [(1.0, 0.0), (-1.0, 1.0), (2.0, -0.5)]
KK = [(32, 0), (33, 0), (47, 0), (15, 17), (16, 16), (40, 23)]
UNALIGNED = [("odd-lda", dict(lda_odd=1)), ("odd-ldb", dict(ldb_odd=1)), ("A+1", dict(off_A=1)), ("B2+1", dict(off_B2=1))]
P128_SHAPE = (130, 12161)          # 2 x 96 tiles of 128 x 128, ragged in both directions
P64_SHAPE = (193, 6021)            # t128 = 96, t64 = 192


def tt_name(ta, tb):
    return "%s%s" % ("t" if ta else "n", "t" if tb else "n")


def p128_cases(ta, tb):
    """every (K, K2) and every (alpha, beta) with this (ta, tb), then each of the four ways to lose 16-byte alignment"""
    t = TT.index((ta, tb))
    M, N = P128_SHAPE
    out = []
    for i, (K, K2) in enumerate(KK):
        a, b = AB[(i + t) % 3]
        out.append(make("p128-%s-K%d+%d-a%g-b%g" % (tt_name(ta, tb), K, K2, a, b), M, N, K, ta, tb, K2=K2, alpha=a, beta=b))
    for i, (what, kw) in enumerate(UNALIGNED):
        a, b = AB[(i + t) % 3]
        out.append(make("p128-%s-%s" % (tt_name(ta, tb), what), M, N, 40, ta, tb, K2=23, alpha=a, beta=b, **kw))
    return out


def p64_cases(ta, tb):
    """the same axes, thinned: three (K, K2) per (ta, tb) (all six over two neighbours), every (alpha, beta), one unaligned form"""
    t = TT.index((ta, tb))
    M, N = P64_SHAPE
    out = []
    for j, pick in enumerate([(0, 3, 5), (1, 4, 2), (2, 5, 3), (0, 4, 1)][t]):      # one and two products with every (ta, tb)
        K, K2 = KK[pick]
        a, b = AB[(j + t) % 3]
        out.append(make("p64-%s-K%d+%d-a%g-b%g" % (tt_name(ta, tb), K, K2, a, b), M, N, K, ta, tb, K2=K2, alpha=a, beta=b))
    what, kw = UNALIGNED[t]
    out.append(make("p64-%s-%s" % (tt_name(ta, tb), what), M, N, 40, ta, tb, K2=23, alpha=2.0, beta=-0.5, **kw))
    return out


def batch_cases():
    mk = lambda name, batch, **kw: make("batch%d-%s" % (batch, name), 250, 250, 40, batch=batch, **kw)
    return [mk("nn", 48), mk("tn-odd-sA", 48, ta=1, sA_odd=1), mk("nt-beta", 48, tb=1, alpha=-1.0, beta=1.0),
            mk("tt-odd-sB-beta", 48, ta=1, tb=1, sB_odd=1, alpha=2.0, beta=-0.5),
            mk("nn", 3), mk("tn-beta", 3, ta=1, alpha=2.0, beta=-0.5), mk("nt-odd-sA", 3, tb=1, sA_odd=1), mk("tt-beta", 3, ta=1, tb=1, alpha=-1.0, beta=1.0)]


def batch_refusals():
    return [make("batch3-K2", 250, 250, 40, K2=5, batch=3, beta=1.0), make("batch48-K2", 250, 250, 40, K2=8, batch=48)]


LOWER_VALUES = (0, 1, 2, 65, 128)
LOWER_SHAPES = (1700, 1600)        # BM = 128 (14 x 14 = 196 tiles) and BM = 64 (13 x 13 = 169, 25 x 13 = 325)


def lower_case(n, lower):
    """the eigensolver's rank-2k trailing update C -= V W^T + W V^T (A = V, B = W, A2 = W, B2 = V) on a symmetric integer C"""
    return make("lower%d-n%d" % (lower, n), n, n, 32, 0, 1, K2=32, alpha=-1.0, beta=1.0, lower=lower, lower_sym=1)


K64_SHAPES = [(64, 64), (65, 63), (1, 130), (130, 1), (200, 136)]
K64_KS = [0, 1, 3, 4, 5, 16, 17, 33]


def k64_cases(ta, tb):
    t = TT.index((ta, tb))
    out = []
    for s, (M, N) in enumerate(K64_SHAPES):
        for i, K in enumerate(K64_KS):
            a, b = AB[(i + t + s) % 3]
            K2 = 5 if (i + s) % 3 == 0 else 0
            out.append(make("k64-%s-%dx%d-K%d+%d-a%g-b%g" % (tt_name(ta, tb), M, N, K, K2, a, b), M, N, K, ta, tb, K2=K2, alpha=a, beta=b))
    # K = K2 = 0: beta C (and alpha 0 = 0 with beta = 0)
    out.append(make("k64-%s-empty-beta" % tt_name(ta, tb), 65, 63, 0, ta, tb, alpha=2.0, beta=-0.5))
    out.append(make("k64-%s-empty" % tt_name(ta, tb), 65, 63, 0, ta, tb, alpha=1.0, beta=0.0))
    return out


CUT_VALUES = (0, 1, 2, 4, 3, 7)    # 0: with a skip pointer whose flag is down
CUT_SIZES = (64, 130, 200)


def cut_cases(cut, poison=0):
    out, i = [], 0
    for M in CUT_SIZES:
        for N in CUT_SIZES:
            for K in CUT_SIZES:
                for tb in (0, 1):
                    a, b = AB[i % 3]
                    i += 1
                    out.append(make("cut%d-n%s-%dx%dx%d-a%g-b%g%s" % (cut, "t" if tb else "n", M, N, K, a, b, "-poison" if poison else ""), M, N, K,
                                    0, tb, alpha=a, beta=b, cut=cut, skip=SKIP_NONE if cut else SKIP_DOWN, poison=poison))
    return out


def cw_cases(k=200, poison=0):
    """the products the wide Cholesky issues for a k x k matrix at its first block (cw_gemm of hfmi_chol_wide.hip seen from the
    column-major side: operands and transposition flags traded, one leading dimension, the break flag passed and down)"""
    ld, nb = even_up(k) + (-even_up(k)) % 32, 64
    m = k - nb
    kw = dict(lda=ld, ldb=ld, ldc=ld, skip=SKIP_DOWN, poison=poison)
    out = [make("cw-row-panel", m, nb, nb, 0, 1, alpha=1.0, beta=0.0, cut=0, **kw),
           make("cw-trailing-update", m, m, nb, 0, 1, alpha=-1.0, beta=1.0, cut=1, **kw),
           make("cw-backsub-cut", m, nb, m, 0, 0, alpha=1.0, beta=0.0, cut=2, **kw),
           make("cw-backsub", m, nb, nb, 0, 0, alpha=-1.0, beta=0.0, cut=0, **kw),
           make("cw-r-rtot", k, k, k, 0, 0, alpha=1.0, beta=0.0, cut=7, **kw)]
    return [dict(c, name=c["name"] + "-poison") for c in out if c["cut"] & 6] if poison else out


def skip_up_cases():
    """a raised flag: nothing is written, on a small shape and on one that would run the pipelined kernel without the flag"""
    return [make("skip-up-small", 130, 130, 64, 0, 1, alpha=-1.0, beta=1.0, cut=1, skip=SKIP_UP),
            make("skip-up-large", 1700, 1700, 32, 0, 0, alpha=1.0, beta=0.0, cut=0, skip=SKIP_UP)]


def cut_refusals():
    return [make("cut-ta", 130, 130, 64, 1, 0, cut=2, beta=1.0), make("cut-K2", 130, 130, 64, 0, 1, K2=5, cut=1),
            make("skip-ta", 130, 130, 64, 1, 1, skip=SKIP_DOWN), make("skip-K2", 130, 130, 64, 0, 0, K2=5, skip=SKIP_UP)]


def gemm0_cases():
    """HFMI_EIG_GEMM=0 (a child process): one case each of the 128-tile list, the batch list and the lower list on the 64 x 64 kernel"""
    return [p128_cases(1, 0)[5], batch_cases()[2], lower_case(1600, 65)]


def rounding_cases():
    """one Gaussian case per kernel"""
    return [make("round-k64", 200, 136, 333, 1, 0, K2=77, alpha=-0.7, beta=1.3),
            make("round-p128", P128_SHAPE[0], P128_SHAPE[1], 200, 0, 1, K2=56, alpha=-0.7, beta=1.3),
            make("round-p64", P64_SHAPE[0], P64_SHAPE[1], 200, 1, 1, K2=56, alpha=-0.7, beta=1.3)]


def all_default_cases():
    """every case that runs with the process default of the switch (pipelined = 1)"""
    out = []
    for ta, tb in TT:
        out += p128_cases(ta, tb) + p64_cases(ta, tb) + k64_cases(ta, tb)
    out += batch_cases() + batch_refusals()
    out += [lower_case(n, lo) for n in LOWER_SHAPES for lo in LOWER_VALUES]
    for cut in CUT_VALUES:
        out += cut_cases(cut)
        if cut & 6:
            out += cut_cases(cut, poison=1)
    out += cw_cases() + cw_cases(poison=1) + skip_up_cases() + cut_refusals() + rounding_cases()
    return out


# ------------------------------------------------------------------ operands of a case
def ints(rng, shape, amp):
    return rng.integers(-amp, amp, size=shape, endpoint=True).astype(np.float64)


def fill_operands(d, rng, gaussian=False):
    """flat allocations A, B, A2, B2, C0 of a case.  Operands: integers in [-a, a] (exact_amplitude) or Gaussians inside the matrices,
    NaN in every pad row, gap and guard (nothing there may be read).  poison: NaN also in every element of op(A), op(B) that the cuts
    say is not read -- op(A)[i, k] with k >= (i // 64 + 1) 64 under bit 1, op(B)[k, j] with k < (j // 64) 64 under bit 2.
    C0: the payload-NaN sentinel in pads, gaps and guards; inside the matrices NaN when beta == 0 (C must not be read) and integers of
    at most 2^19 otherwise (symmetric for the lower cases)."""
    amp = 1.0 if gaussian else exact_amplitude(d)
    arrs = {}
    for which in ("A", "B", "A2", "B2"):
        if which in ("A2", "B2") and d["K2"] == 0:
            arrs[which] = None
            continue
        al = np.full(alloc_size(d, which), np.nan)
        for b in range(d["batch"]):
            v = view(al, d, which, b)
            v[...] = rng.standard_normal(v.shape) if gaussian else ints(rng, v.shape, amp)
        arrs[which] = al
    if d["lower_sym"]:       # V W^T + W V^T: the second product is the first with the operands traded (same shapes and strides)
        arrs["A2"], arrs["B2"] = arrs["B"].copy(), arrs["A"].copy()
    if d["poison"]:
        oa, ob = op(view(arrs["A"], d, "A"), d["ta"]), op(view(arrs["B"], d, "B"), d["tb"])
        if d["cut"] & 2:
            for i in range(d["M"]):
                oa[i, (i // 64 + 1) * 64:] = np.nan
        if d["cut"] & 4:
            for j in range(d["N"]):
                ob[:(j // 64) * 64, j] = np.nan
    C0 = np.full(alloc_size(d, "C", tail=9), SENTINEL)
    for b in range(d["batch"]):
        v = view(C0, d, "C", b)
        if d["beta"] == 0.0:
            v[...] = np.nan
        elif gaussian:
            v[...] = rng.standard_normal(v.shape)
        else:
            v[...] = ints(rng, v.shape, C0_AMP)
            if d["lower_sym"]:
                v[...] = np.tril(v) + np.tril(v, -1).T
    return arrs["A"], arrs["B"], arrs["A2"], arrs["B2"], C0
