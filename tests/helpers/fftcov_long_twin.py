"""The long route of the grid kernel covariance (hfmi_op_kernel_cov_grid_long, hfmi_grid_sampler_create_long), restated in Python from
the section "split-line passes" of hippyflow_amd/csrc/hfmi_fftcov_plan.h:

* ``plan`` / ``plan_words``: the launch plan, compared word for word with ``hfmi_fftcov_long_plan_predict``;
* ``line_entries``: every (line, position) a pass touches, by the line map the split kernel uses, for the coverage checks;
* ``split_fft`` / ``apply``: the split transform in numpy, Bailey's four-step without transposes in the device's storage order, and the
  apply built from it (scatter, forward passes, multiply by Lambda / P, inverse passes, gather);
* ``sampler_growth``: the growth a long-route sampler takes, from the spectrum of tests/helpers/grid_metric_twin.py.

The apply bound is that of tests/test_gpu_grid_kernel_cov.py::test_apply_against_host (``column_bounds`` of fftcov_twin.py):
per column  32 max(1, log2 P) eps sqrt(P) ||c||_2 ||W_j||_2  +  8 N eps || |C| |W_j| ||_2,  P the product of the embedding lengths.
The split adds one complex multiply by a twiddle per entry and per split axis on each side; a twiddle within a few ulps of the truth is
a relative perturbation of O(eps) per entry, i.e. a term O(eps ||c|| ||W||) per split axis and side, which the log2 P factor of the
bound (one per radix-2 stage: log2 P = log2 L1 + log2 L2 stages either way) already covers: the split does not add a stage.  No extra
term is needed, and the numpy twin is held to the formula unchanged (tests/test_fftcov_long_cpu.py)."""
import ctypes as C

import numpy as np

import fftcov_plan_twin as pt

MAX_LINE, MIN_LINE = 4096, 4
LONG_MAXN = 1 << 23
MAX_GROWTH = 6
MAX_PASSES = 11
STATIC_LDS = pt.STATIC_LDS + 4 * pt.MAX_LINES
TW_STORE, TW_LOAD, GEN, LOAD_FULL, STORE_FULL = 256, 512, 32, 64, 128
WHOLE, HI, LO = 0, 1, 2
APPLY, DRAW, FACTOR, FACTOR_T, SPECTRUM = 0, 1, 2, 3, 4
HEAD_WORDS, PASS_WORDS = 16, 24
PLAN_WORDS = HEAD_WORDS + MAX_PASSES * PASS_WORDS
SUB_FIELDS = ("part", "L1", "L2", "inner", "esub", "sub_stride", "pm", "sm")
EPS = np.finfo(np.float64).eps


def max_line_ok(v):
    return MIN_LINE <= v <= MAX_LINE and v & (v - 1) == 0


def embedding(shape, growth=0):
    n = list(shape) + [1] * (3 - len(shape))
    return n, [pt.embed_len(v) << growth if v > 1 else 1 for v in n]


def feasible(shape, growth, max_line):
    if not 0 <= growth <= MAX_GROWTH or not max_line_ok(max_line):
        return False
    n, P = embedding(shape, growth)
    return all(1 <= v <= LONG_MAXN for v in shape) and all(p <= max_line * max_line for p in P)


def split_of(P, max_line):
    """(L1, L2): L2 = max_line, L1 = P / max_line for an axis longer than max_line; (1, P) otherwise"""
    return (P // max_line, max_line) if P > max_line else (1, P)


def _shape_pass(q):
    """fftcov_pass_shape: lines per workgroup, LDS, threads, grid from L, stride, nlines"""
    L, stride, nlines = q["L"], q["stride"], q["nlines"]
    lpw = max(1, pt.ELEMS // L)
    if stride > 1:
        lpw = max(lpw, min(4, pt.STRIDED_ELEMS // L))
    lpw = min(lpw, pt.MAX_LINES)
    while lpw > 1 and lpw // 2 >= nlines:
        lpw //= 2
    pad = 0 if lpw == 1 else (1 if (lpw >= 16 or L < 16) else 16 // lpw)
    ls = L + pad
    lds = 16 * (lpw * ls + max(L // 4, 1))
    threads = min(pt.MAX_THREADS, max(64, (lpw * L // 4 + 63) // 64 * 64))
    q.update(lpw=lpw, ls=ls, threads=threads, lds=lds, grid_x=(nlines + lpw - 1) // lpw)


class _Plan:
    def __init__(self, shape, growth, max_line):
        self.d = len(shape)
        self.n, self.P = embedding(shape, growth)
        self.split = [split_of(p, max_line) for p in self.P]
        self.passes = []

    def add(self, axis, part, flags, ext, nload, nstore):
        P, (L1, L2) = self.P, self.split[axis]
        if part == WHOLE:
            q = pt.make_pass(P, axis, flags, ext, nload, nstore)
            q["lds_total"] = q["lds"] + pt.STATIC_LDS
            q.update(part=WHOLE, L1=L1, L2=L2, inner=q["stride"], esub=1, sub_stride=0, pm=1, sm=0)
        else:
            S = int(np.prod(P[:axis], dtype=np.int64))
            if part == HI:
                L, stride, esub, sub_stride, pm, sm = L1, S * L2, min(L2, ext[axis]), S, L2, 1
            else:
                L, stride, esub, sub_stride, pm, sm = L2, S, L1, S * L2, 1, 0
            e1 = ext[1] if axis < 1 else 1
            e2 = ext[2] if axis < 2 else 1
            if axis == 0:
                oe0, os0, os1 = ext[1], P[0], P[0] * P[1]
            elif axis == 1:
                oe0, os0, os1 = ext[2], P[0] * P[1], 0
            else:
                oe0, os0, os1 = 1, 0, 0
            q = dict(axis=axis, flags=flags, L=L, stride=stride, nlines=S * esub * e1 * e2, nload=nload, nstore=nstore, oe0=oe0, os0=os0,
                     os1=os1)
            _shape_pass(q)
            q["lds_total"] = q["lds"] + STATIC_LDS
            q.update(part=part, L1=L1, L2=L2, inner=S, esub=esub, sub_stride=sub_stride, pm=pm, sm=sm)
        self.passes.append(q)

    def forward(self, a, first_flags, ext, in_len, last):
        L1, L2 = self.split[a]
        if L1 == 1:
            if not last:
                self.add(a, WHOLE, pt.FWD | first_flags, ext, in_len, self.P[a])
            return
        e = list(ext)
        e[a] = in_len
        self.add(a, HI, pt.FWD | TW_STORE | first_flags, e, in_len, self.P[a])
        if not last:
            self.add(a, LO, pt.FWD, ext, min(in_len, L2), L2)

    def inverse(self, a, last_flags, ext, out_len, first):
        L1, L2 = self.split[a]
        if L1 == 1:
            if not first:
                self.add(a, WHOLE, pt.INV | last_flags, ext, self.P[a], out_len)
            return
        if not first:
            self.add(a, LO, pt.INV, ext, L2, min(out_len, L2))
        e = list(ext)
        e[a] = out_len
        self.add(a, HI, pt.INV | TW_LOAD | last_flags, e, self.P[a], out_len)

    def middle(self, flags, extra_whole, ext, in_len, out_len):
        a = self.d - 1
        L1, L2 = self.split[a]
        if L1 == 1:
            self.add(a, WHOLE, flags | extra_whole, ext, in_len, out_len)
        else:
            self.add(a, LO, flags, ext, min(in_len, L2), min(out_len, L2))


def plan(kind, shape, growth=0, max_line=MAX_LINE, nvec=2, budget=0, forced=0):
    """the long route's plan as a dict (head) with a list of passes, each the 16 fields of fftcov_plan_twin plus SUB_FIELDS"""
    p = _Plan(shape, growth, max_line)
    d, n, P = p.d, p.n, p.P
    full, data = list(P), list(n)
    if kind == SPECTRUM:
        for a in range(d):
            p.forward(a, 0, full, full[a], False)
    elif kind == DRAW:
        a = d - 1
        gather = pt.GATHER if d == 1 else 0
        p.middle(GEN | pt.INV, gather, data, full[a], data[a])
        if p.split[a][0] > 1:
            p.inverse(a, gather, data, data[a], True)
        for b in range(d - 2, -1, -1):
            p.inverse(b, pt.GATHER if b == 0 else 0, data, data[b], False)
    else:
        transpose = kind == FACTOR_T
        factor = kind in (FACTOR, FACTOR_T)
        fwd_ext = full if factor and not transpose else data
        inv_ext = full if factor and transpose else data
        load_side = LOAD_FULL if factor and not transpose else 0
        store_side = STORE_FULL if transpose else 0
        in_len = full if factor and not transpose else data
        out_len = full if transpose else data
        for a in range(d):
            p.forward(a, (pt.SCATTER | load_side) if a == 0 else 0, fwd_ext, in_len[a], a == d - 1)
        p.middle(pt.FWD | pt.MUL | pt.INV, (pt.SCATTER | pt.GATHER | load_side | store_side) if d == 1 else 0, data, in_len[d - 1],
                 out_len[d - 1])
        for a in range(d - 1, -1, -1):
            p.inverse(a, (pt.GATHER | store_side) if a == 0 else 0, inv_ext, out_len[a], a == d - 1)
    Ptot = P[0] * P[1] * P[2]
    pairs = (nvec + 1) // 2
    b = budget if budget > 0 else pt.DEFAULT_BUDGET
    chunk = forced if forced > 0 else b // (16 * Ptot)
    chunk = max(1, min(chunk, pt.MAX_PAIRS, pairs))
    lmax = max(L2 for _, L2 in p.split)
    return dict(d=d, P=P, n=n, split=p.split, Ptot=Ptot, pairs=pairs, chunk_pairs=chunk,
                nchunks=(pairs + chunk - 1) // chunk if pairs else 0, pair_bytes=16 * Ptot, twiddles=max(lmax // 4, 1), Pmax=lmax,
                growth=growth, kind=kind, max_line=max_line, passes=p.passes)


def plan_words(p):
    w = [0] * PLAN_WORDS
    w[:HEAD_WORDS] = [p["d"], p["P"][0], p["P"][1], p["P"][2], p["Ptot"], p["pairs"], p["chunk_pairs"], p["nchunks"], len(p["passes"]),
                      p["pair_bytes"], p["twiddles"], p["Pmax"], STATIC_LDS, p["growth"], p["kind"], p["max_line"]]
    for i, q in enumerate(p["passes"]):
        w[HEAD_WORDS + i * PASS_WORDS:HEAD_WORDS + (i + 1) * PASS_WORDS] = [q[f] for f in pt.PASS_FIELDS + SUB_FIELDS]
    return w


def predict(L, kind, shape, growth=0, max_line=MAX_LINE, nvec=2, budget=0):
    """the library's words for the same call (raises HfmiError where the library refuses)"""
    words = (C.c_int64 * PLAN_WORDS)()
    n = (C.c_int64 * max(1, len(shape)))(*shape)
    L.call("hfmi_fftcov_long_plan_predict", int(kind), len(shape), C.cast(n, C.c_void_p), int(growth), int(max_line), int(nvec), int(budget),
           words)
    return list(words)


def line_entries(q):
    """(bases, positions): the first entry of every line by the split kernel's line map, and for each line the axis positions of its
    L line positions (p pm + sub sm)"""
    line = np.arange(q["nlines"], dtype=np.int64)
    inner, r = line % q["inner"], line // q["inner"]
    sub, o = r % q["esub"], r // q["esub"]
    if q["part"] == WHOLE:
        sub = np.zeros_like(line)
    base = inner + sub * q["sub_stride"] + (o % q["oe0"]) * q["os0"] + (o // q["oe0"]) * q["os1"]
    pos = np.arange(q["L"], dtype=np.int64)[None, :] * q["pm"] + (sub * q["sm"])[:, None]
    return base, pos


# ------------------------------------------------------------------------------------------------ the split transform in numpy
def bitrev(L):
    """position -> index of an L-point decimation-in-frequency output (L a power of two)"""
    b = max(int(L).bit_length() - 1, 0)
    p = np.arange(L)
    r = np.zeros(L, dtype=np.int64)
    for i in range(b):
        r |= ((p >> i) & 1) << (b - 1 - i)
    return r


def _fft_storage(x, axis, L):
    """an L-point DFT along `axis` whose result sits in digit-reversed storage order (what one in-place DIF pass leaves)"""
    return np.take(np.fft.fft(x, axis=axis), bitrev(L), axis=axis)


def _ifft_storage(x, axis, L):
    """the unnormalised inverse DFT of digit-reversed input along `axis`, natural order out (one DIT pass)"""
    inv = np.argsort(bitrev(L))
    return np.fft.ifft(np.take(x, inv, axis=axis), axis=axis) * L


def split_fft(x, axis, L1, L2, inverse=False):
    """the transform of numpy axis `axis` (length P = L1 L2, natural order in) as the two passes of the long route: the L1-point DFTs of
    the high sub-axis (s = L2 n1 + n2) with the twiddle exp(-2 pi i n2 k1 / P) at their store, then the L2-point DFTs of the low one.
    The result is in the storage order of one P-point pass.  inverse=True: the mirror (digit-reversed in, natural out, unnormalised)."""
    P = L1 * L2
    shp = list(x.shape)
    y = x.reshape(shp[:axis] + [L1, L2] + shp[axis + 1:])
    bshape = [1] * y.ndim
    bshape[axis], bshape[axis + 1] = L1, L2
    k1 = bitrev(L1)[:, None]
    n2 = np.arange(L2)[None, :]
    tw = np.exp(-2j * np.pi * ((n2 * k1) % P) / P).reshape(bshape)
    if not inverse:
        y = _fft_storage(y, axis, L1) * tw
        y = _fft_storage(y, axis + 1, L2)
    else:
        y = _ifft_storage(y, axis + 1, L2) * np.conj(tw)
        y = _ifft_storage(y, axis, L1)
    return y.reshape(shp)


def storage_fftn(x, split):
    """the forward passes over every axis of a numpy array of shape (P2, P1, P0)[-d:] (grid axis c is numpy axis d - 1 - c)"""
    d = x.ndim
    for c in range(d):
        L1, L2 = split[c]
        x = split_fft(x, d - 1 - c, L1, L2)
    return x


def storage_ifftn(x, split):
    d = x.ndim
    for c in range(d - 1, -1, -1):
        L1, L2 = split[c]
        x = split_fft(x, d - 1 - c, L1, L2, inverse=True)
    return x


def storage_permutation(P):
    """index arrays that take numpy.fft.fftn's natural order to the storage order (per numpy axis: bitrev of that axis)"""
    return np.ix_(*[bitrev(p) for p in P[::-1]])


def apply(shape, spacing, family, sigma, ell, nugget, W, nodes=None, G=None, max_line=MAX_LINE):
    """Y = C W by the split passes (column from grid_metric_twin, spectrum by the same forward passes, stored order throughout)"""
    import grid_metric_twin as gm
    shape = tuple(int(v) for v in shape)
    d = len(shape)
    P = [pt.embed_len(v) for v in shape]
    split = [split_of(p, max_line) for p in P]
    col = gm.first_column(shape, spacing, family, sigma, ell, nugget, G).astype(np.complex128)
    lam = storage_fftn(col, split).real / col.size
    N, k = W.shape
    g = np.arange(int(np.prod(shape))) if nodes is None else np.asarray(nodes, dtype=np.int64)
    assert g.size == N
    idx, rest = [], g
    for v in shape:
        idx.append(rest % v)
        rest = rest // v
    idx = tuple(idx[::-1])
    Y = np.empty((N, k))
    for j in range(0, k, 2):
        z = np.zeros(col.shape, dtype=np.complex128)
        z[idx] = W[:, j] + (1j * W[:, j + 1] if j + 1 < k else 0.0)
        y = storage_ifftn(lam * storage_fftn(z, split), split)[idx]
        Y[:, j] = y.real
        if j + 1 < k:
            Y[:, j + 1] = y.imag
    assert d == len(split)
    return Y


# ------------------------------------------------------------------------------------------------ the sampler's growth
FLOOR_C = 16.0


def floor(Ptot, lmax):
    return FLOOR_C * EPS * max(int(Ptot - 1).bit_length() if Ptot > 1 else 0, 1) * lmax


def first_column(shape, spacing, family, sigma, ell, nugget, G=None, growth=0):
    """grid_metric_twin.first_column bit for bit with one kernel evaluation per entry: that one evaluates the kernel over the whole
    padded array for each of the 2^d sign choices and keeps the entries at the half positions of the flipped axes; this one evaluates a
    sign choice with flipped axes only on those half positions (same operations per entry, and x + 0.0 = x).  A quarter of the time in
    two dimensions, which the 8192 x 8192 embeddings of the growth table need."""
    import grid_metric_twin as gm
    d = len(shape)
    P = [(gm.embed_len(n) << growth) if n > 1 else 1 for n in shape]
    Lf = np.eye(d) if G is None else np.linalg.cholesky(np.asarray(G, dtype=np.float64).reshape(d, d))
    view = lambda c: [-1 if a == c else 1 for a in range(d)][::-1]
    total = np.zeros(P[::-1])
    count = np.zeros(P[::-1])
    for b in range(1 << d):
        flipped = [c for c in range(d) if b & (1 << c)]
        if any(P[c] < 2 for c in flipped):
            continue
        u, where = [], [slice(None)] * d
        for c in range(d):
            s = np.arange(P[c]) if c not in flipped else np.array([P[c] // 2])
            o = (np.where(2 * s < P[c], s, s - P[c]) * float(spacing[c])).reshape(view(c))
            u.append(-o if c in flipped else o)
            if c in flipped:
                where[d - 1 - c] = slice(P[c] // 2, P[c] // 2 + 1)
        r2 = 0.0
        for c in range(d):
            w = Lf[c, c] * u[c]
            for e in range(c + 1, d):
                w = w + Lf[e, c] * u[e]
            r2 = r2 + w * w
        where = tuple(where)
        r2 = np.broadcast_to(r2, total[where].shape)
        total[where] = total[where] + gm.phi(family, np.sqrt(r2) / ell)
        count[where] = count[where] + 1.0
    col = sigma ** 2 * (total / count)
    col[(0,) * d] += nugget
    return col


def sampler_growth(shape, spacing, family, sigma, ell, nugget, G=None, max_growth=MAX_GROWTH, max_line=MAX_LINE, long_route=True, trace=None):
    """(growth, P, lambda_min / lambda_max, definite) the sampler takes: the first growth 0 .. max_growth whose spectrum is above minus
    the floor, among the feasible ones (long route: every P_c <= max_line^2; old route: every P_c <= 4096 and growth <= 3).  The
    spectrum is numpy.fft.fftn of the column of grid_metric_twin (first_column above: the same bits).  ``trace``: a list that receives
    (growth, P, lambda_min, lambda_max, definite) of every growth tried."""

    def ok(g):
        if long_route:
            return feasible(shape, g, max_line)
        return g <= 3 and all(p <= 4096 for p in embedding(shape, g)[1])

    g, last = 0, None
    while True:
        if not ok(g):
            return last if last is not None else (None, None, None, False)
        lam = np.fft.fftn(first_column(shape, spacing, family, sigma, ell, nugget, G, growth=g)).real
        lo, hi = lam.min(), lam.max()
        definite = lo >= -floor(lam.size, hi)
        last = (g, embedding(shape, g)[1][:len(shape)], lo / hi, definite)
        if trace is not None:
            trace.append((g, last[1], float(lo), float(hi), bool(definite)))
        del lam
        if definite or g == max_growth:
            return last
        g += 1
