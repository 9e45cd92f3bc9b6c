"""The mixed-radix lines of the box Whittle-Matern operators (k_boxcov_pass_mr), restated in numpy from the head comment of
hippyflow_amd/csrc/hfmi_boxcov_plan.h: the rule of an axis, the order of the factors, the position map, the stages themselves and the
workgroup shape; the plan of a grid with such lines, whose power-of-two passes are those of boxcov_plan_twin.
tests/test_box_sizes_cpu.py compares it word for word with ``hfmi_boxcov_plan_predict`` and the stages with ``numpy.fft.fft``."""
import numpy as np

import boxcov_plan_twin as tw

MAX_LINE = 4096
MAX_NODES = {tw.NEUMANN: 2049, tw.PERIODIC: 4096}
PASS_FIELDS = tw.PASS_FIELDS + ("n3", "n5")


def factor(L):
    """(n3, n5, logQ) of a mixed-radix line L = 3^n3 5^n5 2^logQ, logQ >= 2 and an odd factor present; None otherwise"""
    if L < 4 or L % 4:
        return None
    count = {}
    for r in (3, 5, 2):
        count[r] = 0
        while L % r == 0:
            L //= r
            count[r] += 1
    if L != 1 or count[3] + count[5] == 0:
        return None
    return count[3], count[5], count[2]


def pow2(v):
    return v >= 1 and v & (v - 1) == 0


def axis_ok(n, boundary):
    if boundary not in MAX_NODES or n < 1 or n > MAX_NODES[boundary]:
        return False
    L = tw.line_len(n, boundary)
    return pow2(L) or factor(L) is not None


def legal_lengths():
    """every legal line length of 4 or more, power-of-two ones included"""
    return [L for L in range(4, MAX_LINE + 1) if pow2(L) or factor(L) is not None]


def radices(L):
    """the odd stages of the forward transform in order: all 3s, then all 5s"""
    n3, n5, _ = factor(L)
    return [3] * n3 + [5] * n5


def modes(L):
    """mode[p]: over a block with leading odd factor r, p div sub + r mode_sub(p mod sub); bit reversal on the tail"""
    _, _, logQ = factor(L)

    def rec(p, B, rs):
        if not rs:
            return int(format(p, "0%db" % logQ)[::-1], 2)
        r, sub = rs[0], B // rs[0]
        return p // sub + r * rec(p % sub, sub, rs[1:])

    return np.array([rec(p, L, radices(L)) for p in range(L)])


def staged_forward(x):
    """the forward stages on one line: the odd stages as the head comment states them, then a decimation-in-frequency radix-2 FFT on
    every block of Q entries (its result in bit-reversed order, which is what the radix-4 / radix-2 stages leave)"""
    x = np.array(x, dtype=np.complex128)
    L = x.size
    _, _, logQ = factor(L)
    B = L
    for r in radices(L):
        sub = B // r
        y = np.empty_like(x)
        q = np.arange(sub)
        for b0 in range(0, L, B):
            for t in range(r):
                acc = sum(x[b0 + q + s * sub] * np.exp(-2j * np.pi * s * t / r) for s in range(r))
                y[b0 + t * sub + q] = acc * np.exp(-2j * np.pi * q * t / B)
        x, B = y, sub
    h = B // 2
    while h >= 1:
        v = x.reshape(-1, 2, h)                      # every block of 2 h entries: its halves
        a, b = v[:, 0, :].copy(), v[:, 1, :].copy()
        v[:, 0, :] = a + b
        v[:, 1, :] = (a - b) * np.exp(-2j * np.pi * np.arange(h) / (2 * h))
        h //= 2
    return x


def pow2floor(v):
    f = 1
    while 2 * f <= v:
        f *= 2
    return f


def make_pass(n, boundary, P, axis, flags):
    L = P[axis]
    f = factor(L)
    if f is None:
        q = tw.make_pass(n, boundary, P, axis, flags)
        q.update(n3=0, n5=0)
        return q
    stride = int(np.prod(n[:axis], dtype=np.int64))
    nlines = n[0] * n[1] * n[2] // n[axis]
    lpw = pow2floor(tw.ELEMS // L)
    if stride > 1:
        lpw = max(lpw, min(4, pow2floor(tw.STRIDED_ELEMS // L)))
    lpw = min(lpw, tw.MAX_LINES)
    while lpw > 1 and lpw // 2 >= nlines:
        lpw //= 2
    pad = 0 if lpw == 1 else (1 if (lpw >= 16 or L < 16) else 16 // lpw)
    ls = L + pad
    lds = 16 * (lpw * ls + L // 4)
    threads = min(tw.MAX_THREADS, max(64, (lpw * L // 4 + 63) // 64 * 64))
    return dict(axis=axis, flags=flags, L=L, mirror=int(boundary[axis] == tw.NEUMANN and n[axis] > 1), n=n[axis], stride=stride,
                span=stride * n[axis], nlines=nlines, lpw=lpw, ls=ls, threads=threads, lds=lds, lds_total=lds + tw.STATIC_LDS,
                grid_x=(nlines + lpw - 1) // lpw, n3=f[0], n5=f[1])


def plan(shape, boundary, nvec, budget=0, forced=0):
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    bd = list(boundary) + [tw.NEUMANN] * (3 - d)
    P = [tw.line_len(v, b) for v, b in zip(n, bd)]
    N = n[0] * n[1] * n[2]
    passes = [make_pass(n, bd, P, a, tw.FWD | (tw.SCATTER if a == 0 else 0)) for a in range(d - 1)]
    passes.append(make_pass(n, bd, P, d - 1, tw.FWD | tw.MUL | tw.INV | ((tw.SCATTER | tw.GATHER) if d == 1 else 0)))
    passes += [make_pass(n, bd, P, a, tw.INV | (tw.GATHER if a == 0 else 0)) for a in range(d - 2, -1, -1)]
    pairs = (nvec + 1) // 2
    chunk = forced if forced > 0 else (budget if budget > 0 else tw.DEFAULT_BUDGET) // (16 * N)
    chunk = max(1, min(chunk, tw.MAX_PAIRS, pairs))
    Pmax2 = max([v for v in P if pow2(v)] + [1])          # the power-of-two lines' table; a mixed-radix line has its own L / 4 entries
    return dict(d=d, n=n, P=P, N=N, pairs=pairs, chunk_pairs=chunk, nchunks=(pairs + chunk - 1) // chunk if pairs else 0,
                pair_bytes=16 * N, twiddles=max(Pmax2 // 4, 1), Pmax=Pmax2, passes=passes)


def plan_words(p):
    w = [0] * tw.PLAN_WORDS
    w[:16] = [p["d"], p["n"][0], p["n"][1], p["n"][2], p["N"], p["pairs"], p["chunk_pairs"], p["nchunks"], len(p["passes"]),
              p["pair_bytes"], p["twiddles"], p["Pmax"], tw.STATIC_LDS, p["P"][0], p["P"][1], p["P"][2]]
    for i, q in enumerate(p["passes"]):
        w[tw.HEAD_WORDS + i * tw.PASS_WORDS:tw.HEAD_WORDS + (i + 1) * tw.PASS_WORDS] = [q[f] for f in PASS_FIELDS]
    return w
