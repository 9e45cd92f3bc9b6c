"""The launch plan of the FFT apply of a kernel covariance on a grid, restated in Python from the rules in the head comment of
hippyflow_amd/csrc/hfmi_fftcov_plan.h; tests/test_fftcov_plan_cpu.py compares it word for word with ``hfmi_fftcov_plan_predict``."""
import ctypes as C

import numpy as np

LDS_BYTES = 163840
MAX_LINES = 256
STATIC_LDS = 2 * 8 * MAX_LINES
MAX_THREADS = 512
MAX_PAIRS = 4096
DEFAULT_BUDGET = 512 << 20
ELEMS, STRIDED_ELEMS = 2048, 8192
FWD, MUL, INV, SCATTER, GATHER = 1, 2, 4, 8, 16
HEAD_WORDS, PASS_WORDS, PLAN_WORDS = 16, 16, 96
PASS_FIELDS = ("axis", "flags", "L", "stride", "nlines", "nload", "nstore", "lpw", "ls", "threads", "lds", "lds_total", "grid_x",
               "oe0", "os0", "os1")


def embed_len(n):
    P = 1
    while P < 2 * n - 1:
        P *= 2
    return P


def make_pass(P, axis, flags, ext, nload, nstore):
    L = P[axis]
    stride = int(np.prod(P[:axis], dtype=np.int64))
    e1 = ext[1] if axis < 1 else 1
    e2 = ext[2] if axis < 2 else 1
    nlines = stride * e1 * e2
    if axis == 0:
        oe0, os0, os1 = ext[1], P[0], P[0] * P[1]
    elif axis == 1:
        oe0, os0, os1 = ext[2], P[0] * P[1], 0
    else:
        oe0, os0, os1 = 1, 0, 0
    lpw = max(1, ELEMS // L)
    if stride > 1:
        lpw = max(lpw, min(4, STRIDED_ELEMS // L))
    lpw = min(lpw, MAX_LINES)
    while lpw > 1 and lpw // 2 >= nlines:
        lpw //= 2
    pad = 0 if lpw == 1 else (1 if (lpw >= 16 or L < 16) else 16 // lpw)
    ls = L + pad
    lds = 16 * (lpw * ls + max(L // 4, 1))
    items = lpw * L // 4
    threads = min(MAX_THREADS, max(64, (items + 63) // 64 * 64))
    return dict(axis=axis, flags=flags, L=L, stride=stride, nlines=nlines, nload=nload, nstore=nstore, lpw=lpw, ls=ls, threads=threads,
                lds=lds, lds_total=lds + STATIC_LDS, grid_x=(nlines + lpw - 1) // lpw, oe0=oe0, os0=os0, os1=os1)


def plan(shape, nvec, budget=0, forced=0):
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    P = [embed_len(v) for v in n]
    Ptot = P[0] * P[1] * P[2]
    passes = []
    for a in range(d - 1):
        passes.append(make_pass(P, a, FWD | (SCATTER if a == 0 else 0), n, n[a], P[a]))
    passes.append(make_pass(P, d - 1, FWD | MUL | INV | ((SCATTER | GATHER) if d == 1 else 0), n, n[d - 1], n[d - 1]))
    for a in range(d - 2, -1, -1):
        passes.append(make_pass(P, a, INV | (GATHER if a == 0 else 0), n, P[a], n[a]))
    pairs = (nvec + 1) // 2
    if budget <= 0:
        budget = DEFAULT_BUDGET
    chunk = forced if forced > 0 else budget // (16 * Ptot)
    chunk = max(1, min(chunk, MAX_PAIRS, pairs))
    return dict(d=d, P=P, Ptot=Ptot, pairs=pairs, chunk_pairs=chunk, nchunks=(pairs + chunk - 1) // chunk if pairs else 0,
                pair_bytes=16 * Ptot, twiddles=max(max(P) // 4, 1), Pmax=max(P), passes=passes)


def plan_words(p):
    w = [0] * PLAN_WORDS
    w[:13] = [p["d"], p["P"][0], p["P"][1], p["P"][2], p["Ptot"], p["pairs"], p["chunk_pairs"], p["nchunks"], len(p["passes"]),
              p["pair_bytes"], p["twiddles"], p["Pmax"], STATIC_LDS]
    for i, q in enumerate(p["passes"]):
        w[HEAD_WORDS + i * PASS_WORDS:HEAD_WORDS + (i + 1) * PASS_WORDS] = [q[f] for f in PASS_FIELDS]
    return w


def predict(L, shape, nvec, budget=0):
    """the library's words for the same call"""
    words = (C.c_int64 * PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    L.call("hfmi_fftcov_plan_predict", len(shape), C.cast(n, C.c_void_p), int(nvec), int(budget), words)
    return list(words)


def line_bases(q):
    """first entry of every line of a pass, by the line map the kernel uses"""
    line = np.arange(q["nlines"], dtype=np.int64)
    inner, o = line % q["stride"], line // q["stride"]
    return inner + (o % q["oe0"]) * q["os0"] + (o // q["oe0"]) * q["os1"]


def expected_bases(p, shape, q):
    """the lines a pass along q['axis'] must take: every position of the axes below it, the first n_b positions of the axes above it"""
    P = p["P"]
    n = list(shape) + [1] * (3 - len(shape))
    a = q["axis"]
    rng = [np.arange(P[b]) if b < a else np.arange(1) if b == a else np.arange(n[b]) for b in range(3)]
    i0, i1, i2 = np.meshgrid(*rng, indexing="ij")
    return np.sort((i0 + P[0] * (i1 + P[1] * i2)).ravel())
