"""The launch plan of the box Whittle-Matern operators (hfmi_op_box), restated in Python from the rules in the head comment of
hippyflow_amd/csrc/hfmi_boxcov_plan.h; tests/test_box_prior_cpu.py compares it word for word with ``hfmi_boxcov_plan_predict``."""
import ctypes as C

import numpy as np

LDS_BYTES = 163840
MAX_LINES = 256
STATIC_LDS = (8 + 4) * MAX_LINES
MAX_THREADS = 512
MAX_PAIRS = 4096
DEFAULT_BUDGET = 512 << 20
ELEMS, STRIDED_ELEMS = 2048, 8192
FWD, MUL, INV, SCATTER, GATHER = 1, 2, 4, 8, 16
NEUMANN, PERIODIC = 0, 1
HEAD_WORDS, PASS_WORDS, PLAN_WORDS = 16, 16, 96
PASS_FIELDS = ("axis", "flags", "L", "mirror", "n", "stride", "span", "nlines", "lpw", "ls", "threads", "lds", "lds_total", "grid_x")


def line_len(n, boundary):
    if boundary == NEUMANN:
        return 2 * (n - 1) if n > 1 else 1
    return n


def make_pass(n, boundary, P, axis, flags):
    L = P[axis]
    stride = int(np.prod(n[:axis], dtype=np.int64))
    N = n[0] * n[1] * n[2]
    nlines = N // n[axis]
    # the workgroup shape: fftcov_pass_shape of hfmi_fftcov_plan.h
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
    return dict(axis=axis, flags=flags, L=L, mirror=int(boundary[axis] == NEUMANN and n[axis] > 1), n=n[axis], stride=stride,
                span=stride * n[axis], nlines=nlines, lpw=lpw, ls=ls, threads=threads, lds=lds, lds_total=lds + STATIC_LDS,
                grid_x=(nlines + lpw - 1) // lpw)


def plan(shape, boundary, nvec, budget=0, forced=0):
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    bd = list(boundary) + [NEUMANN] * (3 - d)
    P = [line_len(v, b) for v, b in zip(n, bd)]
    N = n[0] * n[1] * n[2]
    passes = []
    for a in range(d - 1):
        passes.append(make_pass(n, bd, P, a, FWD | (SCATTER if a == 0 else 0)))
    passes.append(make_pass(n, bd, P, d - 1, FWD | MUL | INV | ((SCATTER | GATHER) if d == 1 else 0)))
    for a in range(d - 2, -1, -1):
        passes.append(make_pass(n, bd, P, a, INV | (GATHER if a == 0 else 0)))
    pairs = (nvec + 1) // 2
    if budget <= 0:
        budget = DEFAULT_BUDGET
    chunk = forced if forced > 0 else budget // (16 * N)
    chunk = max(1, min(chunk, MAX_PAIRS, pairs))
    return dict(d=d, n=n, P=P, N=N, pairs=pairs, chunk_pairs=chunk, nchunks=(pairs + chunk - 1) // chunk if pairs else 0,
                pair_bytes=16 * N, twiddles=max(max(P) // 4, 1), Pmax=max(P), passes=passes)


def plan_words(p):
    w = [0] * PLAN_WORDS
    w[:16] = [p["d"], p["n"][0], p["n"][1], p["n"][2], p["N"], p["pairs"], p["chunk_pairs"], p["nchunks"], len(p["passes"]),
              p["pair_bytes"], p["twiddles"], p["Pmax"], STATIC_LDS, p["P"][0], p["P"][1], p["P"][2]]
    for i, q in enumerate(p["passes"]):
        w[HEAD_WORDS + i * PASS_WORDS:HEAD_WORDS + i * PASS_WORDS + len(PASS_FIELDS)] = [q[f] for f in PASS_FIELDS]
    return w


def predict(L, shape, boundary, nvec, budget=0):
    """the library's words for the same call"""
    words = (C.c_int64 * PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    b = (C.c_int * len(shape))(*boundary)
    L.call("hfmi_boxcov_plan_predict", len(shape), C.cast(n, C.c_void_p), C.cast(b, C.c_void_p), int(nvec), int(budget), words)
    return list(words)


def line_bases(q):
    """first entry of every line of a pass, by the line map the kernel uses"""
    line = np.arange(q["nlines"], dtype=np.int64)
    return line % q["stride"] + (line // q["stride"]) * q["span"]
