"""The launch plan of a draw of the grid sampler (hfmi_grid_sampler_draw), restated in Python from the rules in the comment above
``fftcov_sample_plan_passes`` in hippyflow_amd/csrc/hfmi_fftcov_plan.h; tests/test_grid_sampler_plan_cpu.py compares it word for word
with ``hfmi_fftcov_sample_plan_predict``.  The rule of one pass is the apply's (``fftcov_plan_twin.make_pass``)."""
import ctypes as C

from fftcov_plan_twin import (DEFAULT_BUDGET, GATHER, HEAD_WORDS, INV, MAX_PAIRS, PASS_FIELDS, PASS_WORDS, PLAN_WORDS, STATIC_LDS,
                              embed_len, make_pass)

GEN = 32
MAXP = 4096
MAX_GROWTH = 3


def embedding(shape, growth):
    """P_c = embed_len(n_c) << growth for n_c > 1, 1 otherwise (three entries)"""
    n = list(shape) + [1] * (3 - len(shape))
    return [embed_len(v) << growth if v > 1 else 1 for v in n]


def feasible(shape, growth):
    return 0 <= growth <= MAX_GROWTH and max(embedding(shape, growth)) <= MAXP


def plan(shape, growth, nsamples, budget=0, forced=0):
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    P = embedding(shape, growth)
    Ptot = P[0] * P[1] * P[2]
    passes = [make_pass(P, d - 1, GEN | INV | (GATHER if d == 1 else 0), n, P[d - 1], n[d - 1])]
    for a in range(d - 2, -1, -1):
        passes.append(make_pass(P, a, INV | (GATHER if a == 0 else 0), n, P[a], n[a]))
    pairs = (nsamples + 1) // 2
    if budget <= 0:
        budget = DEFAULT_BUDGET
    chunk = forced if forced > 0 else budget // (16 * Ptot)
    chunk = max(1, min(chunk, MAX_PAIRS, pairs))
    return dict(d=d, P=P, Ptot=Ptot, growth=growth, pairs=pairs, chunk_pairs=chunk, nchunks=(pairs + chunk - 1) // chunk if pairs else 0,
                pair_bytes=16 * Ptot, twiddles=max(max(P) // 4, 1), Pmax=max(P), passes=passes)


def plan_words(p):
    w = [0] * PLAN_WORDS
    w[:14] = [p["d"], p["P"][0], p["P"][1], p["P"][2], p["Ptot"], p["pairs"], p["chunk_pairs"], p["nchunks"], len(p["passes"]),
              p["pair_bytes"], p["twiddles"], p["Pmax"], STATIC_LDS, p["growth"]]
    for i, q in enumerate(p["passes"]):
        w[HEAD_WORDS + i * PASS_WORDS:HEAD_WORDS + (i + 1) * PASS_WORDS] = [q[f] for f in PASS_FIELDS]
    return w


def predict(L, shape, growth, nsamples, budget=0):
    """the library's words for the same call"""
    words = (C.c_int64 * PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    L.call("hfmi_fftcov_sample_plan_predict", len(shape), C.cast(n, C.c_void_p), int(growth), int(nsamples), int(budget), words)
    return list(words)
