"""One SHA-256 per case over the output bytes of small applies, draws and factor applies that run the in-LDS line transform
(hfmi_fft_lds.h) through every kernel that holds it: k_fftcov_pass, k_fftcov_draw, k_fftcov_factor, k_fftcov_split, k_fftcov_split_draw,
k_boxcov_pass and k_boxcov_pass_mr.  Fixed inputs (numpy's default_rng with the seed of the case) and fixed draw seeds, every case a few
thousand nodes at the most.  Run it once per build, a fresh process each (HFMI_LIB selects the library), and compare the columns: a
change that keeps the order of the floating-point operations keeps every digest.  Nothing is asserted.
    HFMI_LIB=/path/to/libhfmi.so python scripts/fft_lds_digests.py [--label this] [--out profiles/fft_lds_digests.jsonl]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402

NEU, PER = "neumann", "periodic"
# (shape, max_line or None, nodes: a seeded 3/4 subset?)
GRID_APPLY = [((33,), None, False), ((17, 9), None, True), ((7, 5, 3), None, False), ((3, 1), None, False),
              ((13, 5), 8, False), ((65,), 16, False), ((5, 3, 6), 4, True)]
# (shape, max_line or None, forced growth)
GRID_DRAW = [((33,), None, 0), ((2,), None, 0), ((3,), None, 0), ((13, 5), None, 2), ((5, 3), None, 0), ((7, 6, 5), None, 0),
             ((9,), 16, 2), ((9, 8), 8, 1), ((3,), 4, 0)]
# d = 1: the fused pass of k_fftcov_factor; (6, 5): passes of k_fftcov_pass on the root table
GRID_FACTOR = [((1,), 0), ((2,), 0), ((3,), 0), ((7,), 0), ((7,), 1), ((33,), 2), ((6, 5), 1)]
BOX = [((33,), NEU), ((32,), PER), ((2,), NEU), ((9, 5), NEU), ((3, 9), NEU), ((3, 2), NEU), ((3, 1), NEU), ((8, 5), (PER, NEU)), ((5, 3, 4), (NEU, NEU, PER)),
       ((7,), NEU), ((11,), NEU), ((13,), NEU), ((31,), NEU), ((60,), PER), ((13, 11), NEU), ((3, 13), NEU), ((3, 31), NEU), ((31, 3), NEU),
       ((7, 3, 12), (NEU, NEU, PER)), ((9, 7), NEU), ((7, 9), NEU), ((12, 8), PER), ((5, 7, 4), (NEU, NEU, PER)), ((97, 33), NEU)]


def digest(mv):
    return hashlib.sha256(np.ascontiguousarray(mv.to_dense()).tobytes()).hexdigest()[:16]


def name(shape, *more):
    return "x".join(map(str, shape)) + "".join("-%s" % m for m in more if m not in (None, False, ""))


def block(ctx, N, k, seed):
    return hf.MultiVector.from_dense(np.ascontiguousarray(np.random.default_rng(seed).standard_normal((N, k))), ctx=ctx)


def grid_op(ctx, shape, ml, subset):
    d = len(shape)
    nodes = None
    if subset:
        total = int(np.prod(shape))
        nodes = np.sort(np.random.default_rng(total).permutation(total)[:3 * total // 4]).astype(np.int64)
    if ml is None:
        return hf.GridKernelCovarianceOperator(shape, (0.2, 0.25, 0.3)[:d], family="matern12", sigma=1.3, ell=0.4, nodes=nodes, ctx=ctx)
    L.call("hfmi_tuning_set", b"fftcov_max_line", ml)
    try:
        return hf.GridKernelCovarianceOperator(shape, (0.2, 0.25, 0.3)[:d], family="matern12", sigma=1.3, ell=0.4, nodes=nodes, ctx=ctx, long_axes=True)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_max_line", 4096)


def sampler(op, growth):
    L.call("hfmi_tuning_set", b"fftcov_min_growth", growth)
    try:
        return op.sampler(max_growth=growth, on_indefinite="clip")
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = hf.Context.default()
    out = open(args.out, "a") if args.out else None

    def emit(what, case, value):
        text = json.dumps({"what": "fft_lds_digest", "build": args.label, "kind": what, "case": case, "sha256_16": value})
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()

    def run(what, case, fn):
        try:                                   # a refused case is recorded as such: both builds must refuse it alike
            emit(what, case, fn())
        except (hf.HfmiError, ValueError) as e:
            emit(what, case, "refused: %s" % e)

    def grid_apply(shape, ml, subset):
        op = grid_op(ctx, shape, ml, subset)
        N = op.shape[0]
        Y = hf.MultiVector(N, 3, ctx=ctx)
        op.matMvMult(block(ctx, N, 3, N), Y)
        return digest(Y)

    def grid_factor(shape, growth):
        S = sampler(grid_op(ctx, shape, None, False), growth).factor()
        N, Ptot = S.shape
        Y = hf.MultiVector(N, 3, ctx=ctx)
        S.matMvMult(block(ctx, Ptot, 3, Ptot), Y)
        Z = hf.MultiVector(Ptot, 3, ctx=ctx)
        S.transpose().matMvMult(block(ctx, N, 3, N + 1), Z)
        return digest(Y) + "," + digest(Z)

    def box_crs(shape, boundary):
        d = len(shape)
        box = hf.BoxSpectralCovariance(shape, (0.3, 0.2, 0.25)[:d], 0.7, 1.3, alpha=2.0, theta=(1.0, 2.5, 0.5)[:d], boundary=boundary, ctx=ctx)
        X = block(ctx, box.N, 3, box.N)
        parts = []
        for op in (box.C, box.R, box.S):
            Y = hf.MultiVector(box.N, 3, ctx=ctx)
            op.matMvMult(X, Y)
            parts.append(digest(Y))
        return ",".join(parts)

    for shape, ml, subset in GRID_APPLY:
        run("grid_apply", name(shape, ml and "ml%d" % ml, subset and "subset"), lambda: grid_apply(shape, ml, subset))
    for shape, ml, growth in GRID_DRAW:
        run("grid_draw", name(shape, ml and "ml%d" % ml, "g%d" % growth), lambda: digest(sampler(grid_op(ctx, shape, ml, False), growth).sample(5, 7)))
    for shape, growth in GRID_FACTOR:
        run("grid_factor", name(shape, "g%d" % growth), lambda: grid_factor(shape, growth))
    for shape, boundary in BOX:
        b = [boundary] * len(shape) if isinstance(boundary, str) else boundary
        run("box_CRS", "x".join("%d%s" % (n, v[0]) for n, v in zip(shape, b)), lambda: box_crs(shape, boundary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
