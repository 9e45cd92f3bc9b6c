"""Apply time of the box Whittle-Matern operators (BoxSpectralCovariance, hfmi_op_box) on grids with mixed-radix lines and on their
power-of-two neighbours, in one job:
  * C and S with --columns columns (default 16) on (193, 193), (769, 769) and (97, 97, 97) Neumann (lines of 384, 1536 and 192 entries:
    k_boxcov_pass_mr) and on (129, 129), (257, 257), (513, 513), (1025, 1025), (65, 65, 65) and (129, 129, 129) Neumann (k_boxcov_pass);
  * --pow2-only skips the mixed-radix grids, so that the same script runs on a build without them: the power-of-two grids run the same
    kernel on both builds and their times must agree.
Per line: median milliseconds of --runs INTERLEAVED repetitions (C, S, C, S, ...) after --warmup, HIP events on the context's stream,
every repetition's time, and nanoseconds per node per column so that the sizes compare.  Nothing is asserted.
    python scripts/measure_box_sizes.py [--runs 11] [--warmup 3] [--columns 16] [--pow2-only] [--label this] [--out profiles/box_sizes_time.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402

MIXED = [(193, 193), (769, 769), (97, 97, 97)]
POW2 = [(129, 129), (257, 257), (513, 513), (1025, 1025), (65, 65, 65), (129, 129, 129)]


def interleaved(ctx, fns, runs, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            ctx.timer_start()
            fn()
            ts[i].append(ctx.timer_stop())
    return [float(np.median(t)) for t in ts], [[round(v, 4) for v in t] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--pow2-only", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = hf.Context.default()
    k = args.columns
    out = open(args.out, "a") if args.out else None
    for shape in sorted(POW2 + ([] if args.pow2_only else MIXED), key=lambda s: (len(s), s)):
        d = len(shape)
        box = hf.BoxSpectralCovariance(shape, 1.0 / (shape[0] - 1), 0.7, 1.3, alpha=2.0, theta=(1.0, 2.5, 0.5)[:d], ctx=ctx)
        N = box.N
        X, Y, Z = (hf.MultiVector(N, k, ctx=ctx) for _ in range(3))
        hf.parRandom.reseed(1)
        hf.parRandom.normal(1.0, X)
        Cop, Sop = box.C, box.S
        (c_ms, s_ms), runs = interleaved(ctx, [lambda: Cop.matMvMult(X, Y), lambda: Sop.matMvMult(X, Z)], args.runs, args.warmup)
        lines = [2 * (n - 1) for n in shape]
        rec = {"what": "box_apply", "build": args.label, "grid": list(shape), "lines": lines, "mixed_radix": any(v & (v - 1) for v in lines),
               "N": N, "k": k, "C_ms": round(c_ms, 4), "S_ms": round(s_ms, 4), "C_ns_per_node_col": round(c_ms * 1e6 / (N * k), 4),
               "S_ns_per_node_col": round(s_ms * 1e6 / (N * k), 4), "runs_ms": runs}
        text = json.dumps(rec)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        del X, Y, Z, box, Cop, Sop
    return 0


if __name__ == "__main__":
    sys.exit(main())
