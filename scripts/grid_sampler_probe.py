"""Time of exact field draws on a regular grid (GridFieldSampler, k_fftcov_draw / k_fftcov_pass of hfmi_fftcov.hip) against the same
operator's apply: for 1024 x 1024 and 128 x 128 x 128 nodes, Matern-3/2, 64 draws next to a 64-vector apply, the median of --runs after
--warmup (HIP events on the context's stream).  The draw is timed on the apply's own embedding (growth 0, negative eigenvalues clipped:
the comparison of d passes with 2 d - 1) and on the embedding the sampler's rule takes when that is another one.  Per pass: the bytes
the plan says it moves -- 16 per entry loaded or stored in the work buffer, 8 per entry of Lambda the noise pass reads (once per
pair here, though the pairs of a chunk can share it through L2), 8 per gathered value.  Per-pass times come from a kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/grid_sampler_probe.py --only 2d --draw-only --runs 1 --warmup 0
    python scripts/grid_sampler_probe.py --only 2d --trace DIR/.../*_kernel_trace.csv
The second call runs nothing on the device: the last chunks x d pass launches of the trace are the one growth-0 draw of the first, pass i
of a chunk is launch i, and it prints time and bytes / time of every pass.
    python scripts/grid_sampler_probe.py [--runs 10] [--warmup 3] [--k 64] [--only 2d|3d] [--max-growth 1] [--draw-only] [--trace CSV]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402

CASES = {"2d": ((1024, 1024), 0.1), "3d": ((128, 128, 128), 0.2)}     # shape, correlation length on the unit box
GEN, GATHER, SCATTER, MUL = 32, 16, 8, 2


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts)) if ts else float("nan"), [round(t, 3) for t in ts]


def plan_words(shape, k, growth=None):
    words = (C.c_int64 * L.FFTCOV_PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    if growth is None:
        L.call("hfmi_fftcov_plan_predict", len(shape), C.cast(n, C.c_void_p), k, 0, words)
    else:
        L.call("hfmi_fftcov_sample_plan_predict", len(shape), C.cast(n, C.c_void_p), growth, k, 0, words)
    return list(words)


def pass_bytes(w, N):
    """per pass and pair of columns: (axis, flags, bytes)"""
    out = []
    for i in range(w[8]):
        axis, flags, Lp, stride, nlines, nload, nstore = w[16 + 16 * i:16 + 16 * i + 7]
        rd = 8 * nlines * Lp if flags & GEN else (16 * N if flags & SCATTER else 16 * nlines * nload)
        if flags & MUL:
            rd += 8 * nlines * Lp
        wr = 16 * N if flags & GATHER else 16 * nlines * nstore
        out.append((axis, flags, rd + wr))
    return out


def trace_times(path, names=("k_fftcov_pass", "k_fftcov_draw")):
    """durations (ms) of the pass launches of a kernel trace, in launch order"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if any(n in r["Kernel_Name"] for n in names):
                rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    return [(n, ms) for _, n, ms in sorted(rows)]


def report(what, shape, N, k, w, ms, all_ms, extra=None):
    pairs, chunk = w[5], w[6]
    per_pass = pass_bytes(w, N)
    total = pairs * sum(b for _, _, b in per_pass)
    out = {"what": what, "grid": list(shape), "N": N, "k": k, "median_ms": round(ms, 3), "runs_ms": all_ms, "padded_grid": w[1:1 + len(shape)],
           "passes": [{"axis": a, "flags": f, "bytes_per_pair": b} for a, f, b in per_pass], "pairs": pairs, "pairs_per_chunk": chunk,
           "bytes": total, "bytes_per_s": total / (ms * 1e-3)}
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--max-growth", type=int, default=1)
    ap.add_argument("--draw-only", action="store_true", help="one sampler at growth 0 and its draws, nothing else (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="kernel trace (csv) of a --draw-only --runs 1 --warmup 0 run with the same --only and --k")
    args = ap.parse_args()
    k = args.k
    if args.trace:
        shape = CASES[args.only][0]
        w = plan_words(shape, k, 0)
        d, nchunks, pairs = w[8], w[7], w[5]
        tail = trace_times(args.trace)[-d * nchunks:]
        assert len(tail) == d * nchunks and "k_fftcov_draw" in tail[0][0], "not the trace of one draw of %d chunks x %d passes" % (nchunks, d)
        for i, (axis, flags, b) in enumerate(pass_bytes(w, int(np.prod(shape)))):
            ms = sum(t for _, t in tail[i::d])
            print(json.dumps({"what": "draw_%s_growth0_pass%d" % (args.only, i + 1), "axis": axis, "flags": flags, "ms": round(ms, 4),
                              "bytes": b * pairs, "bytes_per_s": b * pairs / (ms * 1e-3)}), flush=True)
        return 0
    ctx = hf.Context.default()
    for name, (shape, ell) in CASES.items():
        if args.only and name != args.only:
            continue
        spacing = tuple(1.0 / (n - 1) for n in shape)
        N = int(np.prod(shape))
        op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern32", sigma=1.0, ell=ell, ctx=ctx)
        W, Y = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
        hf.parRandom.reseed(1)
        hf.parRandom.normal(1.0, W)
        wa = plan_words(shape, k)
        ms_apply = float("nan")
        if not args.draw_only:
            ms_apply, all_apply = timed(ctx, lambda: op.matMvMult(W, Y), args.runs, args.warmup)
            report("apply_%s" % name, shape, N, k, wa, ms_apply, all_apply)
        samplers = [("draw_%s_growth0" % name, op.sampler(max_growth=0, on_indefinite="clip"))]
        if not args.draw_only:
            s = op.sampler(max_growth=args.max_growth, on_indefinite="clip")
            if s.growth != 0:
                samplers.append(("draw_%s_growth%d" % (name, s.growth), s))
        for what, smp in samplers:
            ms, all_ms = timed(ctx, lambda: smp.sample(k, 3, out=Y), args.runs, args.warmup)
            w = plan_words(shape, k, smp.growth)
            report(what, shape, N, k, w, ms, all_ms, {
                "growth": smp.growth, "lambda_min_over_max": smp.lambda_min / smp.lambda_max, "n_clipped": smp.n_clipped,
                "cov_error_bound": smp.cov_error_bound, "draw_over_apply": round(ms / ms_apply, 3),
                "passes_over_passes": round(w[8] / wa[8], 3)})
        del op, samplers, W, Y
    return 0


if __name__ == "__main__":
    sys.exit(main())
