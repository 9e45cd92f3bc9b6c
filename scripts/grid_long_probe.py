"""The long route of the grid kernel covariance (GridKernelCovarianceOperator(..., long_axes=True): split-line passes of
hfmi_fftcov_plan.h) in ONE job, HIP events on the context's stream, one JSON line per measurement:

  split   the same grid applied by the long route with nothing split (max_line 4096: the old passes) and with every axis split
          (tuning key "fftcov_max_line" = 64), the two operators' applies ALTERNATING --runs times after --warmup, whole applies by
          the context's timer and every pass by the library's profiler ("prof_level" 3: an event pair around each launch).  Bytes by
          section 11's model (every pass reads and writes the padded grid, 32 P bytes per pair) and as moved (16 bytes per loaded
          and stored position of the lines that exist, 8 per entry of Lambda).  By the model a split pass and the unsplit pass of
          its axis move the same bytes, so the bandwidth ratio of a split pass is t(unsplit pass of the axis) / t(split pass); the
          bar is 0.8 for each.  Grids: 1000 x 1000 and config 2's shape (first 1e5 nodes of 316 x 317).
  record  1-D n = 2^20 apply of 64 vectors; 4096 x 4096 apply of 8 vectors (both with natural splits); the 129 x 129 BiLaplacian sampler
          at growth 4 (P_c = 8192): creation (host wall clock around a synchronised create) and 64 draws.

    python scripts/grid_long_probe.py [--runs 6] [--warmup 2] [--only split|record]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def one(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = [one(ctx, fn) for _ in range(runs)]
    return float(np.median(ts)), [round(t, 3) for t in ts]


def make(shape, nodes, max_line, ctx):
    spacing = tuple(1.0 / (n - 1) for n in shape)
    L.call("hfmi_tuning_set", b"fftcov_max_line", max_line)
    try:
        return hf.GridKernelCovarianceOperator(shape, spacing, family="matern32", sigma=1.0, ell=0.1, nodes=nodes, ctx=ctx, long_axes=True)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_max_line", 4096)


def passes_of(shape, max_line):
    P = [1 << max(0, int(2 * n - 2).bit_length()) if n > 1 else 1 for n in shape]
    s = sum(p > max_line for p in P)
    return 2 * (len(shape) + s) - 1, int(np.prod(P))


def pass_times(ctx, op, X, Y):
    """one apply inside a profiling region at "prof_level" 3: {pass index: (ms over its launches, launches, bytes moved, L, flags, part)}"""
    L.call("hfmi_tuning_set", b"prof_level", 3)
    try:
        ctx.profile_begin()
        op.matMvMult(X, Y)
        recs = ctx.profile_end()
    finally:
        L.call("hfmi_tuning_set", b"prof_level", 2)
    return {r["N"]: (r["ms"], r["launches"], r["bytes_per_launch"] * r["launches"], r["m"], r["k"] // 4, r["k"] % 4)
            for r in recs if r["kernel"] == "fftcov_pass"}


# the unsplit pass of the same axis for each pass of a 2-D apply with both axes split: forward axis 0 (high, low), axis 1 (high forward,
# low fused forward-multiply-inverse, high inverse) against the unsplit fused pass of axis 1, inverse axis 0 (low, high)
UNSPLIT_OF = (0, 0, 1, 1, 1, 2, 2)
PART = ("whole", "high", "low")


def split_case(ctx, name, shape, nodes, k, runs, warmup):
    ops = {ml: make(shape, nodes, ml, ctx) for ml in (4096, 64)}
    N = ops[4096].shape[0]
    X, Y = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.reseed(1)
    hf.parRandom.normal(1.0, X)
    for op in ops.values():
        for _ in range(warmup):
            op.matMvMult(X, Y)
    ts = {ml: [] for ml in ops}
    per = {ml: [] for ml in ops}
    for _ in range(runs):                                  # alternating: unsplit, split, unsplit, ...; whole applies, then pass by pass
        for ml, op in ops.items():
            ts[ml].append(one(ctx, lambda: op.matMvMult(X, Y)))
        for ml, op in ops.items():
            per[ml].append(pass_times(ctx, op, X, Y))
    out, med_pass = {}, {}
    P = passes_of(shape, 4096)[1]
    model_bytes = 32.0 * P * ((k + 1) // 2)                # section 11's model: every pass reads and writes the padded grid
    for ml in ops:
        npass = passes_of(shape, ml)[0]
        med = float(np.median(ts[ml]))
        assert all(sorted(r) == list(range(npass)) for r in per[ml]), "one record per pass"
        med_pass[ml] = [float(np.median([r[i][0] for r in per[ml]])) for i in range(npass)]
        out[ml] = dict(median_ms=round(med, 3), runs_ms=[round(t, 3) for t in ts[ml]], passes=npass, P=P,
                       model_GB=round((npass * model_bytes + 16.0 * N * k) / 1e9, 3), sum_of_pass_medians_ms=round(sum(med_pass[ml]), 3))
        emit(what="apply_%s_max_line%d" % (name, ml), grid=list(shape), N=N, k=k, **out[ml])
        for i in range(npass):
            _, launches, moved, Lq, flags, part = per[ml][0][i]
            emit(what="pass_%s_max_line%d" % (name, ml), index=i, L=Lq, flags=flags, part=PART[part], launches=launches,
                 median_ms=round(med_pass[ml][i], 4), runs_ms=[round(r[i][0], 4) for r in per[ml]],
                 model_TBps=round(model_bytes / (med_pass[ml][i] * 1e-3) / 1e12, 3), moved_GB=round(moved / 1e9, 4),
                 moved_TBps=round(moved / (med_pass[ml][i] * 1e-3) / 1e12, 3))
    assert len(med_pass[64]) == len(UNSPLIT_OF) and len(med_pass[4096]) == 3
    ratios = [round(med_pass[4096][UNSPLIT_OF[i]] / med_pass[64][i], 3) for i in range(len(UNSPLIT_OF))]
    emit(what="split_over_unsplit_%s" % name, bandwidth_ratio_per_split_pass=ratios, unsplit_pass_of=list(UNSPLIT_OF), bar=0.8,
         worst=min(ratios), meets_bar=bool(min(ratios) >= 0.8), time_ratio=round(out[64]["median_ms"] / out[4096]["median_ms"], 3))


def record_apply(ctx, name, shape, k, runs, warmup):
    op = make(shape, None, 4096, ctx)
    N = op.shape[0]
    X, Y = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.reseed(2)
    hf.parRandom.normal(1.0, X)
    med, rs = timed(ctx, lambda: op.matMvMult(X, Y), runs, warmup)
    npass, P = passes_of(shape, 4096)
    pass_bytes = 32.0 * P * ((k + 1) // 2)
    emit(what="apply_%s" % name, grid=list(shape), N=N, k=k, passes=npass, P=P, median_ms=round(med, 3), runs_ms=rs,
         model_GB=round((npass * pass_bytes + 16.0 * N * k) / 1e9, 3), per_pass_TBps=round(pass_bytes / (med * 1e-3 / npass) / 1e12, 3))


def record_sampler(ctx, runs, warmup):
    kw = hf.bilaplacian_kernel_2d(0.1, 0.1)
    op = hf.GridKernelCovarianceOperator((129, 129), 1.0 / 128, ctx=ctx, long_axes=True, **kw)
    ctx.synchronize()
    t0 = time.perf_counter()
    s = op.sampler(max_growth=6)
    ctx.synchronize()
    create_ms = (time.perf_counter() - t0) * 1e3
    Y = hf.MultiVector(op.shape[0], 64, ctx=ctx)
    med, rs = timed(ctx, lambda: s.sample(64, 5, out=Y), runs, warmup)
    Ptot = int(np.prod(s.embedding))
    emit(what="sampler_129x129_bilaplacian", growth=s.growth, embedding=list(s.embedding), n_clipped=s.n_clipped,
         ratio=s.lambda_min / s.lambda_max, create_ms=round(create_ms, 1), draws=64, draw_median_ms=round(med, 3), draw_runs_ms=rs,
         ns_per_padded_entry_per_pair=round(med * 1e6 / (Ptot * 32), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("split", "record"), default=None)
    args = ap.parse_args()
    ctx = hf.Context.default()
    if args.only in (None, "split"):
        split_case(ctx, "1000x1000", (1000, 1000), None, 16, args.runs, args.warmup)
        split_case(ctx, "config2", (316, 317), np.arange(100000, dtype=np.int64), 84, args.runs, args.warmup)
    if args.only in (None, "record"):
        record_apply(ctx, "1d_2^20", (1 << 20,), 64, args.runs, args.warmup)
        record_apply(ctx, "4096x4096", (4096, 4096), 8, args.runs, args.warmup)
        record_sampler(ctx, args.runs, args.warmup)
    return 0


if __name__ == "__main__":
    sys.exit(main())
