"""Apply time of the matrix-free kernel covariance operator (KernelCovarianceOperator, hfmi_kcov.hip) for a block of k vectors on
config 2's grid nodes, next to the explicit path where that fits: the one-off fill of the N x N block (hfmi_block_fill_matern32) and the
apply of hfmi_op_dense_sym.  Per line: median milliseconds of --runs applies after --warmup (HIP events on the context's stream),
2 N^2 k / t as a fraction of the 78.6 TF fp64 MFMA peak, and kernel evaluations per second (N^2 / t).  One JSON line per measurement.
    python scripts/kernel_cov_time.py [--sizes 100000,250000,1000000] [--explicit-up-to 100000] [--k 84] [--runs 5] [--warmup 2]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import workloads  # noqa: E402

PEAK_TF = 78.6


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts))


def line(what, N, k, ms, **extra):
    flops = 2.0 * N * N * k
    out = {"what": what, "N": N, "k": k, "median_ms": round(ms, 3), "tflops": round(flops / ms / 1e9, 2),
           "fraction_of_fp64_mfma_peak": round(flops / ms / 1e9 / PEAK_TF, 3), "evaluations_per_s": N * N / (ms * 1e-3) if what == "matrix_free_apply" else None}
    out.update(extra)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,250000,1000000")
    ap.add_argument("--explicit-up-to", type=int, default=100000)
    ap.add_argument("--k", type=int, default=84)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    ctx = hf.Context.default()
    for N in [int(s) for s in args.sizes.split(",")]:
        nx = int(np.ceil(np.sqrt(N)))
        ny = nx + 1
        k = args.k
        W = hf.MultiVector(N, k, ctx=ctx)
        hf.parRandom.reseed(1)
        hf.parRandom.normal(1.0, W)
        Y = hf.MultiVector(N, k, ctx=ctx)
        runs, warmup = (args.runs, args.warmup) if N <= 300000 else (max(1, args.runs // 2), 1)
        wl = workloads.kle_kernel_workload(nx, ny, N=N, sigma=1.0, ell=0.1, ctx=ctx)
        ms = timed(ctx, lambda: wl.C_operator.matMvMult(W, Y), runs, warmup)
        line("matrix_free_apply", N, k, ms, family="matern32", grid=[nx, ny], runs=runs)
        if N <= args.explicit_up_to:
            Yf = Y.to_dense()
            del wl
            Cb = hf.MultiVector(N, N, ctx=ctx)
            ctx.timer_start()
            workloads.matern32_covariance(Cb, nx, ny, 1.0, 0.1)
            fill_ms = ctx.timer_stop()
            op = hf.npToDeviceOperator(Cb)
            ms_e = timed(ctx, lambda: op.matMvMult(W, Y), runs, warmup)
            Ye = Y.to_dense()
            line("explicit_apply", N, k, ms_e, fill_ms=round(fill_ms, 2), block_gb=round(8.0 * N * N / 1e9, 1),
                 max_rel_difference_of_the_two_results=float(np.abs(Yf - Ye).max() / np.abs(Ye).max()))
            del op, Cb


if __name__ == "__main__":
    main()
