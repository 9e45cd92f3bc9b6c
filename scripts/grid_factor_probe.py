"""Time of an apply of the factor S and of S^T of a grid sampler's embedding (GridCovarianceFactor, hfmi_op_grid_factor; k_fftcov_pass
with the root table, hfmi_fftcov.hip) next to the same operator's apply and to generated-noise draws, in ONE job: 1024 x 1024 and
128 x 128 x 128 nodes, Matern-3/2, 64 vectors, growth 0 and 1 (forced by the tuning key "fftcov_min_growth", negative eigenvalues
clipped), the median of --runs after --warmup (HIP events on the context's stream).  One JSON line per measurement.
    python scripts/grid_factor_probe.py [--runs 10] [--warmup 3] [--k 64] [--only 2d|3d] [--growths 0,1]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402

CASES = {"2d": ((1024, 1024), 0.1), "3d": ((128, 128, 128), 0.2)}     # shape, correlation length on the unit box


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--only", choices=sorted(CASES), default=None)
    ap.add_argument("--growths", default="0,1")
    args = ap.parse_args()
    k = args.k
    ctx = hf.Context.default()
    for name, (shape, ell) in CASES.items():
        if args.only and name != args.only:
            continue
        spacing = tuple(1.0 / (n - 1) for n in shape)
        N = int(np.prod(shape))
        op = hf.GridKernelCovarianceOperator(shape, spacing, family="matern32", sigma=1.0, ell=ell, ctx=ctx)
        X, Y = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
        hf.parRandom.reseed(1)
        hf.parRandom.normal(1.0, X)
        ms_apply, runs_apply = timed(ctx, lambda: op.matMvMult(X, Y), args.runs, args.warmup)
        print(json.dumps({"what": "apply_%s" % name, "grid": list(shape), "N": N, "k": k, "median_ms": round(ms_apply, 3), "runs_ms": runs_apply}), flush=True)
        for g in (int(v) for v in args.growths.split(",")):
            L.call("hfmi_tuning_set", b"fftcov_min_growth", g)
            try:
                smp = op.sampler(max_growth=g, on_indefinite="clip")
            finally:
                L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
            S = smp.factor()
            Ptot = S.shape[1]
            base = {"grid": list(shape), "N": N, "k": k, "growth": smp.growth, "padded_grid": list(smp.embedding), "Ptot": Ptot,
                    "Ptot_over_N": round(Ptot / N, 2), "n_clipped": smp.n_clipped, "cov_error_bound": smp.cov_error_bound}

            def measure(what, fn):
                ms, runs = timed(ctx, fn, args.runs, args.warmup)
                out = {"what": "%s_%s_growth%d" % (what, name, g), "median_ms": round(ms, 3), "runs_ms": runs, "over_apply": round(ms / ms_apply, 3)}
                out.update(base)
                print(json.dumps(out), flush=True)

            # ONE block of k padded vectors, input of S and then output of S^T: at 128^3 and growth 1 it is 8 Ptot k = 64 GiB
            P = hf.MultiVector(Ptot, k, ctx=ctx)
            hf.parRandom.normal(1.0, P)
            measure("S", lambda: S.matMvMult(P, Y))
            measure("St", lambda: S.matMvTranspmult(X, P))
            del P
            measure("draw", lambda: smp.sample(k, 3, out=Y))
            del S, smp
        del op, X, Y
    return 0


if __name__ == "__main__":
    sys.exit(main())
