"""Apply time of the factor K = F F^T, F = [W S | diag(sqrt(delta))], of the interpolated grid covariance
(InterpolatedCovarianceFactor, hfmi_op_interp_factor) against the apply of K itself, in one job:
  * N random points (default 1e6) in the unit square on a 1024 x 1024 grid, Matern-5/2, ell / h = 8, 16 columns;
  * (a) F (noise -> points), (b) F^T (points -> noise), (c) K's apply.
Per line: median milliseconds of --runs INTERLEAVED repetitions (a, b, c, a, b, c, ...) after --warmup, HIP events on the context's
stream, with every repetition's time.  The embedding is the one of growth --growth (negative eigenvalues clipped if there are any: the
passes and their cost are the same), reported with the line.  Nothing is asserted: no factor apply on this route had been timed before.
    python scripts/measure_interp_factor.py [--points 1000000] [--runs 7] [--warmup 2] [--columns 16] [--growth 0]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402


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
    return [float(np.median(t)) for t in ts], [[round(v, 3) for v in t] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--columns", default="16")
    ap.add_argument("--growth", type=int, default=0)
    args = ap.parse_args()
    ctx = hf.Context.default()
    shape, N = (1024, 1024), args.points
    h = 1.0 / (shape[0] - 3)                    # the unit box spans nodes 1 .. n - 2
    pts = np.random.default_rng(2).random((N, 2))
    grid = hf.GridKernelCovarianceOperator(shape, h, family="matern52", sigma=1.0, ell=8 * h, origin=(-h, -h), ctx=ctx)
    K = hf.InterpolatedKernelCovarianceOperator.on_grid(grid, pts)
    L.call("hfmi_tuning_set", b"fftcov_min_growth", args.growth)
    try:
        s = K.sampler(max_growth=args.growth, on_indefinite="clip")
    finally:
        L.call("hfmi_tuning_set", b"fftcov_min_growth", 0)
    F = s.factor()
    Ft = F.transpose()
    Ptot = F.noise_split[0]
    for k in (int(c) for c in args.columns.split(",")):
        Xi, X, Y, Z, KX = (hf.MultiVector(Ptot + N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx),
                           hf.MultiVector(Ptot + N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx))
        hf.parRandom.reseed(1)
        hf.parRandom.normal(1.0, Xi)
        hf.parRandom.normal(1.0, X)
        (a, b, c), runs = interleaved(ctx, [lambda: F.matMvMult(Xi, Y), lambda: Ft.matMvMult(X, Z), lambda: K.matMvMult(X, KX)], args.runs, args.warmup)
        # F (F^T X) against K X: rounding for a definite embedding, the clip's bound otherwise
        F.matMvMult(Z, Y)
        diff = float(np.abs(Y.to_dense() - KX.to_dense()).max() / np.abs(KX.to_dense()).max())
        print(json.dumps({"what": "apply", "N": N, "k": k, "grid": list(shape), "embedding": list(s.embedding), "growth": s.growth, "n_clipped": s.n_clipped,
                          "factor_error_bound": F.factor_error_bound, "noise_entries": Ptot + N, "F_ms": round(a, 3), "Ft_ms": round(b, 3), "K_ms": round(c, 3),
                          "F_over_K": round(a / c, 3), "Ft_over_K": round(b / c, 3), "runs_ms": runs, "max_rel_F_Ft_X_minus_K_X": diff}), flush=True)
        del Xi, X, Y, Z, KX
    return 0


if __name__ == "__main__":
    sys.exit(main())
