"""Apply time of the kernel covariance on a regular grid by FFT (GridKernelCovarianceOperator, hfmi_fftcov.hip) next to the matrix-free
operator (KernelCovarianceOperator, hfmi_kcov.hip) in the same job:
  * one apply at config 2's shape: the first 1e5 nodes of the 316 x 317 grid, k = 84 vectors, Matern-3/2, with either operator;
  * one apply of the grid operator on a 1000 x 1000 grid (N = 1e6, k = 84);
  * the KLEProjector('mass') step (rank 64 + 20 probes) at config 2's shape with either operator.
Per line: median milliseconds of --runs after --warmup (HIP events on the context's stream).  For the FFT apply also its algorithmic
traffic -- passes x 32 P bytes per pair of vectors (a read and a write of the padded grid per pass) plus 16 N k for W and Y -- the
achieved bytes/s and that as a fraction of 8 TB/s.  The last line states the one condition: at config 2's shape the grid apply is
faster than the matrix-free apply.  Exit status 1 when it is not.
    python scripts/grid_cov_time.py [--runs 10] [--warmup 3] [--k 84] [--skip-large] [--skip-kle]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402
from hippyflow_amd import workloads  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts)), [round(t, 3) for t in ts]


def plan_of(shape, k):
    words = (C.c_int64 * L.FFTCOV_PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    L.call("hfmi_fftcov_plan_predict", len(shape), C.cast(n, C.c_void_p), k, 0, words)
    return list(words)


def fft_line(what, shape, N, k, ms, all_ms):
    w = plan_of(shape, k)
    P, pairs, passes = w[4], w[5], w[8]
    traffic = passes * 32.0 * P * pairs + 16.0 * N * k
    out = {"what": what, "grid": list(shape), "N": N, "k": k, "median_ms": round(ms, 3), "runs_ms": all_ms, "padded_grid": w[1:1 + len(shape)],
           "passes": passes, "pairs_per_chunk": w[6], "algorithmic_bytes": traffic, "achieved_bytes_per_s": traffic / (ms * 1e-3),
           "fraction_of_8_TB_per_s": round(traffic / (ms * 1e-3) / HBM_BYTES_PER_S, 3)}
    print(json.dumps(out), flush=True)
    return out


def blocks(ctx, N, k):
    W, Y = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.reseed(1)
    hf.parRandom.normal(1.0, W)
    return W, Y


class _Prior:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=84)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-kle", action="store_true")
    args = ap.parse_args()
    ctx = hf.Context.default()
    nx, ny, N, k = 316, 317, 100000, args.k
    grid_wl = workloads.kle_grid_kernel_workload(nx, ny, N=N, sigma=1.0, ell=0.1, ctx=ctx)
    free_wl = workloads.kle_kernel_workload(nx, ny, N=N, sigma=1.0, ell=0.1, ctx=ctx)
    W, Y = blocks(ctx, N, k)
    ms_grid, all_grid = timed(ctx, lambda: grid_wl.C_operator.matMvMult(W, Y), args.runs, args.warmup)
    Yg = Y.to_dense()
    fft_line("grid_fft_apply_config2", (nx, ny), N, k, ms_grid, all_grid)
    ms_free, all_free = timed(ctx, lambda: free_wl.C_operator.matMvMult(W, Y), args.runs, args.warmup)
    Yf = Y.to_dense()
    print(json.dumps({"what": "matrix_free_apply_config2", "N": N, "k": k, "median_ms": round(ms_free, 3), "runs_ms": all_free,
                      "tflops": round(2.0 * N * N * k / ms_free / 1e9, 2),
                      "max_rel_difference_of_the_two_results": float(np.abs(Yg - Yf).max() / np.abs(Yf).max())}), flush=True)
    del W, Y, Yg, Yf
    if not args.skip_kle:
        for name, wl in (("grid_fft", grid_wl), ("matrix_free", free_wl)):
            prior = _Prior()
            prior.M, prior.C = wl.M, wl.C_operator
            params = hf.KLEParameterList()
            params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = 64, k - 64, False, False
            kle = hf.KLEProjector(prior, parameters=params, ctx=ctx)

            def step():
                hf.parRandom.reseed(7)
                kle.construct_input_subspace("mass")

            ms, all_ms = timed(ctx, step, args.runs, args.warmup)
            print(json.dumps({"what": "kle_mass_step_config2_" + name, "N": N, "rank": 64, "probes": k, "median_ms": round(ms, 3),
                              "runs_ms": all_ms, "d_0": float(np.asarray(kle.d_KLE)[0])}), flush=True)
            del kle
    del grid_wl, free_wl
    if not args.skip_large:
        shape = (1000, 1000)
        N1 = shape[0] * shape[1]
        op = hf.GridKernelCovarianceOperator(shape, (1.0 / 999, 1.0 / 999), family="matern32", sigma=1.0, ell=0.1, ctx=ctx)
        W, Y = blocks(ctx, N1, k)
        ms, all_ms = timed(ctx, lambda: op.matMvMult(W, Y), args.runs, args.warmup)
        fft_line("grid_fft_apply_1000x1000", shape, N1, k, ms, all_ms)
    ok = ms_grid < ms_free
    print(json.dumps({"what": "condition", "grid_apply_faster_than_matrix_free_at_config2": bool(ok),
                      "matrix_free_over_grid": round(ms_free / ms_grid, 2)}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
