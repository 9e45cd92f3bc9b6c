"""What an entry of the general Matern family costs beside the named ones: one apply of KernelCovarianceOperator at N = 32768 scattered
2-D points, k = 32 vectors (k_kcov<2, .>), for "matern32", "matern1" and "matern" with nu = 1.25 (hfmi_kcov.hip, hfmi_kcov_k1.h,
hfmi_kcov_nu.h).  One process, one device; after --warmup applies of every operator, --rounds rounds that alternate the three operators,
each timing a window of --reps applies by HIP events on the context's stream (a window is a few tens of milliseconds: one apply alone
would measure the clock's ramp).  Reported per family: the median, minimum and maximum over the rounds of the time of ONE apply, and the
ratios of the medians.  There is no bar to meet; the first two families exist on the parent commit and must not move
(scripts/kernel_spec_probe.py holds matern32 to the parent's time and bits).  One JSON line per family and one of ratios, appended to
profiles/matern_nu_probe.jsonl, then the table of docs/measurements.md.
    python scripts/matern_nu_probe.py [--N 32768] [--k 32] [--nu 1.25] [--rounds 9] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=32768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--nu", type=float, default=1.25)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "matern_nu_probe.jsonl"))
    args = ap.parse_args()
    import hippyflow_amd as hf
    if hf.device_count() < 1:
        raise RuntimeError("the probe needs a GPU: libhfmi has no CPU path")
    ctx = hf.Context.default()
    N, k = args.N, args.k
    pts = np.random.default_rng(0).random((N, 2))
    W = hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.reseed(1)
    hf.parRandom.normal(1.0, W)
    Y = hf.MultiVector(N, k, ctx=ctx)
    kernels = [("matern32", {}), ("matern1", {}), ("matern nu=%g" % args.nu, {"nu": args.nu})]
    ops = [hf.KernelCovarianceOperator(pts, family=name.split()[0], sigma=1.0, ell=0.1, ctx=ctx, **kw) for name, kw in kernels]
    for op in ops:
        for _ in range(args.warmup):
            op.matMvMult(W, Y)
    times = [[] for _ in ops]
    for _ in range(args.rounds):
        for i, op in enumerate(ops):
            ctx.timer_start()
            for _ in range(args.reps):
                op.matMvMult(W, Y)
            times[i].append(ctx.timer_stop() / args.reps)
    assert np.all(np.isfinite(Y.to_dense()))
    rows = []
    flops = 2.0 * N * N * k
    for (name, _), ts in zip(kernels, times):
        ts = np.asarray(ts)
        rows.append({"what": name, "N": N, "k": k, "median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4),
                     "max_ms": round(float(ts.max()), 4), "rounds": args.rounds, "applies_per_window": args.reps,
                     "tflops": round(flops / (float(np.median(ts)) * 1e-3) / 1e12, 2), "build_tag": hf._lib.build_tag(),
                     "device": ctx.device_info()})
    m32, m1, mnu = (r["median_ms"] for r in rows)
    rows.append({"what": "ratios", "matern1_over_matern32": round(m1 / m32, 3), "matern_nu_over_matern32": round(mnu / m32, 3),
                 "matern_nu_over_matern1": round(mnu / m1, 3)})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for r in rows:
            print(json.dumps(r), flush=True)
            fh.write(json.dumps(r) + "\n")
    print("\n| kernel | median ms | min .. max ms | TF | rounds x applies |")
    print("|---|---|---|---|---|")
    for r in rows[:-1]:
        print("| %s | %.4f | %.4f .. %.4f | %.2f | %d x %d |" % (r["what"], r["median_ms"], r["min_ms"], r["max_ms"], r["tflops"], r["rounds"],
                                                             r["applies_per_window"]))
    print("\nmatern1 / matern32 = %.3f; matern(nu) / matern32 = %.3f; matern(nu) / matern1 = %.3f" % (m1 / m32, mnu / m32, mnu / m1))


if __name__ == "__main__":
    main()
