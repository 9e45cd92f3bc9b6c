"""What the rectangular kernel covariance costs the square operator, and how far a row shard fills the device
(KernelCovarianceOperator / .rows, hfmi_kcov.hip).  N grid points (d = 2, Matern-3/2), a block of k vectors; per measurement the median and
the spread (max - min) of --runs applies after --warmup (HIP events on the context's stream).  All in one job on one device:

  (a) the square operator's apply on the PARENT commit: --parent-tree names a built checkout of it
      (git worktree add DIR HEAD~1 && python -c "import sys; sys.path.insert(0, 'DIR'); import __graft_entry__ as g; g.build()"),
      timed by this script in child processes, before and after the measurements of this build (a-b-a);
  (b) the square operator's apply on this build;
  (c) the slab with all rows, rows(0, N), on this build;
  (d) slabs of N/2, N/4, N/8 rows, with the tile arithmetic: 128-row tiles against the compute units.

The bar: (b) and (c) are not slower than (a) by more than the spread of (a) over its repeated runs.  One JSON line per measurement, then the
table of docs/measurements.md.
    python scripts/kernel_cross_cov_time.py --parent-tree DIR [--N 131072] [--k 84] [--runs 10] [--warmup 3]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return ts


def setup(tree, N, k):
    sys.path.insert(0, tree)
    import hippyflow_amd as hf
    from hippyflow_amd import workloads
    assert os.path.dirname(os.path.dirname(os.path.abspath(hf.__file__))) == os.path.abspath(tree), hf.__file__
    ctx = hf.Context.default()
    nx = int(np.ceil(np.sqrt(N)))
    wl = workloads.kle_kernel_workload(nx, nx + 1, N=N, sigma=1.0, ell=0.1, ctx=ctx)
    W = hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.reseed(1)
    hf.parRandom.normal(1.0, W)
    return hf, ctx, wl.C_operator, W, hf.MultiVector(N, k, ctx=ctx)


def square_only(args):
    """child: the square apply of the tree this process imports"""
    hf, ctx, C_op, W, Y = setup(args.tree, args.N, args.k)
    ts = timed(ctx, lambda: C_op.matMvMult(W, Y), args.runs, args.warmup)
    print(json.dumps({"times_ms": ts, "build_tag": hf._lib.build_tag(), "checksum": float(np.abs(Y.to_dense()).sum())}), flush=True)


def parent_times(args):
    cmd = [sys.executable, os.path.abspath(__file__), "--square-only", "--tree", os.path.abspath(args.parent_tree), "--N", str(args.N),
           "--k", str(args.k), "--runs", str(args.runs), "--warmup", str(args.warmup)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError("parent measurement failed:\n" + out.stderr[-2000:])
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--square-only", action="store_true")
    ap.add_argument("--N", type=int, default=131072)
    ap.add_argument("--k", type=int, default=84)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.square_only:
        return square_only(args)
    if not args.parent_tree:
        ap.error("--parent-tree is needed for (a)")
    N, k = args.N, args.k
    rows = []

    def record(what, ts, nrows, **extra):
        ts = np.asarray(ts)
        r = {"what": what, "N": N, "k": k, "rows": nrows, "median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3),
             "max_ms": round(float(ts.max()), 3), "spread_ms": round(float(ts.max() - ts.min()), 3), "runs": len(ts)}
        r.update(extra)
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    before = parent_times(args)
    hf, ctx, C_op, W, Y = setup(args.tree, N, k)
    cus = ctx.device_info()["compute_units"]
    tag = hf._lib.build_tag()
    b = record("(b) square apply, this build", timed(ctx, lambda: C_op.matMvMult(W, Y), args.runs, args.warmup), N, build_tag=tag)
    checksum = float(np.abs(Y.to_dense()).sum())
    for what, nrows in (("(c) slab of all rows", N), ("(d) slab of N/2 rows", N // 2), ("(d) slab of N/4 rows", N // 4), ("(d) slab of N/8 rows", N // 8)):
        slab = C_op.rows(0, nrows)
        tiles = -(-nrows // 128)
        record(what, timed(ctx, lambda: slab.matMvMult(W, Y), args.runs, args.warmup), nrows, build_tag=tag, tiles_of_128_rows=tiles,
               compute_units=cus, tiles_per_cu=round(tiles / cus, 2))
    del C_op, W, Y
    ctx.synchronize()
    after = parent_times(args)
    assert before["build_tag"] == after["build_tag"] != tag, "the parent tree is this build"
    assert before["checksum"] == after["checksum"] == checksum, "the parent computes something else"
    a = record("(a) square apply, parent commit", before["times_ms"] + after["times_ms"], N, build_tag=before["build_tag"])
    rows.insert(0, rows.pop())
    c = rows[2]
    verdict = {"bar_ms": round(a["median_ms"] + a["spread_ms"], 3), "b_within_bar": b["median_ms"] <= a["median_ms"] + a["spread_ms"],
               "c_within_bar": c["median_ms"] <= a["median_ms"] + a["spread_ms"]}
    print(json.dumps(verdict), flush=True)
    print("\n| measurement | rows | 128-row tiles | tiles / CU (%d CUs) | median ms | min .. max ms | spread ms | runs | build |" % cus)
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        tiles = -(-r["rows"] // 128)
        print("| %s | %d | %d | %.2f | %.3f | %.3f .. %.3f | %.3f | %d | `%s` |" % (r["what"], r["rows"], tiles, tiles / cus, r["median_ms"],
              r["min_ms"], r["max_ms"], r["spread_ms"], r["runs"], r["build_tag"]))
    print("\n(b) and (c) against (a): median(a) + spread(a) = %.3f ms; (b) %s, (c) %s" % (
        verdict["bar_ms"], "within" if verdict["b_within_bar"] else "SLOWER", "within" if verdict["c_within_bar"] else "SLOWER"))


if __name__ == "__main__":
    main()
