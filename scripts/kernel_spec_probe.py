"""What the Matern-1 family and a metric cost the matrix-free kernel covariance, and that the four first families are what they were
(KernelCovarianceOperator / GridKernelCovarianceOperator; hfmi_kcov.hip, hfmi_kcov_k1.h, hfmi_fftcov.hip).  N scattered 2-D points, a block
of k vectors (the documented point: N = 1e5, k = 84, k_kcov<6, .>); per measurement the median and the spread (max - min) of --runs applies
after --warmup (HIP events on the context's stream).  All in one job on one device, every build in a child process of its own:

  (a) matern32 on the PARENT commit: --parent-tree names a built checkout of it
      (git worktree add DIR HEAD~1 && python -c "import sys; sys.path.insert(0, 'DIR'); import __graft_entry__ as g; g.build()"),
      before and after the measurements of this build (a-b-a);
  (b) matern32 on this build;  (c) matern32 with a rotated metric;  (d) matern1;  (e) matern1 with the metric.

Asserted: the median of (b) is within 2 % of the median of (a) (four times the 0.5 % repeat spread recorded for this kernel); and, for
one scattered and one grid case of the four first families, the apply, the sampler's draws and its factor are the parent's bit for bit
(SHA-256 of the results, computed by both builds in this job).  (d) / (b) is reported, with no target.  One JSON line per
measurement, appended to profiles/kernel_spec_probe.jsonl, then the table of docs/measurements.md.
    python scripts/kernel_spec_probe.py --parent-tree DIR [--N 100000] [--k 84] [--runs 10] [--warmup 3]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROTATED = [[1.25, -0.75], [-0.75, 1.25]]                # inv(anisotropy_2d(2, 0.5, pi / 4)): Theta = [[1.25, 0.75], [0.75, 1.25]], det Theta = 1


def timed(ctx, fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return ts


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child(args):
    """one build (the tree this process imports): the timings asked for and the digests of the old families' results"""
    sys.path.insert(0, args.tree)
    import hippyflow_amd as hf
    assert os.path.dirname(os.path.dirname(os.path.abspath(hf.__file__))) == os.path.abspath(args.tree), hf.__file__
    ctx = hf.Context.default()
    N, k = args.N, args.k
    pts = np.random.default_rng(0).random((N, 2))
    W = hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.reseed(1)
    hf.parRandom.normal(1.0, W)
    Y = hf.MultiVector(N, k, ctx=ctx)
    out = {"build_tag": hf._lib.build_tag(), "device": ctx.device_info(), "times_ms": {}, "digests": {}}
    for what in args.what.split(","):
        family, _, metric = what.partition("+")
        kw = {"metric": np.array(ROTATED)} if metric else {}
        op = hf.KernelCovarianceOperator(pts, family=family, sigma=1.0, ell=0.1, ctx=ctx, **kw)
        out["times_ms"][what] = timed(ctx, lambda: op.matMvMult(W, Y), args.runs, args.warmup)
        if what == "matern32":
            out["digests"]["scattered apply matern32 N=%d k=%d" % (N, k)] = digest(Y.to_dense())
        del op
    # the four first families at a size whose results can be hashed whole: scattered apply and rows; grid apply, draws, factor
    n, kk = 3001, 17
    Ws = np.random.default_rng(2).standard_normal((n, kk))
    for family in ("matern12", "matern32", "matern52", "sqexp"):
        op = hf.KernelCovarianceOperator(pts[:n], family=family, sigma=1.3, ell=0.2, nugget=0.1, ctx=ctx)
        Ys = hf.MultiVector(n, kk, ctx=ctx)
        op.matMvMult(hf.MultiVector.from_dense(Ws, ctx=ctx), Ys)
        out["digests"]["scattered apply %s" % family] = digest(Ys.to_dense())
        g = hf.GridKernelCovarianceOperator((64, 40), (0.013, 0.021), family=family, sigma=1.3, ell=0.2, nugget=0.1, ctx=ctx)
        Wg = np.random.default_rng(3).standard_normal((64 * 40, 5))
        Yg = hf.MultiVector(64 * 40, 5, ctx=ctx)
        g.matMvMult(hf.MultiVector.from_dense(Wg, ctx=ctx), Yg)
        out["digests"]["grid apply %s" % family] = digest(Yg.to_dense())
        s = g.sampler(max_growth=3, on_indefinite="clip", seed=5)
        out["digests"]["grid draws %s" % family] = digest(s.sample(4, seed=5).to_dense())
        S = s.factor()
        V = hf.MultiVector(S.shape[1], 5, ctx=ctx)
        S.transpose().matMvMult(hf.MultiVector.from_dense(Wg, ctx=ctx), V)
        out["digests"]["grid factor %s" % family] = digest(V.to_dense())
    f = hf.pivoted_cholesky(hf.KernelCovarianceOperator(pts[:n], family="matern32", sigma=1.3, ell=0.2, ctx=ctx), 30)
    out["digests"]["pivoted cholesky matern32"] = digest(f.L.to_dense())
    print(json.dumps(out), flush=True)


def run_child(tree, what, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", os.path.abspath(tree), "--what", what, "--N", str(args.N),
           "--k", str(args.k), "--runs", str(args.runs), "--warmup", str(args.warmup)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("measurement of %s failed (exit %d):\n%s" % (tree, out.returncode, out.stderr[-2000:]))
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--what", default="matern32")
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--k", type=int, default=84)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "kernel_spec_probe.jsonl"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_tree:
        ap.error("--parent-tree is needed for (a)")
    before = run_child(args.parent_tree, "matern32", args)
    this = run_child(args.tree, "matern32,matern32+metric,matern1,matern1+metric", args)
    after = run_child(args.parent_tree, "matern32", args)
    assert before["build_tag"] == after["build_tag"] != this["build_tag"], "the parent tree is this build"
    rows = []

    def record(what, ts, tag):
        ts = np.asarray(ts)
        flops = 2.0 * args.N * args.N * args.k
        r = {"what": what, "N": args.N, "k": args.k, "median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3),
             "max_ms": round(float(ts.max()), 3), "spread_ms": round(float(ts.max() - ts.min()), 3), "runs": len(ts),
             "tflops": round(flops / (float(np.median(ts)) * 1e-3) / 1e12, 2), "build_tag": tag, "device": this["device"]}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    a = record("(a) matern32, parent commit", before["times_ms"]["matern32"] + after["times_ms"]["matern32"], before["build_tag"])
    b = record("(b) matern32, this build", this["times_ms"]["matern32"], this["build_tag"])
    record("(c) matern32 with a metric", this["times_ms"]["matern32+metric"], this["build_tag"])
    d = record("(d) matern1", this["times_ms"]["matern1"], this["build_tag"])
    record("(e) matern1 with a metric", this["times_ms"]["matern1+metric"], this["build_tag"])
    differing = sorted(key for key in before["digests"] if before["digests"][key] != this["digests"].get(key) or after["digests"][key] != before["digests"][key])
    verdict = {"what": "verdict", "matern32_over_parent": round(b["median_ms"] / a["median_ms"], 4), "within_2_percent": bool(abs(b["median_ms"] / a["median_ms"] - 1.0) <= 0.02),
               "matern1_over_matern32": round(d["median_ms"] / b["median_ms"], 3), "results_compared": len(before["digests"]), "results_differing": differing}
    rows.append(verdict)
    print(json.dumps(verdict), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
    print("\n| measurement | median ms | min .. max ms | spread ms | TF | runs | build |")
    print("|---|---|---|---|---|---|---|")
    for r in rows[:-1]:
        print("| %s | %.3f | %.3f .. %.3f | %.3f | %.2f | %d | `%s` |" % (r["what"], r["median_ms"], r["min_ms"], r["max_ms"], r["spread_ms"], r["tflops"],
                                                                      r["runs"], r["build_tag"]))
    print("\n(b) / (a) = %.4f; (d) / (b) = %.3f; %d results of the four first families compared with the parent's, %d differ"
          % (verdict["matern32_over_parent"], verdict["matern1_over_matern32"], verdict["results_compared"], len(differing)))
    assert not differing, "results of the first four families differ from the parent's: %s" % differing
    assert verdict["within_2_percent"], "matern32 is %.2f %% away from the parent's median" % (100.0 * (verdict["matern32_over_parent"] - 1.0))


if __name__ == "__main__":
    main()
