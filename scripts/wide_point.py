"""First timings of the wide route (256 < k <= 2048 vectors): ``MultiVector.orthogonalize`` (Cholesky-QR, hfmi_borth_qr without the
read-back of R) on a Gaussian block and ``doublePass`` (r = k - 48, s = 1) on a ``SnapshotGramOperator`` of k + 64 Gaussian snapshots,
at every (N, k) of --points.  The orthogonalisation is split with the per-launch records of a profiling region: ``gram_ms`` is the
sum over the passes of the Gram contractions (k_tsgemm_tn), ``qrinv_ms`` of the Q R^-1 contractions (k_tsgemm_nn), and ``kxk_ms`` is the
rest of the wall clock -- the k x k stage: the blocked Cholesky + inverse + R product of hfmi_chol_wide.hip, its status read-back
(one host round trip per pass) and the final R_jj table.  ``kxk_share`` = kxk_ms / wall_ms is the figure docs/measurements.md section 5
quotes.  Every time is the median of --runs repetitions after a warm-up of both routines at N = 8192, k = 320.  Writes one JSON document.
    python scripts/wide_point.py [--points 100000:512,...] [--runs 3] [--out profiles/wide_point.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import _lib as L  # noqa: E402

DEFAULT_POINTS = "100000:512,100000:1024,100000:2048,1000000:512,1000000:1024,1000000:2048"


def gaussian(ctx, N, k, seed):
    hf.parRandom.reseed(seed)
    B = hf.MultiVector(N, k, ctx=ctx)
    hf.parRandom.normal(1.0, B)
    return B


def orthogonalize_once(ctx, Z):
    """(wall ms, gram ms, Q R^-1 ms, passes) of one Cholesky-QR of a copy of Z"""
    Q = hf.MultiVector(Z)
    passes = C.c_int(0)
    ctx.synchronize()
    ctx.profile_begin()
    t0 = time.perf_counter()
    L.call("hfmi_borth_qr", Q.handle, None, None, None, L.QR_CHOL, C.byref(passes))
    ctx.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    recs = ctx.profile_end()
    tn = sum(r["ms"] for r in recs if r["kernel"] == "k_tsgemm_tn")
    nn = sum(r["ms"] for r in recs if r["kernel"] == "k_tsgemm_nn")
    return wall, tn, nn, passes.value


def double_pass_once(ctx, op, Omega, r):
    ctx.synchronize()
    ctx.profile_begin()
    t0 = time.perf_counter()
    d, U = hf.doublePass(op, Omega, r, s=1)
    ctx.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    ctx.profile_end()
    return wall, ctx.profile_phases(), float(d[0]), float(d[-1])


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default=DEFAULT_POINTS)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "wide_point.json"))
    args = ap.parse_args()
    ctx = hf.Context.default()
    points = [tuple(int(x) for x in p.split(":")) for p in args.points.split(",")]
    wZ = gaussian(ctx, 8192, 320, 1)
    orthogonalize_once(ctx, wZ)
    double_pass_once(ctx, hf.SnapshotGramOperator(gaussian(ctx, 8192, 384, 2)), wZ, 272)
    del wZ
    doc = {"device": ctx.device_info(), "build_tag": hf.build_tag(), "runs": args.runs, "points": []}
    for N, k in points:
        Z = gaussian(ctx, N, k, 10 + k)
        runs = [orthogonalize_once(ctx, Z) for _ in range(args.runs)]
        wall, tn, nn = med([r[0] for r in runs]), med([r[1] for r in runs]), med([r[2] for r in runs])
        rec = {"N": N, "k": k, "qr_passes": runs[0][3], "qr_wall_ms": round(wall, 3), "gram_ms": round(tn, 3), "qrinv_ms": round(nn, 3),
               "kxk_ms": round(wall - tn - nn, 3), "kxk_share": round((wall - tn - nn) / wall, 4),
               "qr_wall_ms_runs": [round(r[0], 3) for r in runs]}
        X = gaussian(ctx, N, k + 64, 20 + k)                 # k + 64 snapshots: the operator's rank exceeds the probe count
        op = hf.SnapshotGramOperator(X)
        r_out = k - 48
        dp = [double_pass_once(ctx, op, Z, r_out) for _ in range(args.runs)]
        i = int(np.argsort([d[0] for d in dp])[len(dp) // 2])
        rec.update({"double_pass_r": r_out, "double_pass_snapshots": k + 64, "double_pass_ms": round(dp[i][0], 3),
                    "double_pass_ms_runs": [round(d[0], 3) for d in dp],
                    "double_pass_phases_ms": {n: round(v, 3) for n, v in dp[i][1].items() if v > 0.0},
                    "d_first": dp[i][2], "d_last": dp[i][3]})
        print(json.dumps(rec), flush=True)
        doc["points"].append(rec)
        del op, X, Z
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
