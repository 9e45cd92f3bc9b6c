"""doublePass[G] against singlePass[G] per solve on the single-GPU shapes of configs 4, 3 and 2 (as bench.py builds them):
median wall time of --runs solves after --warmup, operator applications per solve, the leading-eigenvalue relative error of
each method against the exact spectrum where the workload has one, and the largest principal angle between the two
subspaces (leading 10 and all r vectors; B-inner product for the generalized problem).  One JSON line per config.
    python scripts/single_pass_time.py [--configs 4,3,2] [--runs 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import workloads  # noqa: E402


def build(config):
    """(op, B, Binv, host B or None, N, r, p, exact eigenvalues or None, description) as bench.py's build_workload"""
    if config == 4:
        N, ns, q, r, p = 500 * 400, 512, 100, 64, 10
        wl = workloads.as_workload(N, ns, q=q, latent=q, rate=0.06, seed=4, first_sample=0, ns_total=ns, noise=0.01)
        return wl, wl.operator, None, None, None, N, r, p, None, "config4 mean J^T J, %d x (%d x %d), noise 0.01" % (ns, q, N)
    if config == 3:
        N, n, r, p = 500000, 2048, 128, 10
        wl = workloads.pod_workload(N, n, latent=256, rate=0.05, seed=3)
        return wl, wl.operator, None, None, None, N, r, p, wl.exact_eigenvalues, "config3 snapshot Gram, %d x N=%d" % (n, N)
    nx, ny, N, r, p = 316, 317, 100000, 64, 20
    wl = workloads.kle_matern_workload(nx, ny, N=N, sigma=1.0, ell=0.1)
    op = hf.MassPreconditionedCovarianceOperator(wl.C_operator, wl.M_operator)
    return (wl, op, wl.M_operator, hf.CsrPCGSolver(wl.M_operator.csr), wl.M, N, r, p, None,
            "config2 M C M u = lambda M u, dense Matern-3/2 C, N=%d" % N)


def max_angle(U1, U2, Bh=None):
    """largest principal angle between range(U1) and range(U2), both (B-)orthonormal"""
    C = U1.T @ (U2 if Bh is None else Bh @ U2)
    s = np.linalg.svd(C, compute_uv=False)
    return float(np.arccos(np.clip(s.min(), -1.0, 1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4,3,2")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for config in [int(c) for c in args.configs.split(",")]:
        wl, op, B, Binv, Bh, N, r, p, exact, desc = build(config)
        Omega = hf.MultiVector(N, r + p)
        hf.parRandom.reseed(1)
        hf.parRandom.normal(1.0, Omega)
        out = {"config": config, "workload": desc, "N": N, "rank": r, "oversampling": p, "s": 1}
        res = {}
        for name, fn in (("double_pass", hf.doublePassG if B else hf.doublePass), ("single_pass", hf.singlePassG if B else hf.singlePass)):
            call = (lambda fn=fn: fn(op, B, Binv, Omega, r, s=1)) if B else (lambda fn=fn: fn(op, Omega, r, s=1))
            for _ in range(args.warmup):
                d, U = call()
            ts = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                d, U = call()
                ts.append(1e3 * (time.perf_counter() - t0))
            res[name] = (d, U.to_dense())
            out[name] = {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "runs": len(ts),
                         "operator_applications": 2 if name == "double_pass" else 1,
                         "leading_eig_rel_err": (float(abs(d[0] - exact[0]) / exact[0]) if exact is not None else None),
                         "leading10_eig_max_rel_err": (float(np.max(np.abs(d[:10] - exact[:10]) / exact[:10])) if exact is not None else None)}
        (d1, U1), (d2, U2) = res["double_pass"], res["single_pass"]
        out["single_vs_double"] = {"eig_rel_diff_leading10": float(np.max(np.abs(d2[:10] - d1[:10]) / np.abs(d1[:10]))),
                                   "eig_rel_diff_all": float(np.max(np.abs(d2 - d1)) / abs(d1[0])),
                                   "max_principal_angle_leading10_rad": max_angle(U1[:, :10], U2[:, :10], Bh),
                                   "max_principal_angle_all_rad": max_angle(U1, U2, Bh)}
        out["speedup"] = out["double_pass"]["ms_median"] / out["single_pass"]["ms_median"]
        print(json.dumps(out), flush=True)
        del wl, op, res, U1, U2


if __name__ == "__main__":
    main()
