"""The bi-Laplacian prior solve R^-1 = A^-1 M_l A^-1 on the device (BiLaplacianRsolver: AMG-preconditioned CG,
hfmi_amg.hip) against the host sparse-LU pool (workloads.SparseLUPriorSolver), in one job.  One JSON line per measurement:

  shard      config 4's prior-preconditioned shard as bench.py --prior builds it (64 samples, N = 2e5, k = 74,
             doublePassG(J^T J, R, R^-1)): ms per step (median of --runs after --warmup), the apply_Binv phase (separate
             profiled step), A-solve iterations, hierarchy setup seconds; device and host Rsolver in the same process
  a_solve    one A-solve at k = 74 and one V-cycle: ms (median), iterations, and achieved bytes/s from the algorithmic
             bytes of the hierarchy (nnz, rows, N k) against 8 TB/s
  kle        KLEProjector on an implicit bi-Laplacian prior at config 2's size (N ~ 1e5, r = 64, p = 20, orthogonality
             'mass'; no dense C), device against host Rsolver

    python scripts/amg_prior_time.py [--runs 5] [--warmup 1] [--host-workers 16] [--only shard,a_solve,kle] [--out FILE]
Kernel times: run it once more under rocprofv3 --kernel-trace --stats with --only a_solve."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hippyflow_amd as hf  # noqa: E402
from hippyflow_amd import workloads  # noqa: E402

HBM_PEAK = 8.0e12


def vcycle_bytes(h, k):
    """Algorithmic bytes of one V-cycle on k vectors: every pass over an n x k array once, every sparse matrix (8-byte value,
    4-byte index) once per product.  Per smoothed level: Chebyshev degree d before and after (first step from zero: 3
    arrays; every other step: b, x, x_prev read, x written), residual (3 arrays + A), restriction (res read, coarse b written
    + R), prolongation (coarse x read, x read and written + P); coarsest level: the dense inverse and 2 arrays."""
    total = 0.0
    d = h.degree
    for lv, nxt in zip(h.levels, h.levels[1:]):
        n, nc, zA = lv.A.shape[0], nxt.A.shape[0], lv.A.nnz
        arrays = (3 + 4 * (d - 1)) + 3 + 1 + 2 + 4 * d
        total += 8.0 * k * (arrays * n + 2 * nc)
        total += 12.0 * zA * (2 * d) + 12.0 * (lv.R.nnz + lv.P.nnz)
    nL = h.levels[-1].A.shape[0]
    return total + 8.0 * nL * nL + 16.0 * nL * k


def solve_bytes(h, k, iterations):
    """A-solve: per CG iteration one V-cycle, A p (p read, Ap written + A), two dots (4 arrays), the x / r update (4 read, 2
    written), the direction (3 arrays); once: two transposes, the first V-cycle and the true residual (3 arrays + A)."""
    n, zA = h.levels[0].A.shape[0], h.levels[0].A.nnz
    per_it = vcycle_bytes(h, k) + 8.0 * k * n * (2 + 4 + 6 + 3) + 12.0 * zA
    once = vcycle_bytes(h, k) + 8.0 * k * n * (4 + 3 + 2) + 12.0 * zA
    return iterations * per_it + once


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    hf.Context.default().synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        hf.Context.default().synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), len(ts)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def shard(args):
    nx, ny, q, ns, r, p = 500, 400, 100, 64, 64, 10
    N, k = nx * ny, r + p
    wl = workloads.as_workload(N, ns, q=q, latent=q, rate=0.06, seed=4, first_sample=0, ns_total=512, noise=0.01)
    t0 = time.perf_counter()
    prior = workloads.BiLaplacianPrior(nx, ny, delta=1.0, gamma=0.1, processes=args.host_workers)
    host_setup = time.perf_counter() - t0
    B = hf.CsrOperator(prior.R)
    t0 = time.perf_counter()
    Rdev = hf.BiLaplacianRsolver(prior.A, prior.M_lumped)
    dev_setup = time.perf_counter() - t0
    Rhost = hf.HostCallbackOperator(prior.Rsolver, N, chunk_vectors=(0 if args.host_workers > 8 else None))
    hf.parRandom.reseed(1)
    Omega = hf.MultiVector(N, k)
    hf.parRandom.normal(1.0, Omega)
    ctx = hf.Context.default()
    rec = {"measurement": "shard", "workload": "config4 prior-preconditioned shard: doublePassG(mean J^T J, R, R^-1), %d samples "
           "x (%d x %d), r=%d, p=%d, R = A M_l^-1 A, A = M + 0.1 K on %d x %d" % (ns, q, N, r, p, nx, ny), "N": N, "k": k,
           "hierarchy": Rdev.Asolver.hierarchy().info(), "device_setup_s": dev_setup,
           "host_setup_s": host_setup, "host_workers": prior.Rsolver.processes}
    out = {}
    for name, Binv in (("device", Rdev), ("host", Rhost)):
        med, mn, n = timed(lambda: hf.doublePassG(wl.operator, B, Binv, Omega, r, s=1), args.runs, args.warmup)
        ctx.profile_begin()
        d, U = hf.doublePassG(wl.operator, B, Binv, Omega, r, s=1)
        ctx.profile_end()
        ph = ctx.profile_phases()
        out[name] = d
        rec[name] = {"ms_per_step_median": med, "ms_per_step_min": mn, "runs": n,
                     "phases_ms": {kk: v for kk, v in ph.items() if v > 0}}
    rec["device"]["amg_iterations_last_solve"] = Rdev.info()["iterations"]
    rec["eig_rel_diff_device_vs_host"] = float(np.abs(out["device"] - out["host"]).max() / np.abs(out["host"]).max())
    rec["speedup_host_over_device"] = rec["host"]["ms_per_step_median"] / rec["device"]["ms_per_step_median"]
    prior.Rsolver.close()
    emit(rec, args.out)


def a_solve(args):
    nx, ny, k = 500, 400, 74
    A = (workloads.grid_mass_matrix(nx, ny) + 0.1 * workloads.grid_stiffness_matrix(nx, ny)).tocsr()
    N = A.shape[0]
    t0 = time.perf_counter()
    S = hf.CsrAMGSolver(A, rel_tol=1e-12)
    setup = time.perf_counter() - t0
    h = S.hierarchy()
    Bh = np.random.default_rng(0).standard_normal((N, k))
    Bm, X = hf.MultiVector.from_dense(Bh), hf.MultiVector(N, k)
    med, mn, n = timed(lambda: S.matMvMult(Bm, X), args.runs, args.warmup)
    its = S.info()["iterations"]
    res = float((np.linalg.norm(Bh - A @ X.to_dense(), axis=0) / np.linalg.norm(Bh, axis=0)).max())
    vmed, vmn, vn = timed(lambda: S.vcycle(Bm, X), args.runs * 4, args.warmup)
    sb, vb = solve_bytes(h, k, its), vcycle_bytes(h, k)
    emit({"measurement": "a_solve", "matrix": "A = M + 0.1 K, %d x %d P1 grid" % (nx, ny), "N": N, "k": k, "setup_s": setup,
          "hierarchy": h.info(), "solve_ms_median": med, "solve_ms_min": mn, "iterations": its, "max_rel_residual": res,
          "solve_algorithmic_bytes": sb, "solve_achieved_TBps": sb / (mn * 1e-3) / 1e12,
          "solve_share_of_8TBps": sb / (mn * 1e-3) / HBM_PEAK,
          "vcycle_ms_median": vmed, "vcycle_ms_min": vmn, "vcycle_algorithmic_bytes": vb,
          "vcycle_achieved_TBps": vb / (vmn * 1e-3) / 1e12, "vcycle_share_of_8TBps": vb / (vmn * 1e-3) / HBM_PEAK}, args.out)


def kle(args):
    nx, ny, r, p = 316, 317, 64, 20
    params = hf.KLEParameterList()
    params['rank'], params['oversampling'], params['verbose'], params['save_and_plot'] = r, p, False, False
    rec = {"measurement": "kle", "workload": "KLEProjector.construct_input_subspace('mass'), implicit bi-Laplacian prior "
           "C = A^-1 M_l A^-1 on %d x %d (no dense C), r=%d, p=%d" % (nx, ny, r, p), "N": nx * ny}
    d = {}
    for name in ("device", "host"):
        t0 = time.perf_counter()
        prior = workloads.BiLaplacianPrior(nx, ny, processes=args.host_workers, rsolver=name)
        rec[name + "_setup_s"] = time.perf_counter() - t0
        kp = hf.KLEProjector(prior, parameters=params)

        def run():
            hf.parRandom.reseed(3)
            d[name] = kp.construct_input_subspace('mass')[0]
        med, mn, n = timed(run, max(2, args.runs // 2), args.warmup)
        rec[name] = {"ms_median": med, "ms_min": mn, "runs": n}
        if name == "host":
            prior.Rsolver.close()
    rec["eig_rel_diff_device_vs_host"] = float(np.abs(d["device"] - d["host"]).max() / np.abs(d["host"]).max())
    rec["speedup_host_over_device"] = rec["host"]["ms_median"] / rec["device"]["ms_median"]
    emit(rec, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-workers", type=int, default=16)
    ap.add_argument("--only", default="shard,a_solve,kle")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    if hf.device_count() < 1:
        raise SystemExit("amg_prior_time.py needs a GPU")
    for what in args.only.split(","):
        {"shard": shard, "a_solve": a_solve, "kle": kle}[what](args)


if __name__ == "__main__":
    main()
