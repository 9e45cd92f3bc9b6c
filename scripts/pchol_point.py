"""Time of the pivoted Cholesky factor of a kernel covariance (hf.pivoted_cholesky, hfmi_pchol.hip) and of the KLE taken from it, on 2-D
scattered points, Matern-3/2, ell = 0.1, diagonal mass matrix.  Per point (N, max_rank): wall-clock seconds of the factorisation (it ends
in a device synchronise), the bytes the algorithm needs -- 4 N k^2, every earlier column read once per step -- over that time as a fraction
of the 8 TB/s HBM peak, and the time of ``eig(64, M)``.  At the first point only, the matrix-free randomized KLE (doublePassG, r = 64,
p = 20) runs on the same points beside it (the probe draw is inside its time), and both residuals ||M C M V - M V d||_F / ||M C M V||_F
are evaluated with the matrix-free operator.  Every time is the median of --runs repetitions after a warm-up of both routes at N = 8192;
the double pass has one more untimed run at its own size first (the mass solve estimates its spectrum in its first solve).  Writes one
JSON document.
    python scripts/pchol_point.py [--points 100000:256,1000000:256,1000000:1024] [--runs 3] [--out profiles/pchol_point.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hippyflow_amd as hf  # noqa: E402

HBM_PEAK = 8.0e12
FAMILY, SIGMA, ELL, R, P = "matern32", 1.0, 0.1, 64, 20


def wall(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ctx.synchronize()
    return time.perf_counter() - t0, out


def residual(C, M, mdiag, d, V):
    """||M C M V - M V d||_F / ||M C M V||_F with C applied matrix-free"""
    MV, CMV = hf.MultiVector(V), hf.MultiVector(V)
    hf.MatMvMult(M, V, MV)
    C.matMvMult(MV, CMV)
    A = mdiag[:, None] * CMV.to_dense()
    return float(np.linalg.norm(A - MV.to_dense() * np.asarray(d)[None, :]) / np.linalg.norm(A))


def run_double_pass(ctx, C, M, N, solver=None):
    """the matrix-free randomized KLE on (C, M): doublePassG, r = R, p = P, one pass, the same probe block every time"""
    hf.parRandom.reseed(1)
    Omega = hf.MultiVector(N, R + P, ctx=ctx)
    hf.parRandom.normal(1.0, Omega)
    A = hf.MassPreconditionedCovarianceOperator(C, M)
    return hf.doublePassG(A, M, solver or hf.CsrPCGSolver(M.csr, ctx=ctx), Omega, R, s=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="100000:256,1000000:256,1000000:1024")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "pchol_point.json"))
    args = ap.parse_args()
    ctx = hf.Context.default()
    points = [tuple(int(x) for x in p.split(":")) for p in args.points.split(",")]
    # warm-up at a small size: both routes once, with the timed r and p (code objects of every kernel either route launches)
    wN = 8192
    wrng = np.random.default_rng(0)
    wpts, wM = wrng.random((wN, 2)), hf.CsrOperator(sp.diags((0.5 + wrng.random(wN)) / wN).tocsr(), ctx=ctx)
    wC = hf.KernelCovarianceOperator(wpts, family=FAMILY, sigma=SIGMA, ell=ELL, ctx=ctx)
    hf.pivoted_cholesky(wC, 300).eig(R, wM)
    run_double_pass(ctx, wC, wM, wN)
    del wC, wM
    doc = {"device": ctx.device_info(), "build_tag": hf.build_tag(), "family": FAMILY, "sigma": SIGMA, "ell": ELL, "d": 2,
           "hbm_peak_bytes_per_s": HBM_PEAK, "points": []}
    for i, (N, k) in enumerate(points):
        rng = np.random.default_rng(N)
        pts = rng.random((N, 2))
        mdiag = (0.5 + rng.random(N)) / N
        M = hf.CsrOperator(sp.diags(mdiag).tocsr(), ctx=ctx)
        C = hf.KernelCovarianceOperator(pts, family=FAMILY, sigma=SIGMA, ell=ELL, ctx=ctx)
        times, f = [], None
        for _ in range(args.runs):
            f = None                                    # one factor (8 N k bytes) at a time
            t, f = wall(ctx, lambda: hf.pivoted_cholesky(C, k))
            times.append(t)
        t_f = float(np.median(times))
        nbytes = 4.0 * N * f.rank ** 2
        eig_times = []
        for _ in range(args.runs):
            d = V = MV = None                           # one result (and one M L inside eig) at a time
            t, (d, V, MV) = wall(ctx, lambda: f.eig(R, M))
            eig_times.append(t)
        t_eig = float(np.median(eig_times))
        rec = {"N": N, "max_rank": k, "rank": f.rank, "stop_reason": f.stop_reason, "factor_s": round(t_f, 4),
               "factor_s_runs": [round(t, 4) for t in times], "algorithm_bytes": nbytes,
               "fraction_of_hbm_peak": round(nbytes / t_f / HBM_PEAK, 4), "steps_per_s": round(f.rank / t_f, 1),
               "eig_r": R, "eig_s": round(t_eig, 4), "eig_s_runs": [round(t, 4) for t in eig_times], "relative_residual_trace": float(f.residual_trace / f.trace[0]),
               "eigenvalue_error_bound": f.eigenvalue_error_bound(M), "d_first": float(d[0]), "d_last": float(d[-1])}
        if i == 0:
            rec["factor_kle_residual"] = residual(C, M, mdiag, d, V)
            solver = hf.CsrPCGSolver(M.csr, ctx=ctx)
            run_double_pass(ctx, C, M, N, solver)       # untimed: this solver's spectrum estimate, this size's workspaces
            dp_times = []
            for _ in range(args.runs):
                t, (d2, U2) = wall(ctx, lambda: run_double_pass(ctx, C, M, N, solver))
                dp_times.append(t)
            t_dp = float(np.median(dp_times))
            rec.update({"double_pass_s": round(t_dp, 4), "double_pass_s_runs": [round(t, 4) for t in dp_times], "double_pass_oversampling": P, "double_pass_kle_residual": residual(C, M, mdiag, d2, U2),
                        "double_pass_d_first": float(d2[0]), "double_pass_d_last": float(d2[-1]),
                        "max_d_difference_over_d0": float(np.abs(np.asarray(d2) - d).max() / d[0])})
        print(json.dumps(rec), flush=True)
        doc["points"].append(rec)
        del f, V, MV, C, M
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
