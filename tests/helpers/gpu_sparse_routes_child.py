"""Child of tests/test_gpu_sparse_routes.py: under the environment it was started with, solves M^-1 B for the 1-D P1 mass matrix of
tests/test_gpu_kernels.py::_fem (N = 1500) at k = 6 and k = 84 with the tolerances of test_sparse_solver_chebyshev_and_cg_routes, runs
one V-cycle of CsrAMGSolver (nx = 64, k = 6: its smoother takes the same step plan) against tests/helpers/amg_vcycle_twin.py, and
prints one JSON line: the figures of every case, the method the solver reports, and the step plans the process's own knobs give."""
import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import hippyflow_amd as hf                           # noqa: E402
from hippyflow_amd import _lib as L                  # noqa: E402
from hippyflow_amd import workloads                  # noqa: E402
from tests.helpers import amg_vcycle_twin as vtwin   # noqa: E402
from tests.helpers import spsolve_rules_twin as tw   # noqa: E402

N, NX = 1500, 64


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def mass(n):
    h = 1.0 / (n - 1)
    main = np.full(n, 4 * h / 6)
    main[[0, -1]] = 2 * h / 6
    return sp.diags([np.full(n - 1, h / 6), main, np.full(n - 1, h / 6)], [-1, 0, 1], format="csr")


def step_plan(nrows, k, resid):
    """(wave, rows per wave, workgroups) of a Chebyshev step under the process's own knobs"""
    words = (C.c_int64 * tw.WORDS)()
    L.call("hfmi_cheb_rules_predict", 0.5, 2.0, 1e-13, 500, nrows, k, resid, None, 0, None, words)
    return [words[tw.WAVE], words[tw.UNR], words[tw.GRID]], list(words[tw.KNOB0:tw.KNOB0 + 3])


def run_mass(k, M, lu):
    rng = np.random.default_rng(k)
    X = rng.standard_normal((N, k)) * np.exp(rng.standard_normal(k))[None, :]        # columns of very different size
    X[:, k // 2] = 0.0                                                               # and a zero right-hand side
    Z = hf.MultiVector(N, k)
    solver = hf.CsrPCGSolver(M, rel_tol=1e-13)
    solver.matMvMult(hf.MultiVector.from_dense(X), Z)
    Zd = Z.to_dense()
    res = np.linalg.norm(M @ Zd - X, axis=0)
    f = dict(method=solver.info()["method"], iterations=solver.info()["iterations"],
             worst_residual=float(np.max(res / np.maximum(np.linalg.norm(X, axis=0), 1e-300))),
             zero_column_nonzero=bool(Zd[:, k // 2].any()), rel_lu=float(rel(Zd, lu.solve(X))))
    ok = bool(np.all(res <= 2e-13 * np.linalg.norm(X, axis=0) + 1e-300)) and not f["zero_column_nonzero"] and f["rel_lu"] < 1e-11
    return f, ok


def run_vcycle(k):
    A = (workloads.grid_mass_matrix(NX, NX) + 0.1 * workloads.grid_stiffness_matrix(NX, NX)).tocsr()
    S = hf.CsrAMGSolver(A, rel_tol=1e-12)
    B = np.random.default_rng(k).standard_normal((A.shape[0], k))
    X = hf.MultiVector(A.shape[0], k)
    S.vcycle(hf.MultiVector.from_dense(B), X)
    f = dict(levels=len(S.hierarchy().levels), rel_twin=float(rel(X.to_dense(), vtwin.vcycle(S.hierarchy(), B))))
    return f, f["rel_twin"] <= 1e-12 and f["levels"] >= 3


def main():
    if hf.device_count() < 1:
        print(json.dumps({"error": "no GPU visible"}))
        return 2
    out = {"cases": {}, "plans": {}, "failed": []}
    M = mass(N)
    lu = spla.splu(M.tocsc())
    for name, (f, ok) in (("mass 6", run_mass(6, M, lu)), ("mass 84", run_mass(84, M, lu)), ("vcycle 6", run_vcycle(6))):
        out["cases"][name] = f
        if not ok:
            out["failed"].append(name)
    for k in (6, 84):
        out["plans"]["step %d" % k], out["knobs"] = step_plan(N, k, 0)
        out["plans"]["resid %d" % k], _ = step_plan(N, k, 1)
    print(json.dumps(out))
    return 1 if out["failed"] else 0


if __name__ == "__main__":
    sys.exit(main())
