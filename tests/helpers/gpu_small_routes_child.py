"""Child of tests/test_gpu_small_routes.py: runs the k x k routes named on the command line ("chol", "jacobi", "dc") under the
environment it was started with, checks every result against numpy with the tolerances of
tests/test_gpu_kernels.py::test_blocked_cholesky_against_lapack_and_the_column_kernel and ::test_sym_eig_small_matches_eigh, and
prints one JSON line: the figures of every case, and the plan records that say which kernels the environment selected."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import hippyflow_amd as hf                      # noqa: E402
from hippyflow_amd import _lib as L             # noqa: E402
from tests.helpers import small_plan_twin as tw  # noqa: E402

CHOL_K = (7, 8, 74, 139, 140, 200)
JACOBI_K = (30, 74, 138, 140)
DC_K = (31, 33, 129, 161, 225)


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def families(kind, k, method=0):
    """the kernel families of the plan the process's own knobs give"""
    words = (C.c_int64 * tw.PLAN_WORDS)()
    L.call("hfmi_small_plan_predict", kind, k, method, None, words)
    return [words[tw.LAUNCH0 + tw.LAUNCH_WORDS * i] for i in range(words[tw.NLAUNCH])], \
        [list(words[tw.LAUNCH0 + tw.LAUNCH_WORDS * i + 1:tw.LAUNCH0 + tw.LAUNCH_WORDS * i + 5]) for i in range(words[tw.NLAUNCH])]


def run_chol(k):
    rng = np.random.default_rng(1000 + k)
    N = 4 * k + 64
    Z = rng.standard_normal((N, k)) * np.exp(-0.03 * np.arange(k))
    Q = hf.MultiVector.from_dense(Z)
    R = Q.orthogonalize()
    Qd = Q.to_dense()
    Qn, Rn = np.linalg.qr(Z)
    sgn = np.sign(np.diag(Rn))
    Rn, Qn = Rn * sgn[:, None], Qn * sgn
    f = dict(orth=float(np.abs(Qd.T @ Qd - np.eye(k)).max()), lower=bool(np.tril(R, -1).any()), diag_min=float(np.diag(R).min()),
             rel_R=float(rel(R, Rn)), dQ=float(np.abs(Qd - Qn).max()))
    ok = f["orth"] < 1e-14 * max(k, 8) and not f["lower"] and f["diag_min"] > 0 and f["rel_R"] < 1e-12 and f["dQ"] < 1e-11
    return f, ok


def run_eig(k, method):
    rng = np.random.default_rng(k)
    Qm = np.linalg.qr(rng.standard_normal((k, k)))[0]
    lam = np.exp(-0.25 * np.arange(k)) * np.where(np.arange(k) % 7 == 3, -1.0, 1.0)   # decaying, some negative
    T = (Qm * lam) @ Qm.T
    T = 0.5 * (T + T.T)
    d, V = hf.sym_eig_small(T, method=method)
    w = np.linalg.eigvalsh(T)[::-1]
    d_abs, _ = hf.sym_eig_small(T, sort_by_abs=True, method=method)
    f = dict(dval=float(np.max(np.abs(d - w))), scale=float(np.abs(w).max()), sorted=bool(np.all(np.diff(d) <= 0)),
             orth=float(np.linalg.norm(V.T @ V - np.eye(k))), resid=float(np.linalg.norm(T @ V - V * d)),
             abs_sorted=bool(np.all(np.diff(np.abs(d_abs)) <= 0)))
    ok = f["dval"] < 1e-14 * k * f["scale"] and f["sorted"] and f["orth"] < 1e-13 * k and f["resid"] < 1e-13 * k * f["scale"] and f["abs_sorted"]
    return f, ok


def main(routes):
    if hf.device_count() < 1:
        print(json.dumps({"error": "no GPU visible"}))
        return 2
    out = {"cases": {}, "plans": {}, "failed": []}
    for route in routes:
        ks = {"chol": CHOL_K, "jacobi": JACOBI_K, "dc": DC_K}[route]
        for k in ks:
            name = "%s %d" % (route, k)
            if route == "chol":
                out["plans"][name] = families(tw.CHOL, k)
                f, ok = run_chol(k)
            else:
                out["plans"][name] = families(tw.EIGH, k, 1 if route == "jacobi" else 0)
                f, ok = run_eig(k, route)
            out["cases"][name] = f
            if not ok:
                out["failed"].append(name)
    print(json.dumps(out))
    return 1 if out["failed"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
