"""GPU suite: the environment-only A/B routes of the one-compute-unit k x k stage (hippyflow_amd/csrc/hfmi_small_plan.h).  The
default routes, tuning "chol" = 1 and method="jacobi" are walked at every ladder boundary by tests/test_gpu_kernels.py; the
switches below select kernels nothing else runs.  The environment is read once per process, so every setting gets a fresh child
interpreter (tests/helpers/gpu_small_routes_child.py): one after another, each under its own time limit, and none is started after
one that exits non-zero.  A child runs the routes its setting touches -- MultiVector.orthogonalize on a graded (4k + 64) x k block,
sym_eig_small(method="jacobi"), sym_eig_small(method="dc") -- and checks each result against numpy with the tolerances of
test_blocked_cholesky_against_lapack_and_the_column_kernel and test_sym_eig_small_matches_eigh.

HFMI_SMALL_THREADS gets no GPU run: it is a workgroup-shape experiment knob; tests/test_small_plan_cpu.py covers its plans and
its refusals."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import small_plan_twin as tw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("HFMI_SMALL_THREADS", "HFMI_CHOL", "HFMI_CHOL_GENERIC", "HFMI_CHOL_TILE", "HFMI_JACOBI_DB", "HFMI_JACOBI_REPLAY_LDS", "HFMI_EIG",
            "HFMI_TRI_WAVES", "HFMI_DC_SPLIT_TOP", "HFMI_DC_TIMING", "HFMI_TUNE")
# (environment, routes, (case, family the plan must name for it): the kernel the setting is there to select)
SETTINGS = [
    ({"HFMI_CHOL": "tile", "HFMI_CHOL_GENERIC": "1"}, ["chol"], [("chol 74", tw.SF_CHOL_INV), ("chol 200", tw.SF_CHOL_INV)]),
    ({"HFMI_CHOL": "tile", "HFMI_CHOL_TILE": "0"}, ["chol"], [("chol 74", tw.SF_CHOL_REG), ("chol 139", tw.SF_CHOL_REG), ("chol 140", tw.SF_CHOL_BIG)]),
    ({"HFMI_JACOBI_DB": "0"}, ["jacobi"], [("jacobi 138", tw.SF_JACOBI_EIG), ("jacobi 74", tw.SF_JACOBI_EIG)]),
    ({"HFMI_JACOBI_DB": "2"}, ["jacobi"], [("jacobi 30", tw.SF_JACOBI_EIG_DB), ("jacobi 74", tw.SF_JACOBI_EIG_DB), ("jacobi 140", tw.SF_JACOBI_EIG)]),
    ({"HFMI_JACOBI_REPLAY_LDS": "1"}, ["jacobi"], [("jacobi 30", tw.SF_JACOBI_VECTORS), ("jacobi 74", tw.SF_JACOBI_VECTORS)]),
    ({"HFMI_TRI_WAVES": "4"}, ["dc"], [("dc 31", tw.SF_TRIDIAG), ("dc 225", tw.SF_TRIDIAG)]),
    ({"HFMI_DC_SPLIT_TOP": "0"}, ["dc"], [("dc 33", tw.SF_DC_BACK), ("dc 225", tw.SF_DC_BACK)]),
]


def test_environment_only_routes_match_numpy():
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    script = os.path.join(ROOT, "tests", "helpers", "gpu_small_routes_child.py")
    for env, routes, selected in SETTINGS:
        r = subprocess.run([sys.executable, script] + routes, env=dict(base, **env), capture_output=True, text=True, timeout=120, cwd=ROOT)
        lines = r.stdout.strip().splitlines()
        print(env, lines[-1] if lines else r.stderr[-2000:])
        assert r.returncode == 0, "%s: exit %d\n%s\n%s" % (env, r.returncode, lines[-1] if lines else "", r.stderr[-2000:])
        out = json.loads(lines[-1])
        assert not out["failed"] and len(out["cases"]) == sum({"chol": 6, "jacobi": 4, "dc": 5}[x] for x in routes), env
        for case, family in selected:
            fams, params = out["plans"][case]
            assert family in fams, (env, case, fams)
        if env.get("HFMI_TRI_WAVES") == "4":
            assert all(p[0][2] == 4 for p in (out["plans"][c][1] for c in out["plans"])), env       # k_tridiag<RI, CJ, 4>
        if env.get("HFMI_DC_SPLIT_TOP") == "0":
            assert all(tw.SF_DC_TOP not in out["plans"][c][0] for c in out["plans"]), env
