"""GPU suite: the environment-only A/B routes of the sparse SPD solves (hippyflow_amd/csrc/hfmi_spsolve_rules.h).  The default routes
are walked by tests/test_gpu_kernels.py and tests/test_gpu_amg.py; the switches below select kernels nothing else runs.  The
environment is read once per process, so every setting gets a fresh child interpreter (tests/helpers/gpu_sparse_routes_child.py): one
after another, each under its own time limit, and none is started after one that exits non-zero.  A child solves with the mass matrix
at k = 6 and k = 84 (tolerances of test_sparse_solver_chebyshev_and_cg_routes) and runs one V-cycle against its numpy twin."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("HFMI_PCG", "HFMI_CHEB_THREADMAP", "HFMI_CHEB_UNR")
# (environment, method the solver must report, knobs the process must have read, [wave, rows per wave] of a step at k = 6 and k = 84)
SETTINGS = [
    ({"HFMI_PCG": "1"}, "cg", [1, 0, 1], [1, 1]),
    ({"HFMI_CHEB_THREADMAP": "1"}, "chebyshev", [0, 1, 1], [0, 1]),
    ({"HFMI_CHEB_UNR": "2"}, "chebyshev", [0, 0, 2], [1, 2]),
    ({"HFMI_CHEB_UNR": "4"}, "chebyshev", [0, 0, 4], [1, 4]),
]


def test_environment_only_routes_match_the_references():
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    script = os.path.join(ROOT, "tests", "helpers", "gpu_sparse_routes_child.py")
    for env, method, knobs, step in SETTINGS:
        r = subprocess.run([sys.executable, script], env=dict(base, **env), capture_output=True, text=True, timeout=120, cwd=ROOT)
        lines = r.stdout.strip().splitlines()
        print(env, lines[-1] if lines else r.stderr[-2000:])
        assert r.returncode == 0, "%s: exit %d\n%s\n%s" % (env, r.returncode, lines[-1] if lines else "", r.stderr[-2000:])
        out = json.loads(lines[-1])
        assert not out["failed"] and sorted(out["cases"]) == ["mass 6", "mass 84", "vcycle 6"], env
        assert out["knobs"] == knobs, env
        for k in (6, 84):
            assert out["cases"]["mass %d" % k]["method"] == method, env
            assert out["plans"]["step %d" % k][:2] == step, env                   # the kernel the setting is there to select
            assert out["plans"]["resid %d" % k][:2] == [step[0], 1], env          # the residual launch never unrolls
