"""CPU suite: the launch plan of the whole-GPU symmetric eigensolver (hippyflow_amd/csrc/hfmi_eig_plan.h, run by sym_eig_large of
hfmi_eig_blocked.hip) through ``hfmi_eig_plan_predict`` -- the planner and the tridiagonalisation walk the driver itself runs,
without a device.  The sweep covers EVERY n from 3 to 16384 (about 3 s; not the sampled fallback), with the LDS figures of an
MI355X: 163840 bytes per workgroup, 4108 bytes of static LDS in the deflation kernel.  The invariants are those a launch needs to
be in bounds (tests/helpers/eig_plan_check.py: workspace regions, partial sums against what each kernel instance reads, LDS
against the device and the raised attribute); the literal values are those the code and the documents state; the knob cases run
in child interpreters, because the switches are read once per process."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import eig_blocked_twin as twin
from tests.helpers import eig_plan_check as ck

ROOT = ck.ROOT

ALL_SIZES = list(range(3, 16385))


@pytest.fixture(scope="module")
def sweep():
    """the plan of every n, computed once"""
    for name in os.environ:
        assert not name.startswith("HFMI_EIG_"), "the sweep wants the default knobs, %s is set" % name
    return ck.predict(ALL_SIZES)


def plan(sweep, n):
    return tuple(a[n - 3] for a in sweep)


def test_every_plan_keeps_the_launch_invariants(sweep):
    S = sweep[0]
    assert (S[:, ck.ROUTE] == 1).all()
    ck.check_invariants(ALL_SIZES, *sweep)


def test_leaf_level_is_the_twins(sweep):
    assert (sweep[0][:, ck.LF] == [min(twin.leaf_level(n, 128), 7) for n in ALL_SIZES]).all()


def test_n_below_3_takes_the_jacobi_route():
    S, R, V, W = ck.predict([1, 2])
    assert (S == 0).all() and (R == 0).all() and (V == 0).all() and (W == 0).all()


def test_literal_values_of_code_and_documents(sweep):
    S = sweep[0]
    at = lambda n, q: int(S[n - 3, q])      # noqa: E731
    # the +144 pad of a power-of-two leading dimension
    assert (at(4096, ck.LD), at(8192, ck.LD), at(16384, ck.LD)) == (4240, 8336, 16528)
    assert (at(4095, ck.LD), at(4097, ck.LD), at(2048, ck.LD), at(8064, ck.LD)) == (4240, 4224, 2048, 8064)
    # 512-wide block reflectors from n = 2048 on
    assert (at(2047, ck.WY), at(2048, ck.WY)) == (256, 512)
    # the top merge: MODE 0 up to cap = 4160 (n = 4159), MODE 1 up to n = 9919 (9984 poles x 16 + 4108 bytes = 163852 > 163840), MODE 2 beyond
    top = sweep[2][:, 0, :]
    assert [int(top[n - 3, 1]) for n in (4096, 4159, 4160, 9919, 9920, 16384)] == [0, 0, 1, 1, 2, 2]
    assert (int(top[9919 - 3, 0]), int(top[9920 - 3, 0])) == (9920, 9984)
    assert int(top[9920 - 3, 2]) == 0 and int(top[9919 - 3, 2]) == 9920 * 16
    # n = 16384: the <..., 32> instances only, 256 partial norms for k_tri_b<8, 32> and up to 129 for k_tri_bs<32>
    W = sweep[3][16384 - 3]
    launched = [i for i in range(ck.TRI_B_4_8, ck.TRI_BS_32 + 1) if W[i, ck.LAUNCHES]]
    assert launched == [ck.TRI_B_8_32, ck.TRI_BS_32]
    assert (int(W[ck.TRI_B_8_32, ck.NPN]), int(W[ck.TRI_BS_32, ck.NPN])) == (256, 129)
    assert int(W[ck.TRI_B_8_32, ck.LDS]) == 131072 == at(16384, ck.TRI_B_ATTR)
    assert at(16384, ck.MAX_NTILES) == 2080 and at(16384, ck.MAX_NB) == 64
    # 4096 < n <= 8192: CB = 16, the attribute raised to nr x 8 bytes; below: CB = 8, no attribute
    for n, insts, attr in ((8192, [ck.TRI_B_8_16, ck.TRI_BS_16], 65536), (4097, [ck.TRI_B_8_16, ck.TRI_BS_16], 4224 * 8),
                           (4096, [ck.TRI_B_8_8, ck.TRI_BS_8], 0), (2049, [ck.TRI_B_8_8], 0)):
        Wn = sweep[3][n - 3]
        assert [i for i in range(ck.TRI_B_4_8, ck.TRI_BS_32 + 1) if Wn[i, ck.LAUNCHES]] == insts, n
        assert at(n, ck.TRI_B_ATTR) == attr, n
    # n <= 2048: the unblocked tail from column 0, no panel column; beyond, the tail starts at the first panel boundary with <= 2048 rows
    small = S[:2048 - 2]
    assert (small[:, ck.J_UNB] == 0).all() and (small[:, ck.PANEL_COLS] == 0).all() and (small[:, ck.PANEL_ENDS] == 0).all()
    assert (at(2049, ck.J_UNB), at(4300, ck.J_UNB), at(16384, ck.J_UNB)) == (64, 2304, 14336)
    # the k_tri_u ladder: 512 / 1024 / 2048 rows of LDS vectors
    for n, rung in ((512, ck.TRI_U_4), (513, ck.TRI_U_8), (1024, ck.TRI_U_8), (1025, ck.TRI_U_16), (2048, ck.TRI_U_16)):
        Wn = sweep[3][n - 3]
        assert max(i for i in range(ck.TRI_U_4, ck.TRI_U_20 + 1) if Wn[i, ck.LAUNCHES]) == rung, n
    # the default knobs, as clamped
    assert S[0, ck.SYM_MIN:ck.LEAF_MAX + 1].tolist() == [3072, 2048, 128]
    # the lower-triangle products start at 3072 rows of trailing block
    assert not sweep[3][3072 - 3][ck.TRI_BS_8, ck.LAUNCHES] and sweep[3][3073 - 3][ck.TRI_BS_8, ck.LAUNCHES] == 1


def test_nvec_changes_nothing_of_the_plan(sweep):
    for n in (300, 4300, 9920):
        for a, b in zip(ck.predict([n], nvec=64), plan(sweep, n)):
            assert (a[0] == b).all()


# the plan's switches among the settings of tests/test_gpu_eig_blocked.py::test_sym_eig_blocked_ab_knobs_give_the_same_spectrum
# (HFMI_XFER_* and HFMI_EIG_GEMM belong to other units)
KNOB_CASES = [{"HFMI_EIG_SYM_MIN": "0"}, {"HFMI_EIG_SYM_MIN": "1024"}, {"HFMI_EIG_LEAF": "64"}, {"HFMI_EIG_TRI_UNR": "4"},
              {"HFMI_EIG_UNB_MAX": "0"}, {"HFMI_EIG_UNB_MAX": "700"}, {"HFMI_EIG_WY": "256"}, {"HFMI_EIG_WY": "512"},
              {"HFMI_EIG_FULL_UPDATE": "1"}, {"HFMI_EIG_NO_LD_PAD": "1"}, {"HFMI_EIG_LARGE": "jacobi"}, {}]


@pytest.fixture(scope="module")
def knob_facts():
    """one child interpreter per setting, all started at once: each checks the invariants on ck.knob_sizes() and prints its facts"""
    script = os.path.join(ROOT, "tests", "helpers", "eig_plan_check.py")
    base = {k: v for k, v in os.environ.items() if not k.startswith("HFMI_EIG_")}
    procs = [subprocess.Popen([sys.executable, script], env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              cwd=ROOT) for env in KNOB_CASES]
    out = {}
    for env, p in zip(KNOB_CASES, procs):
        stdout, stderr = p.communicate(timeout=120)
        assert p.returncode == 0, "%s: %s" % (env, stderr[-2000:])
        out[json.dumps(env, sort_keys=True)] = json.loads(stdout.strip().splitlines()[-1])
    return out


def knob(knob_facts, **env):
    return knob_facts[json.dumps(env, sort_keys=True)]


def test_knob_cases(knob_facts):
    default = knob(knob_facts)
    d4300 = default["at"]["4300"]
    assert default["any_bs"] and default["any_tail_column"] and default["any_lower_update"] and default["any_mirror"]
    assert default["jacobi_max"] == 0 and default["max_leaf_rows"] <= 128 and not default["ld_is_nr"]
    assert d4300["launches"][ck.TRI_BS_16] == 4300 - 1 - 3072 + 1 and d4300["WY"] == 512 and d4300["Lf"] == 6

    f = knob(knob_facts, HFMI_EIG_SYM_MIN="0")       # never the lower-triangle products: nothing to cut, nothing to mirror
    assert not f["any_bs"] and not f["any_lower_update"] and not f["any_mirror"] and f["at"]["4300"]["knobs"][0] == 1 << 30
    f = knob(knob_facts, HFMI_EIG_SYM_MIN="1024")    # ... from 1024 rows on: every panel column of n = 4300 (the tail takes the last 2048)
    assert f["at"]["4300"]["knobs"][0] == 1024 and f["at"]["4300"]["launches"][ck.TRI_BS_16] == 2304 and f["at"]["4300"]["launches"][ck.TRI_B_8_16] == 0
    f = knob(knob_facts, HFMI_EIG_LEAF="64")
    assert f["max_leaf_rows"] <= 64 and f["at"]["4300"]["Lf"] == 7 and f["at"]["300"]["Lf"] == 3 and f["at"]["4300"]["knobs"][2] == 64
    f = knob(knob_facts, HFMI_EIG_TRI_UNR="4")       # n <= 4096 only: beyond, the <8, CB> instances
    assert f["at"]["4096"]["launches"][ck.TRI_B_4_8] > 0 and f["at"]["4096"]["launches"][ck.TRI_B_8_8] == 0
    assert f["at"]["4300"]["launches"] == d4300["launches"]
    f = knob(knob_facts, HFMI_EIG_UNB_MAX="0")       # no tail column anywhere: the panels run to n - 2 and k_tri_tail closes
    assert not f["any_tail_column"] and all(r["j_unb"] == -1 and r["tails"] == 1 for r in f["at"].values())
    f = knob(knob_facts, HFMI_EIG_UNB_MAX="700")     # the first panel boundary with at most 700 rows left
    assert f["at"]["4300"]["j_unb"] == 3648 and f["at"]["300"]["j_unb"] == 0 and f["at"]["4300"]["knobs"][1] == 700
    assert knob(knob_facts, HFMI_EIG_WY="256")["at"]["4300"]["WY"] == 256
    assert knob(knob_facts, HFMI_EIG_WY="512")["at"]["300"]["WY"] == 512
    f = knob(knob_facts, HFMI_EIG_FULL_UPDATE="1")   # every update over the full block: nothing to mirror
    assert f["any_bs"] and not f["any_lower_update"] and not f["any_mirror"]
    f = knob(knob_facts, HFMI_EIG_NO_LD_PAD="1")
    assert f["ld_is_nr"] and f["at"]["4096"]["ld"] == 4096 and f["at"]["8192"]["ld"] == 8192
    f = knob(knob_facts, HFMI_EIG_LARGE="jacobi")    # up to n = 4096
    assert f["jacobi_max"] == 4096 and f["at"]["4096"]["route"] == 0 and f["at"]["4097"]["route"] == 1 and f["at"]["4300"] == d4300
