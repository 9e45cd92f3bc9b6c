"""CPU suite: the launch plans of the one-compute-unit k x k stage (hippyflow_amd/csrc/hfmi_small_plan.h) through
``hfmi_small_plan_predict`` -- the planners the seven launchers themselves ask, without a device.  Every k from 1 to 256, the four
kinds, both eigh methods, the default knobs and every A/B setting one at a time are compared word for word with the if-chains the
planners replaced (tests/helpers/small_plan_twin.py); on the same sweep, the conditions each kernel's indexing needs to stay in
bounds; the literal values the code comments and the documents state; and, in child interpreters (the environment is read once
per process), how the switches are clamped and that a tuning key, once set, counts before its environment value."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import pytest

from hippyflow_amd import _lib as L
from tests.helpers import small_plan_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 163840          # of a workgroup on gfx950
ALL_K = range(1, 257)
CALLS = [(tw.CHOL, 0), (tw.EIGH, 0), (tw.EIGH, 1), (tw.SVD, 0), (tw.LU, 0)]
SETTINGS = [{}, {"chol_key": 1}, {"chol_key": 1, "chol_generic": 1}, {"chol_key": 1, "chol_tile": 0}, {"eig_key": 1}, {"jacobi_db": 0},
            {"jacobi_db": 2}, {"jacobi_replay_lds": 1}, {"tri_waves": 4}, {"dc_split_top": 0}, {"small_threads": 256},
            {"small_threads": 512}]

tw.chol_tiles = functools.lru_cache(maxsize=None)(tw.chol_tiles)      # the twin's count is O(k^2) and asked for again by every setting


def predict(kind, k, method, kn):
    words = (C.c_int64 * tw.PLAN_WORDS)()
    L.call("hfmi_small_plan_predict", kind, k, method, (C.c_int * tw.KNOB_WORDS)(*tw.knob_words(kn)), words)
    return list(words)


@pytest.fixture(scope="module")
def sweep():
    """{(setting index, kind, method, k): record}, computed once"""
    out = {}
    for s, setting in enumerate(SETTINGS):
        kn = tw.knobs(**setting)
        for kind, method in CALLS:
            for k in ALL_K:
                out[s, kind, method, k] = predict(kind, k, method, kn)
    return out


def launches(w):
    return [w[tw.LAUNCH0 + tw.LAUNCH_WORDS * i:tw.LAUNCH0 + tw.LAUNCH_WORDS * (i + 1)] for i in range(w[tw.NLAUNCH])]


def regions(w):
    return [tuple(w[tw.REGION0 + 2 * i:tw.REGION0 + 2 * i + 2]) for i in range(w[tw.NREGIONS])]


def test_every_plan_is_the_parents(sweep):
    for (s, kind, method, k), w in sweep.items():
        assert w == tw.parent_plan(kind, k, method, tw.knobs(**SETTINGS[s])), (SETTINGS[s], kind, method, k)


def test_every_plan_keeps_its_kernels_in_bounds(sweep):
    seen = set()
    for (s, kind, method, k), w in sweep.items():
        where = (SETTINGS[s], kind, method, k)
        if w[tw.REFUSE]:
            assert w[tw.NLAUNCH] == 0 and w[tw.WS_BYTES] == 0, where
            continue
        assert 1 <= w[tw.NLAUNCH] <= tw.MAX_LAUNCHES, where
        for fam, t0, t1, t2, t3, threads, grid, lds, raised in launches(w):
            seen.add(fam)
            assert 64 <= threads <= 1024 and threads % 64 == 0 and grid >= 1, where
            # a workgroup has 160 KB of LDS; without the attribute a kernel gets 64 KB of dynamic LDS
            assert 0 <= lds <= LDS_BYTES and (raised or lds <= 65536), where
            if fam == tw.SF_CHOL_MFMA:
                # wave w keeps block pair q = w + NW t of the nb (nb + 1) / 2 pairs in acc[t], t < SLOTS: a pair beyond is never factored
                nb = (k + 15) // 16
                assert threads == 64 * t0 and t0 * t1 >= nb * (nb + 1) // 2, where
                # scratch: 32 + 5 x 256 doubles of tables, CM_SCR per wave, the double-buffered block row of nb blocks
                assert lds == (32 + 5 * 256 + t0 * tw.CM_SCR + 2 * nb * 256) * 8, where
            elif fam == tw.SF_CHOL_REG:
                # entry e of the triangle sits in register e / 512 of thread e % 512: v[EPT] must reach the last entry
                assert threads == 512 and 512 * t0 >= k * (k + 1) // 2, where
                assert k <= 139 and lds >= (32 + 4 * 256 + k * (k | 1)) * 8, where      # the factor's copy: k rows of k | 1 doubles of LDS
            elif fam in (tw.SF_CHOL_TILE, tw.SF_CHOL_BIG):
                # thread tid owns the tid-th TR x TC rectangle that touches the upper triangle: a rectangle beyond the threads has no owner
                assert tw.chol_tiles(k, t0, t1) <= threads == (512 if fam == tw.SF_CHOL_TILE else 1024), where
                if fam == tw.SF_CHOL_TILE:
                    assert k <= 139 and lds >= (32 + 4 * 256 + k * (k | 1)) * 8, where  # Ml: k rows of k | 1 doubles behind the tables
                else:
                    assert lds >= (32 + 4 * 256) * 8, where                             # the tables only: the copy is in the global slot
            elif fam == tw.SF_CHOL_INV:
                assert lds >= (32 + 3 * 256 + (k * (k | 1) if w[tw.USE_LDS] else 0)) * 8 and (w[tw.USE_LDS] or k > 139), where
            elif fam == tw.SF_JACOBI_EIG:
                n = w[tw.N_EVEN]
                cells = ((n // 2 + 1) >> 1) * (n // 2 + 1)
                # thread tid rotates the 2 x 2 blocks tid + threads bi, bi < NB, of the folded triangle: a cell beyond is never rotated
                assert threads * t0 >= cells, where
                assert t1 == w[tw.USE_LDS] and lds >= (32 + 256 + 256 + (n * n if t1 else 0)) * 8, where   # S in LDS: n x n doubles
            elif fam == tw.SF_JACOBI_EIG_DB:
                n = w[tw.N_EVEN]
                np_ = n // 2
                cells = ((np_ + 1) >> 1) * (np_ + 1)
                # the first 128 threads compute the next round's rotations; the other threads - 128 update NB cells each
                assert threads >= 256 and (threads - 128) * t0 >= cells and np_ <= 128, where
                assert lds >= (32 + 512 + 256 + 8 * (np_ * (np_ + 1) // 2)) * 8, where  # two images of the 2 x 2 blocks of the triangle
            elif fam == tw.SF_JACOBI_SVD:
                assert t0 == w[tw.USE_LDS] and lds >= (32 + 256 + 132 + (k * (k | 1) if t0 else 0)) * 8, where
            elif fam == tw.SF_JACOBI_VECTORS_WAVE:
                # one wave per row, the row in rowbuf[4][130]: n <= 128; four rows per workgroup
                assert w[tw.N_EVEN] <= 128 and threads == 256 and grid * 4 >= k, where
            elif fam == tw.SF_JACOBI_VECTORS:
                assert threads == 128 and grid == k, where                             # one workgroup per row, row[2][SM_MAXK + 2]
            elif fam == tw.SF_TRIDIAG:
                # row r on wave r mod NW in register r / NW < RI, the last LR rows in LDS; column c on lane c mod 64 in register c / 64 < CJ
                assert threads == 64 * t2 and t2 * t0 + t3 >= k and 64 * t1 >= k, where
                assert lds == t3 * 64 * t1 * 8, where                                   # s_dyn[LR][64 CJ]
            elif fam == tw.SF_DC:
                assert threads == 1024 and t0 == (8 if k <= 128 else 4), where
            elif fam == tw.SF_DC_TOP:
                assert grid == ((k + 15) // 16) ** 2 + 16 and threads == 64 and w[tw.SPLIT_TOP], where
            elif fam == tw.SF_DC_BACK:
                # 16 lanes per eigenvector, z[EL] entries each; four eigenvectors per one-wave workgroup
                assert 16 * t0 >= k and threads == 64 and grid * 4 >= k, where
            elif fam == tw.SF_LU:
                nb = w[tw.NB]
                # the panel: m rows of nb | 1 doubles behind the bookkeeping, 64 bytes of static LDS beside it
                assert 1 <= nb <= k and (nb == k or nb % 16 == 0) and lds == tw.LU_BOOK_BYTES + k * (nb | 1) * 8 <= LDS_BYTES - 64, where
            else:
                raise AssertionError("family %d of %s" % (fam, where))
        # the workspace: regions back to back in layout order, disjoint, inside the allocation, each aligned to its element
        end = 0
        R = regions(w)
        for offset, nbytes in R:
            assert offset >= end and nbytes > 0, where
            end = offset + nbytes
        assert end <= w[tw.WS_BYTES], where
        if kind == tw.EIGH and not w[tw.ROUTE]:
            ldq = w[tw.LDQ]
            assert ldq % 16 == 0 and k <= ldq < k + 16 and (1 << w[tw.LEVELS]) >= k, where
            want = [256 * 8] * 3 + [256 * ldq * 8] + [ldq * ldq * 8] * 3 + [256 * 4, 16 * 4, 16 * 8, (3 * 256 + 16) * 4]
            assert [b for _, b in R] == want, where
            assert all(off % 8 == 0 for off, _ in R[:7]) and R[9][0] % 8 == 0 and all(off % 4 == 0 for off, _ in R), where
        elif kind in (tw.EIGH, tw.SVD):
            n = w[tw.N_EVEN]
            rounds = (40 if kind == tw.EIGH else 41) * (n - 1)       # one (c, s) pair of 16 bytes per pivot; the SVD logs a sweep more
            assert [b for _, b in R] == [rounds * (n // 2) * 16, 1024 * 4] and R[0][0] % 16 == 0 and R[1][0] % 4 == 0, where
        else:
            assert R == [] and w[tw.WS_BYTES] == 0, where
    assert seen == set(range(1, 16))     # the settings reach every kernel family


def test_refusals(sweep):
    for kind, method in CALLS:
        for k in (-1, 0, 257, 1000):
            w = predict(kind, k, method, tw.knobs())
            assert w[tw.REFUSE] == tw.REFUSE_RANGE and not any(w[1:tw.KNOB0]), (kind, k)
    # Jacobi with fewer threads: 9 blocks per thread hold 2304 cells of the folded triangle at 256 threads -- np = 66 (k = 132) has
    # 33 x 67 = 2211 of them, np = 67 (k = 133) has 34 x 68 = 2312 and needs a tenth -- and 4608 at 512: np = 95 (k = 190) has 48 x 96
    expect = {}
    for threads, first_literal in ((256, 133), (512, 191)):
        s = SETTINGS.index({"small_threads": threads})
        refused = [k for k in ALL_K if sweep[s, tw.EIGH, 1, k][tw.REFUSE]]
        first = min(k for k in ALL_K if (((k + 1) // 2 + 1) >> 1) * ((k + 1) // 2 + 1) > 9 * threads)
        assert refused == list(range(first, 257)) and first == first_literal
        assert all(sweep[s, tw.EIGH, 1, k][tw.REFUSE] == tw.REFUSE_INSTANCE and sweep[s, tw.EIGH, 1, k][tw.NB] >= 10 for k in refused)
        expect[s] = first
    # nothing else is ever refused
    assert all(not w[tw.REFUSE] for (s, kind, method, k), w in sweep.items() if not (s in expect and kind == tw.EIGH and method == 1))
    with pytest.raises(RuntimeError):
        predict(7, 10, 0, tw.knobs())


def test_literal_values_of_code_and_documents(sweep):
    lu = lambda m: sweep[0, tw.LU, 0, m][tw.NB]      # noqa: E731
    assert lu(138) == 138 and lu(141) == 141 and lu(142) < 142 and lu(256) == 64
    col = SETTINGS.index({"chol_key": 1})
    assert [sweep[col, tw.CHOL, 0, k][tw.USE_LDS] for k in (139, 140)] == [1, 0]                   # the column Cholesky: LDS up to k = 139
    assert [launches(sweep[col, tw.CHOL, 0, k])[0][0] for k in (7, 8, 139, 140, 256)] == \
        [tw.SF_CHOL_REG, tw.SF_CHOL_TILE, tw.SF_CHOL_TILE, tw.SF_CHOL_BIG, tw.SF_CHOL_BIG]
    assert launches(sweep[col, tw.CHOL, 0, 256])[0][1:3] == [6, 6]                                 # 6 x 6 per thread at k = 256
    assert [sweep[0, tw.EIGH, 1, k][tw.USE_LDS] for k in (137, 138, 139)] == [1, 1, 0]             # the Jacobi matrix: LDS up to n = 138
    assert launches(sweep[0, tw.EIGH, 1, 138])[0][0] == tw.SF_JACOBI_EIG_DB and launches(sweep[0, tw.EIGH, 1, 74])[0][0] == tw.SF_JACOBI_EIG
    assert [launches(sweep[0, tw.EIGH, 1, k])[1][0] for k in (128, 129)] == [tw.SF_JACOBI_VECTORS_WAVE, tw.SF_JACOBI_VECTORS]
    assert [sweep[0, tw.SVD, 0, k][tw.USE_LDS] for k in (139, 140)] == [1, 0]
    assert launches(sweep[0, tw.CHOL, 0, 256])[0][:3] == [tw.SF_CHOL_MFMA, 8, 17]                  # k_chol_mfma<8, 17> at k = 256
    assert [launches(sweep[0, tw.CHOL, 0, k])[0][2] for k in (80, 81, 112, 113, 144, 145, 192, 193)] == [2, 4, 4, 6, 6, 10, 10, 17]
    tri = lambda k, s=0: launches(sweep[s, tw.EIGH, 0, k])[0]      # noqa: E731
    assert tri(160)[1:5] == [20, 3, 8, 0] and tri(160)[7:] == [0, 0]                               # LDS rows from k = 161
    assert tri(161)[1:5] == [20, 3, 8, 32] and tri(161)[7:] == [32 * 192 * 8, 1]
    assert tri(256)[1:5] == [24, 4, 8, 64] and tri(256)[7:] == [131072, 1]                         # 128 KB for LR = 64
    assert tri(256, SETTINGS.index({"tri_waves": 4}))[1:6] == [64, 4, 4, 0, 256]
    assert [sweep[0, tw.EIGH, 0, k][tw.SPLIT_TOP] for k in (31, 32)] == [0, 1]
    assert all(not sweep[SETTINGS.index({"dc_split_top": 0}), tw.EIGH, 0, k][tw.SPLIT_TOP] for k in ALL_K)
    assert [launches(sweep[0, tw.EIGH, 0, k])[-1][1] for k in (80, 81, 96, 97, 128, 129, 144, 145, 192, 193, 256)] == \
        [5, 6, 6, 8, 8, 9, 9, 12, 12, 16, 16]
    # the routes: the tuning keys and the caller's method
    assert sweep[SETTINGS.index({"eig_key": 1}), tw.EIGH, 0, 100][tw.ROUTE] == 1 and sweep[0, tw.EIGH, 0, 100][tw.ROUTE] == 0
    assert sweep[0, tw.EIGH, 1, 100][tw.ROUTE] == 1 and sweep[col, tw.CHOL, 0, 100][tw.ROUTE] == 1 and sweep[0, tw.CHOL, 0, 100][tw.ROUTE] == 0


# (environment, tuning keys set in the child after its first look)
KNOB_CASES = [({}, {}), ({"HFMI_SMALL_THREADS": "512"}, {}), ({"HFMI_SMALL_THREADS": "100"}, {}), ({"HFMI_SMALL_THREADS": "2048"}, {}),
              ({"HFMI_SMALL_THREADS": "32"}, {}), ({"HFMI_TRI_WAVES": "4"}, {}), ({"HFMI_TRI_WAVES": "5"}, {}),
              ({"HFMI_CHOL": "tile", "HFMI_CHOL_GENERIC": "1", "HFMI_CHOL_TILE": "0"}, {}), ({"HFMI_CHOL": "mfma", "HFMI_CHOL_TILE": "2"}, {}),
              ({"HFMI_EIG": "jacobi", "HFMI_JACOBI_DB": "2", "HFMI_JACOBI_REPLAY_LDS": "1"}, {}),
              ({"HFMI_EIG": "dc", "HFMI_JACOBI_DB": "0", "HFMI_JACOBI_REPLAY_LDS": "0", "HFMI_CHOL_GENERIC": ""}, {}),
              ({"HFMI_DC_SPLIT_TOP": "0", "HFMI_DC_TIMING": "1"}, {}),
              ({"HFMI_CHOL": "tile", "HFMI_EIG": "jacobi"}, {"chol": 0, "eig": 0}), ({}, {"chol": 1, "eig": 1})]
SWITCHES = ("HFMI_SMALL_THREADS", "HFMI_CHOL", "HFMI_CHOL_GENERIC", "HFMI_CHOL_TILE", "HFMI_JACOBI_DB", "HFMI_JACOBI_REPLAY_LDS", "HFMI_EIG",
            "HFMI_TRI_WAVES", "HFMI_DC_SPLIT_TOP", "HFMI_DC_TIMING", "HFMI_TUNE")


def test_knobs_are_read_and_clamped_as_before_and_a_set_key_counts_first():
    script = os.path.join(ROOT, "tests", "helpers", "small_plan_twin.py")
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    procs = [subprocess.Popen([sys.executable, script, json.dumps(keys)], env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=ROOT) for env, keys in KNOB_CASES]
    for (env, keys), p in zip(KNOB_CASES, procs):
        stdout, stderr = p.communicate(timeout=120)
        assert p.returncode == 0, "%s: %s" % (env, stderr[-2000:])
        got = json.loads(stdout.strip().splitlines()[-1])
        kn = tw.parent_env_knobs(env)
        assert got["before"] == tw.knob_words(kn), env
        assert (got["chol_route"], got["eig_route"]) == (kn["chol_env"], kn["eig_env"]), env
        kn.update(chol_key=keys.get("chol", -1), eig_key=keys.get("eig", -1))
        assert got["after"] == tw.knob_words(kn), (env, keys)
        # the environment value is read only while the key was never set
        assert got["chol_route_after"] == keys.get("chol", kn["chol_env"]) and got["eig_route_after"] == keys.get("eig", kn["eig_env"]), (env, keys)
    clamped = {json.dumps(env): tw.parent_env_knobs(env) for env, _ in KNOB_CASES}
    assert [clamped[json.dumps({"HFMI_SMALL_THREADS": v})]["small_threads"] for v in ("512", "100", "2048", "32")] == [512, 1024, 1024, 1024]
    assert [clamped[json.dumps({"HFMI_TRI_WAVES": v})]["tri_waves"] for v in ("4", "5")] == [4, 8]
