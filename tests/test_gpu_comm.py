"""GPU tests of the native communicator (include/hfmi.h "communicator"): RCCL transport with a one-rank group
(all a one-GPU box can offer: RCCL refuses two ranks on one device) and the p2p transport with 2 and 4 ranks sharing
the GPU, both through the same C entry points the multi-GPU run uses."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import contraction_plan_twin as twin  # noqa: E402
WORKER = os.path.join(ROOT, "tests", "helpers", "gpu_comm_worker.py")
WORKER2 = os.path.join(ROOT, "tests", "helpers", "gpu_comm_worker2.py")


def test_one_rank_rccl_communicator_is_bit_transparent():
    import hippyflow_amd as hf
    from hippyflow_amd import workloads
    coll = hf.NativeCollective.from_unique_id(hf.NativeCollective.unique_id(), 1, 0)
    assert coll.size() == 1 and coll.rank() == 0 and coll.transport == "rccl"
    X = hf.MultiVector(7001, 9)
    hf.parRandom.reseed(3)
    hf.parRandom.normal(1.0, X)
    ref = X.to_dense()
    for op in ("sum", "avg"):
        assert coll.allReduce(X, op) is X
        np.testing.assert_array_equal(X.to_dense(), ref)             # ncclAllReduce over one rank: the same bits
    coll.bcast(X, root=0)
    np.testing.assert_array_equal(X.to_dense(), ref)
    assert coll.allReduce(2.0, "avg") == 2.0 and coll.allReduceMax(3.5) == 3.5
    arr = np.arange(5.0)
    assert coll.allReduce(arr, "sum") is arr
    coll.barrier()
    # the fused solve with the all-reduce enqueued natively == the solve without a collective, bit for bit
    wl = workloads.as_workload(4001, 6, q=5, latent=5, rate=0.3, seed=4)
    Omega = hf.MultiVector(4001, 8)
    hf.parRandom.normal(1.0, Omega)
    for kw in ({}, {"literal_T": True}):
        d0, U0 = hf.doublePass(wl.operator, Omega, 5, s=1, **kw)
        d1, U1 = hf.doublePass(hf.CollectiveOperator(wl.operator, coll, mpi_op="avg"), Omega, 5, s=1, **kw)
        np.testing.assert_array_equal(d0, d1)
        np.testing.assert_array_equal(U0.to_dense(), U1.to_dense())
    with pytest.raises(NotImplementedError):
        hf.doublePass(hf.CollectiveOperator(wl.operator, coll, mpi_op="max"), Omega, 5, s=1)
    coll.close()


def test_rccl_first_contact_failure_falls_back_to_p2p_by_agreement():
    """First-contact hardening: a failing ncclCommInitRank / a first all-reduce that does not deliver sends the ranks to
    the p2p transport TOGETHER, and the communicator says why (injected failures: a one-GPU box cannot produce a real one)."""
    import json
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import json, hippyflow_amd as hf, numpy as np\n"
            "c = hf.NativeCollective.from_unique_id(hf.NativeCollective.unique_id(), 1, 0)\n"
            "X = hf.MultiVector(1000, 3); hf.parRandom.normal(1.0, X); ref = X.to_dense(); c.allReduce(X, 'avg')\n"
            "assert np.array_equal(ref, X.to_dense())\n"
            "print(json.dumps(c.describe()))\n" % ROOT)
    for inject, stage in (("init", "ncclCommInitRank"), ("first", "the first ncclAllReduce")):
        env = dict(os.environ, HFMI_COMM_INJECT=inject, HFMI_COMM_TIMEOUT_S="60")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])     # (RCCL prints its banner to stdout too)
        assert d["transport"] == "p2p" and "fell back from rccl" in d["why"] and stage in d["why"]
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HFMI_RCCL_LIB="/nonexistent/librccl.so"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])     # (RCCL prints its banner to stdout too)
    assert d["transport"] == "p2p" and "librccl not usable" in d["why"] and len(d["devices"]) == 1 and d["devices"][0]


@pytest.mark.parametrize("world,sync", [(2, "host"), (2, "stream"), (4, "host"), (4, "stream"), (8, "stream")])
def test_ranks_sharing_the_gpu_p2p_transport(tmp_path, world, sync):
    """sync = "stream": the stream-ordered p2p path (arrival / completion counters in the node segment, written and polled
    by kernels: no host synchronisation inside a collective) -- what an 8-GPU run falls back to if RCCL misbehaves.  world = 8:
    the rank count of the node this is written for, here with all eight ranks on the one GPU of the box."""
    from hippyflow_amd.launch import spawn_ranks
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="60", HFMI_P2P_SYNC=sync)
    assert spawn_ranks([WORKER, str(tmp_path)], world, env=env, timeout=600) == 0
    rs = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    for rank, r in enumerate(rs):
        assert int(r["size"]) == world and int(r["rank"]) == rank
        assert str(r["transport"]) in ("p2p", "rccl")                 # rccl only where every rank has its own GPU
        if str(r["transport"]) == "p2p":
            assert str(r["p2p_sync"]) == sync
        assert float(r["sum_err"]) == 0.0                             # same summation order as the expectation
        assert float(r["avg_err"]) < 1e-15 and float(r["bcast_err"]) == 0.0 and float(r["vector_err"]) < 1e-14
        assert float(r["big_err"]) < 1e-15
        assert float(r["host_sum"]) == world * (world + 1) / 2
        np.testing.assert_array_equal(r["avg_block"], rs[0]["avg_block"])
        for name in ("gram", "literal"):
            np.testing.assert_array_equal(r["d_" + name], rs[0]["d_" + name])      # every rank holds the same result
            np.testing.assert_array_equal(r["U_" + name], rs[0]["U_" + name])
            np.testing.assert_allclose(r["d_" + name], rs[0]["d_all"], rtol=1e-11)  # == one rank over all samples
        np.testing.assert_allclose(r["d_unfused"], rs[0]["d_all"], rtol=1e-11)
    sgn = np.sign(np.sum(rs[0]["U_gram"] * rs[0]["U_all"], axis=0))
    np.testing.assert_allclose(rs[0]["U_gram"] * sgn, rs[0]["U_all"], atol=1e-9)


def test_row_panel_reduction_is_bit_identical_and_overlapped():
    """Round 3: the rank reduction of an operator application is issued panel by panel on the auxiliary stream while the rest
    of the product is computed (hfmi_op.hip panel_reduce_hook).  Same arithmetic per element: a solve with panels equals the
    solve with ONE all-reduce after the product bit for bit, and the profile shows collective work off the main stream.
    Shape: large enough for two rounds of row tiles and a small matrix too big for the LDS-resident kernel (what config 4 is)."""
    import ctypes as C
    import hippyflow_amd as hf
    from hippyflow_amd import _lib as L
    from hippyflow_amd import workloads
    coll = hf.NativeCollective.from_unique_id(hf.NativeCollective.unique_id(), 1, 0)
    N, ns, q, k, r = 270000, 16, 100, 12, 8          # two rounds of 512-row tiles on 256 CUs + a tail
    wl = workloads.as_workload(N, ns, q=q, latent=20, rate=0.2, seed=11)
    Omega = hf.MultiVector(N, k)
    hf.parRandom.reseed(5)
    hf.parRandom.normal(1.0, Omega)
    A = hf.CollectiveOperator(wl.operator, coll, mpi_op="avg")
    ctx = hf.Context.default()
    cus = ctx.device_info()["compute_units"]

    def streamed_launches():
        """the plan records (include/hfmi.h) of the streaming nn kernel since the last clear, Y = X G of the operator among them"""
        words = (C.c_int * (256 * twin.PLAN_WORDS))()
        n = C.c_int(0)
        L.call("hfmi_plan_read", ctx.handle, 256, words, C.byref(n), None)
        flat = list(words)
        recs = [twin.decode(flat[i * twin.PLAN_WORDS:(i + 1) * twin.PLAN_WORDS]) for i in range(n.value)]
        return [rec for rec in recs if rec["kind"] == "nn"]

    def applications(got, want):
        """how often the launch list `want` occurs in `got` (the solve has other streamed products, of other shapes)"""
        return sum(1 for i in range(len(got)) if got[i:i + len(want)] == want)

    def predicted(panels, halve):
        kn = twin.knobs(nn_halve_last=halve)
        return [rec for rec, _, _ in twin.nn_launches(ns * q, k, N, kn, cus, hook_panels=panels if panels > 1 else 0)]

    out = {}
    for panels in (0, 4):
        L.call("hfmi_tuning_set", b"comm_panels", panels)
        L.call("hfmi_plan_clear", ctx.handle)
        ctx.profile_begin()
        d, U = hf.doublePass(A, Omega, r, s=1)
        ctx.profile_end()
        out[panels] = (d, U.to_dense(), ctx.profile_phases())
        # the launches are the twin's row panels: whole rounds of tiles per launch, the split tail tiles with the last one
        want = predicted(panels, 0)
        assert len(want) == (1 if panels == 0 or N < 2 * cus * 512 else 2) and applications(streamed_launches(), want) >= 1, (panels, streamed_launches(), want)
    # the opt-in half-height last round (one more, smaller, panel; profiles/archive/r04i_halve_last_ab.txt): still the same bits
    L.call("hfmi_tuning_set", b"comm_panels", 4)
    L.call("hfmi_tuning_set", b"nn_halve_last", 1)
    L.call("hfmi_plan_clear", ctx.handle)
    ctx.profile_begin()
    d_h, U_h = hf.doublePass(A, Omega, r, s=1)
    ctx.profile_end()
    halved_phases = ctx.profile_phases()
    L.call("hfmi_tuning_set", b"nn_halve_last", 0)
    want = predicted(4, 1)
    assert applications(streamed_launches(), want) >= 1, (streamed_launches(), want)
    if N >= 2 * cus * 512:        # first round, the two halves of the last round at half the tile height, the split tail
        assert [rec["TT"] for rec in want] == [8, 4, 4, 8] and want[-1]["full_tiles"] == 0 and want[-1]["msplit"] > 1
    np.testing.assert_array_equal(d_h, out[4][0])
    np.testing.assert_array_equal(U_h.to_dense(), out[4][1])
    assert 0.0 < halved_phases["allreduce"] < out[4][2]["allreduce"]          # a smaller last panel is left exposed
    np.testing.assert_array_equal(out[0][0], out[4][0])
    np.testing.assert_array_equal(out[0][1], out[4][1])
    assert out[0][2]["allreduce_overlapped"] == 0.0 and out[4][2]["allreduce_overlapped"] > 0.0
    d0, U0 = hf.doublePass(wl.operator, Omega, r, s=1)               # and both equal the solve without a communicator
    np.testing.assert_array_equal(d0, out[4][0])
    np.testing.assert_array_equal(U0.to_dense(), out[4][1])
    coll.close()


def test_a_late_rank_fails_every_rank_instead_of_returning_unreduced_data(tmp_path):
    """Stream-ordered p2p: a poll that gives up (HFMI_COMM_TIMEOUT_S) skips the reduction.  The rank that gave up must see
    HFMI_ERR_COMM at its next host synchronisation, and so must the rank that arrived late: it meets the poison value the
    first rank published instead of a sequence number (hfmi_comm.hip k_p2p_signal / k_p2p_wait)."""
    import json
    from hippyflow_amd.launch import spawn_ranks
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="120", HFMI_TEST_TIMEOUT_S="1", HFMI_P2P_SYNC="stream", HFMI_TEST_LATE_S="4")
    assert spawn_ranks([WORKER2, str(tmp_path), "late"], 2, env=env, timeout=300) == 0
    for rank in (0, 1):
        r = json.load(open(os.path.join(str(tmp_path), "late_rank%d.json" % rank)))
        assert r["transport"] == "p2p" and r["p2p_sync"] == "stream"
        assert r["outcome"] == "HfmiError", (rank, r)
        assert "did not reach a collective" in r["message"] and "NOT reduced" in r["message"]


@pytest.mark.parametrize("world", [2, 4])
def test_row_panels_across_real_peers_are_bit_identical(tmp_path, world):
    """The panel hook of an operator application with REAL peers behind it (ranks sharing the GPU, stream-ordered p2p on the
    auxiliary stream): 4 panels == one all-reduce after the product, bit for bit, on every rank, and every rank holds the
    same eigenpairs."""
    from hippyflow_amd.launch import spawn_ranks
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="120", HFMI_P2P_SYNC="stream")
    assert spawn_ranks([WORKER2, str(tmp_path), "panels"], world, env=env, timeout=900) == 0
    rs = [np.load(os.path.join(str(tmp_path), "panels_rank%d.npz" % r)) for r in range(world)]
    for r in rs:
        assert str(r["transport"]) == "p2p" and str(r["p2p_sync"]) == "stream"
        np.testing.assert_array_equal(r["d0"], r["d4"])
        np.testing.assert_array_equal(r["U0"], r["U4"])
        assert float(r["overlapped0"]) == 0.0 and float(r["overlapped4"]) > 0.0
        np.testing.assert_array_equal(r["d4"], rs[0]["d4"])
        np.testing.assert_array_equal(r["U4"], rs[0]["U4"])


def test_p2p_reduction_is_bit_identical_over_200_repetitions(tmp_path):
    """Determinism soak: 4 ranks sharing the GPU, stream-ordered p2p, 200 all-reduces of the same inputs --
    every repetition and every rank ends with the bits of the first one."""
    import json
    from hippyflow_amd.launch import spawn_ranks
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="120", HFMI_P2P_SYNC="stream")
    assert spawn_ranks([WORKER2, str(tmp_path), "soak"], 4, env=env, timeout=900) == 0
    rs = [json.load(open(os.path.join(str(tmp_path), "soak_rank%d.json" % r))) for r in range(4)]
    for r in rs:
        assert r["transport"] == "p2p" and r["p2p_sync"] == "stream" and r["reps"] == 200
        assert r["same"], r["mismatches"]
        assert r["digests"] == rs[0]["digests"] and len(r["digests"]) == 4


@pytest.mark.parametrize("world,bad_rank", [(2, 1), (4, 2)])
def test_staging_buffers_grow_in_step_when_one_rank_retried_its_export(tmp_path, world, bad_rank):
    """Advisor (round 5, medium): a rank whose hipIpcGetMemHandle is retried allocates a larger staging buffer than its peers; if it kept
    THAT size as its capacity, a later collective between the agreed size and its own would send it past the growth step its peers
    enter (a hang until the time-out, or stores into a buffer being freed).  The capacity every rank compares with is the agreed size:
    all-reduces of growing sizes with the first export of ONE rank failing (injected), all complete and exact on every rank.  (With the
    old rule -- a build whose only difference is `stage_bytes = actual` -- this test fails exactly as predicted: rank 1 skips the growth
    step of the second collective and both ranks end in the 60 s time-out, profiles/r06_p2p_capacity_ab.txt.)"""
    import json
    from hippyflow_amd.launch import spawn_ranks
    env = dict(os.environ, HFMI_COMM_TIMEOUT_S="60", HFMI_P2P_SYNC="stream", HFMI_P2P_INJECT_EXPORT_FAIL=str(bad_rank))
    assert spawn_ranks([WORKER2, str(tmp_path), "grow"], world, env=env, timeout=600) == 0
    for r in range(world):
        d = json.load(open(os.path.join(str(tmp_path), "grow_rank%d.json" % r)))
        assert d["transport"] == "p2p" and max(d["max_rel_err"]) < 1e-14, d

