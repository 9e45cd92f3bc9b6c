"""One rank of the two-rank single-pass test (started by hippyflow_amd.launch.spawn_ranks; the ranks share the GPU).  Each
rank holds its shard of the samples; per rank it saves
  * singlePass over a CollectiveOperator (the rank average enqueued by the C solve), s = 1 and s = 2;
  * a StreamedSketch with the collective fed its shard in batches of varying size (one all-reduce at the end);
and rank 0 also the one-rank results over all samples."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    outdir = sys.argv[1]
    import hippyflow_amd as hf
    from hippyflow_amd import workloads
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    coll = hf.NativeCollective.from_env()
    ctx = hf.Context.default()
    res = {"size": coll.size(), "rank": rank}

    # sample-sharded J^T J operator (the generator is keyed by the global sample index); a mild decay keeps Wt well conditioned,
    # so the comparison measures the rank reduction, not round-off amplified by the solve
    N, ns_total, q, r, p = 3001, 8, 12, 6, 6          # rank(mean J^T J) = q = r + p: a full-rank sketch
    ns_local = ns_total // world
    wl = workloads.as_workload(N, ns_local, q=q, latent=q, rate=0.1, seed=4, first_sample=rank * ns_local, ns_total=ns_total, ctx=ctx)
    hf.parRandom.reseed(11)
    Omega = hf.MultiVector(N, r + p, ctx=ctx)
    hf.parRandom.normal(1.0, Omega)
    for s in (1, 2):
        d, U = hf.singlePass(hf.CollectiveOperator(wl.operator, coll, mpi_op="avg"), Omega, r, s=s)
        res["d_coll_s%d" % s], res["U_coll_s%d" % s] = d, U.to_dense()
        res["d_dp_coll_s%d" % s] = hf.doublePass(hf.CollectiveOperator(wl.operator, coll, mpi_op="avg"), Omega, r, s=s)[0]
    if rank == 0:
        wl_all = workloads.as_workload(N, ns_total, q=q, latent=q, rate=0.1, seed=4, first_sample=0, ns_total=ns_total, ctx=ctx)
        for s in (1, 2):
            d, U = hf.singlePass(wl_all.operator, Omega, r, s=s)
            res["d_all_s%d" % s], res["U_all_s%d" % s] = d, U.to_dense()
            res["d_dp_all_s%d" % s] = hf.doublePass(wl_all.operator, Omega, r, s=s)[0]

    # streamed sketch: the same snapshot set on every rank, rank i adds the rows i, i + world, ... in batches of 1, 7, 13, ...
    Ns, m, k, n = 4000, 24, 8, 90
    rng = np.random.default_rng(5)
    W0, _ = np.linalg.qr(rng.standard_normal((Ns, 40)))
    X = (rng.standard_normal((n, 40)) * np.exp(-0.12 * np.arange(40))) @ W0.T
    Om = hf.MultiVector.from_dense(np.asfortranarray(np.random.default_rng(6).standard_normal((Ns, m))), ctx=ctx)
    mine = X[rank::world]
    sk = hf.StreamedSketch(Om, kind="snapshots", collective=coll)
    i = 0
    for b in (1, 7, 13, 5, 64):
        if i >= len(mine):
            break
        sk.add(mine[i:i + b])
        i += b
    assert i >= len(mine)
    res["sketch_coll"] = sk.sketch().to_dense()
    d, U = sk.singlePass(k)
    res["d_sketch_coll"], res["U_sketch_coll"] = d, U.to_dense()
    if rank == 0:
        one = hf.StreamedSketch(Om, kind="snapshots")
        one.add(X)
        res["sketch_all"] = one.sketch().to_dense()
        d, U = one.singlePass(k)
        res["d_sketch_all"], res["U_sketch_all"] = d, U.to_dense()
        d, U = hf.singlePass(hf.SnapshotGramOperator(hf.MultiVector.from_vectors(X, ctx=ctx)), Om, k)
        res["d_stored_all"], res["U_stored_all"] = d, U.to_dense()
    coll.barrier()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    coll.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
