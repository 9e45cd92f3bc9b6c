"""One rank of the row-sharded kernel covariance test (started by hippyflow_amd.launch.spawn_ranks; the ranks share the GPU).  Every
rank saves its shard, the sharded apply next to the full apply it computes itself, and the 'mass' KLE with and without sharding; one more
point with more ranks than rows covers an empty shard."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


class _Prior:
    pass


def main():
    outdir = sys.argv[1]
    import hippyflow_amd as hf
    from hippyflow_amd import workloads
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    coll = hf.NativeCollective.from_env()
    ctx = hf.Context.default()
    res = {"size": coll.size(), "rank": coll.rank(), "transport": coll.transport}

    N, d, k = 333, 2, 12
    pts = np.random.default_rng(17).random((N, d))
    C = hf.KernelCovarianceOperator(pts, family="matern32", sigma=1.3, ell=0.3, nugget=0.05, ctx=ctx)
    Cs = C.sharded(coll)
    res["rows"] = np.array([Cs.row0, Cs.row1])
    W = hf.MultiVector.from_dense(np.random.default_rng(3).standard_normal((N, k)), ctx=ctx)
    Yf, Ys = hf.MultiVector(N, k, ctx=ctx), hf.MultiVector(N, k, ctx=ctx)
    C.matMvMult(W, Yf)
    Cs.matMvMult(W, Ys)
    res["Y_full"], res["Y_sharded"] = Yf.to_dense(), Ys.to_dense()
    try:
        Cs.matMvMult(W, Ys, accumulate=True)
        res["accumulate"] = "no error"
    except hf.HfmiError as exc:
        res["accumulate"] = str(exc)

    # the 'mass' KLE: same probe block (shared stream re-seeded), sharding off and on
    M = (workloads.grid_mass_matrix(19, 18)[:N, :N]).tocsr()
    for name, flag in (("off", False), ("on", True)):
        prior = _Prior()
        prior.M, prior.C = M, C
        params = hf.KLEParameterList()
        params["rank"], params["oversampling"], params["verbose"], params["save_and_plot"] = 8, 4, False, False
        hf.parRandom.reseed(7)
        kle = hf.KLEProjector(prior, collective=coll, parameters=params, ctx=ctx)
        kle.shard_kernel_covariance = flag
        dd, dec, enc = kle.construct_input_subspace("mass")
        res["d_" + name], res["dec_" + name], res["enc_" + name] = np.asarray(dd), dec.to_dense(), enc.to_dense()

    # more ranks than rows: the last shard is empty
    N2 = 2
    pts2 = np.random.default_rng(5).random((N2, d))
    C2 = hf.KernelCovarianceOperator(pts2, family="matern52", sigma=1.0, ell=0.5, nugget=0.1, ctx=ctx)
    Cs2 = C2.sharded(coll)
    res["rows2"] = np.array([Cs2.row0, Cs2.row1])
    W2 = hf.MultiVector.from_dense(np.random.default_rng(6).standard_normal((N2, 3)), ctx=ctx)
    Yf2, Ys2 = hf.MultiVector(N2, 3, ctx=ctx), hf.MultiVector(N2, 3, ctx=ctx)
    C2.matMvMult(W2, Yf2)
    Cs2.matMvMult(W2, Ys2)
    res["Y2_full"], res["Y2_sharded"] = Yf2.to_dense(), Ys2.to_dense()

    coll.barrier()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    coll.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
