"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol include/hfmi.h
declares (no compute calls without a GPU), the product path fails loudly without a GPU, and the host-side mirror
of the reference interface keeps the reference's parameter names and defaults."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hfmi_[a-z0-9_]+)\s*\(", text)))


# what the finished library defines in its dynamic symbol table besides the declared entry points: nothing (the export list
# hippyflow_amd/libhfmi.map keeps even the toolchain's __hip_cuid_<hash> markers local); a toolchain symbol that a later
# linker adds goes here by its exact prefix
TOOLCHAIN_SYMBOL_PREFIXES = ()


def _defined_dynamic_symbols(lib_path):
    """names the library DEFINES in its dynamic symbol table (binutils nm, or llvm-readelf of the ROCm toolchain)"""
    import shutil
    import subprocess
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", lib_path], check=True, stdout=subprocess.PIPE, text=True).stdout
        return sorted(line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip())
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    readelf = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "llvm-readelf")
    out = subprocess.run([readelf, "--dyn-syms", "-W", lib_path], check=True, stdout=subprocess.PIPE, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    return sorted(r[7].split("@")[0] for r in rows if len(r) >= 8 and r[0].rstrip(":").isdigit() and r[6] != "UND")


def test_library_exports_every_declared_symbol():
    lib_path = os.path.join(ROOT, "hippyflow_amd", "libhfmi.so")
    if not os.path.exists(lib_path):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(lib_path)
    declared = _declared_symbols()
    assert len(declared) >= 45
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    from hippyflow_amd import _lib
    bound = set(_lib.SIGNATURES) | set(_lib.NON_STATUS)
    assert bound == set(declared), (bound ^ set(declared))
    lib.hfmi_version.restype = ctypes.c_int
    assert lib.hfmi_version() == 100
    # ... and exports nothing else: no launcher, helper, kernel handle or template instantiation (no C++-mangled name at all)
    defined = _defined_dynamic_symbols(lib_path)
    assert set(declared) <= set(defined), sorted(set(declared) - set(defined))
    extra = [s for s in defined if s not in set(declared) and not s.startswith(TOOLCHAIN_SYMBOL_PREFIXES)]
    assert not extra, "%d undeclared symbols exported, e.g. %s" % (len(extra), extra[:8])
    assert not [s for s in defined if s.startswith("_Z")]


def test_no_cpu_fallback():
    import hippyflow_amd as hf
    if hf.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(hf.HfmiError) as e:
        hf.Context(0)
    assert "no HIP device" in str(e.value)
    with pytest.raises(hf.HfmiError):
        hf.MultiVector(10, 2)            # every compute object needs a context: no silent numpy path
    # nothing under hippyflow_amd/ may import the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, "hippyflow_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_parameter_lists_match_reference_defaults(golden_dir):
    import hippyflow_amd as hf
    want = json.load(open(os.path.join(golden_dir, "parameter_defaults.json")))
    for name in ("ActiveSubspaceParameterList", "PODParameterList", "KLEParameterList"):
        pl = getattr(hf, name)()
        assert set(pl.keys()) == set(want[name].keys()), name
        for key, val in want[name].items():
            got = pl[key]
            if isinstance(val, str) and not isinstance(got, str):
                got = repr(got)
            assert got == val, (name, key, got, val)
    pl = hf.PODParameterList()
    pl["rank"] = 7
    assert pl["rank"] == 7
    with pytest.raises(ValueError):
        pl["no_such_key"]


def test_null_collective_semantics(golden_dir):
    import hippyflow_amd as hf
    g = np.load(os.path.join(golden_dir, "collectives.npz"))
    nc = hf.NullCollective()
    assert nc.size() == int(g["null_size"]) and nc.rank() == int(g["null_rank"])
    v = g["parts"][0, :, 0].copy()
    assert nc.allReduce(v, "AVG") is v and nc.bcast(v) is v
    np.testing.assert_array_equal(v, g["null_allreduce"])
    with pytest.raises(NotImplementedError):
        nc.allReduce(v, "max")


def test_grid_mass_matrix_is_a_p1_mass_matrix():
    from hippyflow_amd import workloads
    M = workloads.grid_mass_matrix(7, 5)
    assert M.shape == (35, 35) and abs(M.sum() - 1.0) < 1e-14          # integrates 1 over the unit square
    assert (M != M.T).nnz == 0 and M.getnnz(axis=1).max() <= 7
    assert np.linalg.eigvalsh(M.toarray()).min() > 0


def test_bilaplacian_prior_and_host_lu_solver():
    """The synthetic prior of config 4: R = A M_l^-1 A is SPD, the host LU black box inverts it through both the
    reference's 1-D ``solve(y, x)`` protocol and the block form the pipelined callback uses; the stiffness matrix has the
    constants in its null space."""
    from hippyflow_amd import workloads
    prior = workloads.BiLaplacianPrior(24, 17, delta=1.0, gamma=0.1)
    N = 24 * 17
    assert prior.R.shape == (N, N) and abs(prior.R - prior.R.T).max() < 1e-12
    assert abs(prior.K @ np.ones(N)).max() < 1e-12 and abs(prior.M.sum() - 1.0) < 1e-13
    assert np.linalg.eigvalsh(prior.R.toarray()).min() > 0
    X = np.random.default_rng(0).standard_normal((N, 5))
    Y = prior.Rsolver.solve_block(X)
    np.testing.assert_allclose(prior.R @ Y, X, rtol=1e-8, atol=1e-9)
    y = np.zeros(N)
    prior.Rsolver.solve(y, X[:, 2])
    np.testing.assert_allclose(y, Y[:, 2], rtol=1e-12)
    threaded = workloads.SparseLUPriorSolver(prior.A, prior.M_lumped, threads=3)
    np.testing.assert_allclose(threaded.solve_block(X), Y, rtol=1e-12)


def test_matern_host_kernel_is_a_covariance():
    from hippyflow_amd import workloads
    C = workloads.matern32_host(60, 10, 8, sigma=2.0, ell=0.3)
    assert C.shape == (60, 60) and np.allclose(np.diag(C), 4.0) and abs(C - C.T).max() == 0
    assert np.linalg.eigvalsh(C).min() > 0
    rows = workloads.matern32_host(60, 10, 8, sigma=2.0, ell=0.3, rows=[3, 17])
    np.testing.assert_array_equal(rows, C[[3, 17]])


def test_build_tag_matches_the_sources():
    import hippyflow_amd as hf
    from hippyflow_amd import _build
    assert hf.build_tag() == _build.source_tag()          # the library in the tree was built from the sources in the tree
    tr = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    assert set(tr) >= {"build_tag", "source", "kernels"}


def test_prior_solver_process_pool_equals_in_process_solver():
    """The host R^-1 black box of the prior-preconditioned AS solve (prior.Rsolver, activeSubspaceProjector.py:447-453)
    dealt to worker PROCESSES with their own factorisation (slabs through shared memory) gives the in-process result bit
    for bit, and leaves nothing behind in /dev/shm."""
    import os
    from hippyflow_amd import workloads
    before = set(os.listdir("/dev/shm")) if os.path.isdir("/dev/shm") else set()
    one = workloads.BiLaplacianPrior(40, 30)
    pool = workloads.BiLaplacianPrior(40, 30, processes=3)
    X = np.random.default_rng(0).standard_normal((1200, 7))
    np.testing.assert_array_equal(pool.Rsolver.solve_block(X), one.Rsolver.solve_block(X))
    np.testing.assert_array_equal(pool.Rsolver.solve_block(X[:, :2]), one.Rsolver.solve_block(X[:, :2]))     # fewer vectors than workers
    y = np.zeros(1200)
    pool.Rsolver.solve(y, X[:, 3])
    np.testing.assert_array_equal(y, one.Rsolver.solve_block(X[:, 3:4])[:, 0])
    big = np.random.default_rng(1).standard_normal((1200, 40))                                                # grows the segments
    np.testing.assert_array_equal(pool.Rsolver.solve_block(big), one.Rsolver.solve_block(big))
    pool.Rsolver.close()
    if os.path.isdir("/dev/shm"):
        assert set(os.listdir("/dev/shm")) <= before


def test_spectrum_plot_is_optional_cosmetics(tmp_path):
    """utilities/plotting.py:18-50: eigenvalues above 1e-10 on a logarithmic axis, saved where the caller says; without matplotlib
    the call is a no-op (the arrays are what matters)."""
    import numpy as np
    import hippyflow_amd as hf
    out = os.path.join(str(tmp_path), "spectrum.pdf")
    fig = hf.spectrum_plot(np.array([1.0, 1e-3, 1e-6, 1e-12, 0.0, -1.0]), axis_label=["i", r"$\lambda_i$", r"Eigenvalues of $C$"], out_name=out)
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert fig is None and not os.path.exists(out)
        return
    assert fig is not None and os.path.getsize(out) > 1000
    assert len(fig.axes[0].lines[0].get_ydata()) == 3              # the entries <= 1e-10 are dropped, as in the reference


def test_rank_and_device_follow_the_mpi_launchers_too(monkeypatch):
    """mpirun / srun set neither $RANK nor $LOCAL_RANK (advisor r4): the private Philox key and the default device fall back to the
    launchers' own variables, and a collective built later over a sub-group does not re-key the generator."""
    from hippyflow_amd import _lib as L
    from hippyflow_amd.randomized import _ParRandom
    for name in L._RANK_VARS + L._LOCAL_RANK_VARS:
        monkeypatch.delenv(name, raising=False)
    assert L.launcher_rank() == 0 and L.launcher_local_rank() == 0
    monkeypatch.setenv("OMPI_COMM_WORLD_RANK", "5")
    monkeypatch.setenv("OMPI_COMM_WORLD_LOCAL_RANK", "1")
    assert L.launcher_rank() == 5 and L.launcher_local_rank() == 1
    assert _ParRandom().rank == 5
    monkeypatch.setenv("SLURM_PROCID", "9")                   # the earlier name in the list wins
    assert L.launcher_rank() == 5
    monkeypatch.delenv("OMPI_COMM_WORLD_RANK")
    assert L.launcher_rank() == 9
    monkeypatch.setenv("RANK", "2")                           # torchrun's name first
    assert L.launcher_rank() == 2
    g = _ParRandom(rank=0)
    g.split(3, by_collective=True)                            # world / sample-parallel communicator
    g.split(0, by_collective=True)                            # a sub-group collective built later: ignored
    assert g.rank == 3
    k3 = g.key(False)
    g.split(1)                                                # an explicit split always applies
    assert g.rank == 1 and g.key(False) != k3 and g.key(True) == _ParRandom(rank=7).key(True)
    g.split(6, by_collective=True)                            # ... and is final: a collective constructed later leaves it alone
    assert g.rank == 1
    h = _ParRandom(rank=0)
    h.split(4)                                                # explicit first, collective second: the explicit key stays
    h.split(2, by_collective=True)
    assert h.rank == 4
