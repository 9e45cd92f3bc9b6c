"""A grid kernel covariance as a PRIOR (``GridKernelPrior``) and the double pass that needs no precision (``randomized.doublePassC``) on
the device: ``sample(noise, m)`` is mean + S noise, ``R`` is absent by design, ``doublePassC`` agrees with the device's own
``doublePassG`` given R = inv(C) as a dense operator to within the numpy restatement's own differences
(tests/helpers/grid_factor_twin.py, tests/test_double_pass_c_cpu.py), and ``ActiveSubspaceProjector`` driven over the fake PDE gives the
same (d, decoder, encoder) and the same files with a kernel prior as with a prior that carries the dense R."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fake_pde as fp                             # noqa: E402
import fftcov_twin as ft                          # noqa: E402
import grid_factor_twin as tw                     # noqa: E402

hf = pytest.importorskip("hippyflow_amd")

pytestmark = pytest.mark.gpu
EPS = tw.EPS


@pytest.fixture(scope="module")
def ctx():
    if hf.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    return hf.Context.default()


@pytest.fixture(scope="module")
def references():
    """the numpy record of every doublePassC case, computed once"""
    return [tw.dpc_reference(c) for c in tw.DPC_CASES]


def grid_op(case, ctx):
    shape, spacing, family, ell = case[:4]
    spacing = tw.unit_spacing(shape) if spacing is None else spacing
    return hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.0, ell=ell, ctx=ctx)


def host_vector(values=None, n=None):
    v = hf.HostVector()
    v.init(len(values) if values is not None else n)
    if values is not None:
        v.set_local(np.asarray(values, dtype=np.float64))
    return v


# ---------------------------------------------------------------------------------------------------------------- the prior protocol
@pytest.mark.parametrize("shape,spacing,family,ell", [((33,), (0.031,), "matern12", 0.2), ((6, 5), (0.2, 0.25), "matern32", 0.3)])
def test_sample_is_the_mean_plus_the_factor_of_the_noise(ctx, shape, spacing, family, ell):
    op = hf.GridKernelCovarianceOperator(shape, spacing, family=family, sigma=1.3, ell=ell, ctx=ctx)
    N = op.shape[0]
    mean = 0.2 * np.cos(np.linspace(0.0, np.pi, N))
    prior = hf.GridKernelPrior(op, mean=mean, max_growth=3)
    Ptot = int(np.prod(prior.embedding))
    assert prior.S.shape == (N, Ptot) and prior.C is op and prior.n_clipped == 0 and prior.cov_error_bound == 0.0
    assert prior.growth == prior.sampler.growth and np.array_equal(prior.mean.get_local(), mean)
    noise, m, x = hf.HostVector(), hf.HostVector(), hf.HostVector()
    prior.init_vector(noise, "noise")
    prior.init_vector(m, 0)
    prior.init_vector(x, 1)
    assert (noise.size(), m.size(), x.size()) == (Ptot, N, N)
    hf.parRandom.reseed(5)
    hf.parRandom.normal(1.0, noise)                       # the reference's loop: parRandom.normal(1., noise); prior.sample(noise, m)
    xi = noise.get_local().copy()
    assert abs(xi.std() - 1.0) < 0.2
    prior.sample(noise, m)
    Y = hf.MultiVector(N, 1, ctx=ctx)
    prior.S.matMvMult(hf.MultiVector.from_dense(xi[:, None], ctx=ctx), Y)
    assert np.array_equal(m.get_local(), mean + Y.to_dense()[:, 0])
    prior.sample(noise, m, add_mean=False)
    assert np.array_equal(m.get_local(), Y.to_dense()[:, 0])
    root = tw.root_spectrum(shape, spacing, family, 1.3, ell, 0.0, prior.growth)
    assert np.all(np.abs(Y.to_dense() - tw.apply_S(root, shape, xi[:, None])) <= tw.column_bounds(root, xi[:, None]))
    # the precision is absent by design, and says where to go instead
    assert not hasattr(prior, "R") and not hasattr(prior, "Hlr")
    with pytest.raises(AttributeError, match="doublePassC"):
        prior.R
    # Rsolver.solve(y, x) is y = C x, on host and on device vectors
    y = host_vector(n=N)
    prior.Rsolver.solve(y, host_vector(values=mean))
    CX = hf.MultiVector(N, 1, ctx=ctx)
    op.matMvMult(hf.MultiVector.from_dense(mean[:, None], ctx=ctx), CX)
    assert np.array_equal(y.get_local(), CX.to_dense()[:, 0])
    # sample_block stays the generated-noise draw
    blk = prior.sample_block(4)
    ref = op.sampler(max_growth=3).sample_block(4) + mean[None, :]
    assert blk.shape == (4, N) and np.array_equal(blk, ref)
    with pytest.raises(ValueError):
        prior.sample(host_vector(n=N + 1), m)
    with pytest.raises(ValueError):
        hf.GridKernelPrior(hf.npToDeviceOperator(np.eye(4), ctx=ctx))


# ---------------------------------------------------------------------------------------------------------------- doublePassC
@pytest.mark.parametrize("idx", range(len(tw.DPC_CASES)), ids=["%s-%s-ell%g" % ("x".join(map(str, c[0])), c[2], c[3]) for c in tw.DPC_CASES])
def test_double_pass_c_against_the_devices_double_pass_g(ctx, references, idx):
    """doublePassC(A, C) with C the grid operator against doublePassG(A, R, Rsolver) with R = inv(C) a dense operator and the same
    Omega: d (relative), U (after fixing signs) and U^T R U - I each within 4 times the numpy restatement's own difference / defect
    for the case plus 64 eps k; E^T U - I <= 1e-12."""
    case, r = tw.DPC_CASES[idx], references[idx]
    k = case[5]
    op = grid_op(case, ctx)
    assert np.abs(op.to_dense() - r["C"]).max() <= 4 * EPS
    A = hf.npToDeviceOperator(r["A"], ctx=ctx)
    Omega = hf.MultiVector.from_dense(r["Omega"], ctx=ctx)
    d, U, E = hf.doublePassC(A, op, Omega, k)
    Rop = hf.npToDeviceOperator(r["R"], ctx=ctx)
    dg, Ug = hf.doublePassG(A, Rop, hf.npToDeviceOperator(r["C"], ctx=ctx), Omega, k)
    Ug = Ug.to_dense()
    U, E = tw.fix_signs(U.to_dense(), Ug), tw.fix_signs(E.to_dense(), Ug)
    slack = 64.0 * EPS * k
    dd = np.max(np.abs(d - dg) / np.abs(dg))
    dU = np.abs(U - Ug).max()
    defect = np.abs(U.T @ r["R"] @ U - np.eye(k)).max()
    EtU = np.abs(E.T @ U - np.eye(k)).max()
    print("device doublePassC %s: d %.3g (allowed %.3g), U %.3g (%.3g), U^T R U - I %.3g (%.3g), E^T U - I %.3g, against numpy: d %.3g U %.3g"
          % (case[:4], dd, 4 * r["dd"] + slack, dU, 4 * r["dU"] + slack, defect, 4 * r["defect"] + slack, EtU,
             np.max(np.abs(d - r["d_ref"]) / np.abs(r["d_ref"])), np.abs(U - tw.fix_signs(r["U_ref"], U)).max()))
    assert dd <= 4.0 * r["dd"] + slack
    assert dU <= 4.0 * r["dU"] + slack
    assert defect <= 4.0 * r["defect"] + slack
    assert EtU <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- end to end
class _PrecisionPrior:
    """The same Gaussian as a ``GridKernelPrior`` with the dense precision R = inv(C) and Rsolver on top and no ``C``: the prior the
    reference's default path (doublePassG(A, prior.R, prior.Rsolver)) takes.  Draws are the kernel prior's, so identical seeds give
    identical samples."""

    def __init__(self, kernel_prior, Cm):
        self._k = kernel_prior
        R = np.linalg.inv(Cm)
        self.Rmat = 0.5 * (R + R.T)
        self.R = fp.MatrixOperator(self.Rmat)
        self.Rsolver = kernel_prior.Rsolver
        self.mean = kernel_prior.mean

    def init_vector(self, x, dim):
        self._k.init_vector(x, dim)

    def sample(self, noise, m, add_mean=True):
        self._k.sample(noise, m, add_mean=add_mean)


def run_projector(prior, n, q, tmp, tag):
    obs = fp.ProtocolObservable(fp.NumpyProblem(n, hf.HostVector), fp.MatrixOperator(fp.observation_matrix(q, n)))
    hf.parRandom.reseed(11)
    hf.parRandom.split(0)
    params = hf.ActiveSubspaceParameterList()
    params['samples_per_process'], params['rank'], params['oversampling'] = 6, 7, 3
    params['serialized_sampling'], params['verbose'], params['save_and_plot'] = False, False, True
    out = os.path.join(str(tmp), tag) + "/"
    os.makedirs(out)
    params['output_directory'] = out
    AS = hf.ActiveSubspaceProjector(obs, prior, parameters=params)
    d, dec, enc = AS.construct_input_subspace(prior_preconditioned=True)
    return AS, d, dec.to_dense(), enc.to_dense(), sorted(f for f in os.listdir(out) if f.endswith(".npy"))


def test_active_subspace_projector_with_a_kernel_prior(ctx, references, tmp_path):
    """(6, 5) matern32 ell 0.3, the fake PDE of 30 unknowns with 14 observations: the projector with a ``GridKernelPrior`` (doublePassC,
    no R anywhere) against the same projector with the dense R = inv(C) and the same seeds; tolerances of the doublePassC case."""
    case, r = tw.DPC_CASES[0], references[0]
    k = 7
    op = grid_op(case, ctx)
    N = op.shape[0]
    mean = 0.2 * np.cos(np.linspace(0.0, np.pi, N))
    kp = hf.GridKernelPrior(op, mean=mean)
    AS1, d1, dec1, enc1, files1 = run_projector(kp, N, 14, tmp_path, "kernel")
    AS2, d2, dec2, enc2, files2 = run_projector(_PrecisionPrior(hf.GridKernelPrior(op, mean=mean), r["C"]), N, 14, tmp_path, "precision")
    assert AS1.E_GN is not None and AS2.E_GN is None and AS1.prior_preconditioned and AS2.prior_preconditioned
    assert files1 == files2 and len(files1) >= 2
    dec1, enc1 = tw.fix_signs(dec1, dec2), tw.fix_signs(enc1, enc2)
    slack = 64.0 * EPS * k
    dd, dU, dE = np.max(np.abs(d1 - d2) / np.abs(d2)), np.abs(dec1 - dec2).max(), np.abs(enc1 - enc2).max()
    print("AS projector, kernel prior against dense R: d %.3g (allowed %.3g), decoder %.3g (%.3g), encoder %.3g (%.3g)"
          % (dd, 4 * r["dd"] + slack, dU, 4 * r["dU"] + slack, dE, 4 * r["dU"] + slack))
    assert d1.shape == (k,) and d1[-1] > 0
    assert dd <= 4.0 * r["dd"] + slack
    assert dU <= 4.0 * r["dU"] + slack
    assert dE <= 4.0 * r["dU"] + slack                       # R U on one side, E on the other: the decoder's tolerance
    assert np.abs(enc1.T @ dec1 - np.eye(k)).max() <= 1e-12
    for f in files1:
        a, b = np.load(os.path.join(str(tmp_path), "kernel", f)), np.load(os.path.join(str(tmp_path), "precision", f))
        assert a.shape == b.shape
    # the projection-error routine takes the stored encoder where it took prior.R
    samples = kp.sample_block(16)
    avg1, std1 = AS1.test_errors(ranks=[3, 7], samples=samples)
    avg2, std2 = AS2.test_errors(ranks=[3, 7], samples=samples)
    np.testing.assert_allclose(avg1, avg2, rtol=1e-9)
    assert avg1[1] < avg1[0] < 1.0
    # a projector that holds a decoder and no encoder (restored from files, say) says so, and does not ask the prior for R
    AS1.E_GN = None
    with pytest.raises(RuntimeError, match="E_GN"):
        AS1.test_errors(ranks=[3], samples=samples)
