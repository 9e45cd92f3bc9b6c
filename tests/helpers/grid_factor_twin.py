"""Numpy statements of the factor C = S S^T of a grid sampler's embedding (hfmi_op_grid_factor, hfmi_fftcov.hip) and of the double pass
in encoder coordinates (``randomized.doublePassC``), restated from the rules in hippyflow_amd/csrc/hfmi_fftcov_plan.h and the docstring:

* the launch plan of an apply of S / S^T (``plan``), word for word what ``hfmi_fftcov_factor_plan_predict`` writes;
* S = Rn Chat^(1/2) and S^T = Chat^(1/2) Rn^T with ``numpy.fft`` (``apply_S`` / ``apply_St`` / ``dense_S``): a padded vector has
  prod P_c entries in natural order, entry e = s_0 + P_0 (s_1 + P_1 s_2), i.e. an array of shape (P_{d-1}, ..., P_0) in C order;
  Chat^(1/2) xi = ifftn(sqrt(max(Lambda, 0)) fftn(xi)); two columns ride one transform as in the apply;
* the error bound of a device apply against this twin (``column_bounds``): the FFT term of ``fftcov_twin.column_bounds`` with the root
  spectrum in place of Lambda;
* ``double_pass_c``: the algorithm of ``randomized.doublePassC`` on numpy arrays, with the oracle's B-orthogonalisation.

The case tables are shared between the CPU and the GPU suites."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import hippylib_restated as hl       # noqa: E402

import fftcov_twin as ft                          # noqa: E402
import grid_sampler_twin as gs                    # noqa: E402
from fftcov_plan_twin import (DEFAULT_BUDGET, FWD, GATHER, HEAD_WORDS, INV, MAX_PAIRS, MUL, PASS_FIELDS, PASS_WORDS, PLAN_WORDS, SCATTER,
                              STATIC_LDS, make_pass)
from grid_sampler_plan_twin import embedding as plan_embedding, feasible     # noqa: E402,F401

EPS = np.finfo(np.float64).eps
LOAD_FULL, STORE_FULL = 64, 128


# ---------------------------------------------------------------------------------------------------------------- the launch plan
def plan(shape, growth, transpose, nvec, budget=0, forced=0):
    """2 d - 1 passes.  S: forward along 0 .. d - 2 over ALL lines, the first loading P_0 positions from the block of padded vectors;
    the fused pass along d - 1 loads P_{d-1} and stores n_{d-1}; the apply's inverse passes.  S^T: the apply's forward passes; the fused
    pass loads n_{d-1} and stores P_{d-1}; inverse along d - 2 .. 0 over ALL lines, the last storing P_0 positions into the block."""
    d = len(shape)
    n = list(shape) + [1] * (3 - d)
    P = plan_embedding(shape, growth)
    Ptot = P[0] * P[1] * P[2]
    fwd_ext, inv_ext = (n, P) if transpose else (P, n)
    load_side, store_side = (0, STORE_FULL) if transpose else (LOAD_FULL, 0)
    inlen = (lambda a: n[a]) if transpose else (lambda a: P[a])
    outlen = (lambda a: P[a]) if transpose else (lambda a: n[a])
    passes = []
    for a in range(d - 1):
        passes.append(make_pass(P, a, FWD | ((SCATTER | load_side) if a == 0 else 0), fwd_ext, inlen(a), P[a]))
    passes.append(make_pass(P, d - 1, FWD | MUL | INV | ((SCATTER | GATHER | load_side | store_side) if d == 1 else 0), n, inlen(d - 1),
                            outlen(d - 1)))
    for a in range(d - 2, -1, -1):
        passes.append(make_pass(P, a, INV | ((GATHER | store_side) if a == 0 else 0), inv_ext, P[a], outlen(a)))
    pairs = (nvec + 1) // 2
    if budget <= 0:
        budget = DEFAULT_BUDGET
    chunk = forced if forced > 0 else budget // (16 * Ptot)
    chunk = max(1, min(chunk, MAX_PAIRS, pairs))
    return dict(d=d, P=P, Ptot=Ptot, growth=growth, transpose=transpose, pairs=pairs, chunk_pairs=chunk,
                nchunks=(pairs + chunk - 1) // chunk if pairs else 0, pair_bytes=16 * Ptot, twiddles=max(max(P) // 4, 1), Pmax=max(P),
                passes=passes)


def plan_words(p):
    w = [0] * PLAN_WORDS
    w[:15] = [p["d"], p["P"][0], p["P"][1], p["P"][2], p["Ptot"], p["pairs"], p["chunk_pairs"], p["nchunks"], len(p["passes"]),
              p["pair_bytes"], p["twiddles"], p["Pmax"], STATIC_LDS, p["growth"], p["transpose"]]
    for i, q in enumerate(p["passes"]):
        w[HEAD_WORDS + i * PASS_WORDS:HEAD_WORDS + (i + 1) * PASS_WORDS] = [q[f] for f in PASS_FIELDS]
    return w


def predict(L, shape, growth, transpose, nvec, budget=0):
    """the library's words for the same call"""
    words = (C.c_int64 * PLAN_WORDS)()
    n = (C.c_int64 * len(shape))(*shape)
    L.call("hfmi_fftcov_factor_plan_predict", len(shape), C.cast(n, C.c_void_p), int(growth), int(transpose), int(nvec), int(budget), words)
    return list(words)


def expected_bases(p, shape, q, full_above):
    """the lines a pass along q['axis'] takes: every position of the axes below it; of the axes above it all P_b positions
    (``full_above``: they hold data everywhere) or the first n_b"""
    P = p["P"]
    n = list(shape) + [1] * (3 - len(shape))
    a = q["axis"]
    rng = [np.arange(P[b]) if b < a else np.arange(1) if b == a else np.arange(P[b] if full_above else n[b]) for b in range(3)]
    i0, i1, i2 = np.meshgrid(*rng, indexing="ij")
    return np.sort((i0 + P[0] * (i1 + P[1] * i2)).ravel())


# ---------------------------------------------------------------------------------------------------------------- S and S^T
def root_spectrum(shape, spacing, family, sigma, ell, nugget, growth, lam=None):
    """sqrt(max(Lambda, 0)) in natural frequency order, shape (P_{d-1}, ..., P_0)"""
    if lam is None:
        lam = gs.spectrum(shape, spacing, family, sigma, ell, nugget, growth)
    return np.sqrt(np.maximum(lam, 0.0))


def apply_S(root, shape, Xi, nodes=None):
    """(N, k) = S Xi for Xi of prod P_c rows in natural order"""
    idx = gs.node_index(shape, nodes)
    k = Xi.shape[1]
    Y = np.empty((idx[0].size, k))
    for j in range(0, k, 2):
        z = (Xi[:, j] + (1j * Xi[:, j + 1] if j + 1 < k else 0.0)).reshape(root.shape)
        y = np.fft.ifftn(root * np.fft.fftn(z))[idx]
        Y[:, j] = y.real
        if j + 1 < k:
            Y[:, j + 1] = y.imag
    return Y


def apply_St(root, shape, X, nodes=None):
    """(prod P_c, k) = S^T X"""
    idx = gs.node_index(shape, nodes)
    k = X.shape[1]
    Y = np.empty((root.size, k))
    for j in range(0, k, 2):
        z = np.zeros(root.shape, dtype=np.complex128)
        z[idx] = X[:, j] + (1j * X[:, j + 1] if j + 1 < k else 0.0)
        y = np.fft.ifftn(root * np.fft.fftn(z)).ravel()
        Y[:, j] = y.real
        if j + 1 < k:
            Y[:, j + 1] = y.imag
    return Y


DENSE_MAX_P = 8192


def dense_S(root, shape, nodes=None):
    """S as an (N, prod P_c) array, column by column of the identity"""
    assert root.size <= DENSE_MAX_P
    return apply_S(root, shape, np.eye(root.size), nodes)


def column_bounds(root, W):
    """per column j: 32 max(1, log2 P) eps sqrt(P) ||r||_2 ||W[:, j]||_2 with r the first column of Chat^(1/2) (sqrt(P) ||r||_2 is the
    2-norm of the root spectrum): the FFT term of ``fftcov_twin.column_bounds`` with the root spectrum in place of Lambda"""
    P = root.size
    return 32.0 * max(1.0, np.log2(P)) * EPS * np.linalg.norm(root) * np.linalg.norm(W, axis=0)


def twin_tolerance(Ptot, sigma, nugget):
    """max |S S^T - C| of the fp64 twin: 64 eps log2(prod P_c) (sigma^2 + nugget)"""
    return 64.0 * EPS * np.log2(Ptot) * (sigma ** 2 + nugget)


# the CPU twin's cases: (shape, spacing, family, ell, nugget, growth); sigma = 1, h = 1 / (n - 1) unless given
def unit_spacing(shape):
    return tuple(1.0 / (n - 1) for n in shape)


DEFINITE = [((6, 5), None, "matern32", 0.3, 0.0, 0),
            ((6, 5), None, "matern32", 0.3, 0.0, 1),
            ((7,), None, "matern52", 0.2, 1e-8, 1),
            ((9, 8), None, "sqexp", 0.4, 1e-6, 2)]
# (4, 3, 3): spacing (0.4, 0.3, 0.3), at which lambda_min / lambda_max = -5.1e-3 and the bound is 1.04e-3
CLIPPED = [((4, 3, 3), (0.4, 0.3, 0.3), "matern12", 0.5, 0.0, 0),
           ((9, 8), (0.125, 0.125), "matern32", 1.0, 0.0, 0)]

# the GPU suite's cases: (id, shape, spacing, subset of the nodes, family, ell, nugget, growths).  Kernels whose embeddings have
# no eigenvalue within rounding of zero: the device's spectrum and numpy's differ by rounding, and a square root turns a difference
# delta of an eigenvalue lambda into delta / (2 sqrt(lambda)), which only a spectrum bounded away from zero keeps at rounding level
# (tests/test_grid_factor_twin_cpu.py measures it for these cases).
GPU_SIGMA = 1.3
GPU_CASES = [("7", (7,), (0.15,), False, "matern32", 0.3, 0.0, (0, 1, 2)),
             ("33", (33,), (0.031,), False, "matern12", 0.2, 0.0, (0, 1, 2)),
             ("33-subset", (33,), (0.031,), True, "matern32", 0.1, 1e-2, (0, 2)),
             ("6x5", (6, 5), (0.2, 0.25), False, "matern32", 0.3, 0.0, (0, 1, 2)),
             ("17x12-subset", (17, 12), (0.06, 0.09), True, "matern52", 0.25, 1e-2, (0, 1, 2)),
             ("4x3x3", (4, 3, 3), (0.4, 0.3, 0.3), False, "matern12", 0.5, 0.0, (0, 1, 2)),
             ("9x8x7", (9, 8, 7), (0.12, 0.14, 0.16), False, "matern32", 0.3, 0.0, (0, 1, 2)),
             ("300x70", (300, 70), (1.0 / 299, 1.0 / 69), False, "matern12", 0.05, 0.0, (0, 1)),     # P = 1024 x 256 and 2048 x 512
             ("1", (1,), (0.15,), False, "matern12", 0.3, 0.0, (0,)),        # the fused pass of d = 1 on lines of 1, 4 and 8 entries
             ("2", (2,), (0.15,), False, "matern12", 0.3, 0.0, (0, 1))]
GPU_NVECS = (1, 2, 3, 5)


def gpu_case_is_definite(case, growth):
    """the creation rule's verdict on the embedding of a GPU case at a forced growth (``grid_sampler_twin.floor``)"""
    lam = gs.spectrum(case[1], case[2], case[4], GPU_SIGMA, case[5], case[6], growth)
    return bool(lam.min() >= -gs.floor(lam.size, lam.max()))


def gpu_case_nodes(shape, subset):
    return ft.case_nodes(shape, subset, 11)


# ---------------------------------------------------------------------------------------------------------------- the double pass
def double_pass_c(A, Cm, Omega, k, s=1):
    """``randomized.doublePassC`` on numpy arrays: Yv = (A C)^(s-1) A Omega, (Qv, BQ) = C-orth(Yv) (the oracle's Borthogonalize),
    T = BQ^T A BQ, eigh, descending, k leading vectors W: d, U = BQ W, E = Qv W"""
    Yv = hl.as_block(A @ Omega)
    for _ in range(s - 1):
        Yv = hl.as_block(A @ (Cm @ Yv))
    BQ, _ = hl.mgs_stable(Yv, hl.DenseOperator(Cm))
    T = (A @ BQ).T @ BQ
    d, V = np.linalg.eigh(T)
    order = d.argsort()[::-1][:k]
    return d[order], BQ @ V[:, order], Yv @ V[:, order]


# (shape, spacing or None for h = 1 / (n - 1), family, ell, q, k, p): sigma = 1, no nugget; the last has h = 1 / 8.  k is case[5]
DPC_CASES = [((6, 5), None, "matern32", 0.3, 14, 7, 3),
             ((9, 8), None, "matern52", 0.25, 30, 10, 5),
             ((5, 4, 3), None, "matern12", 0.4, 20, 8, 4),
             ((9, 8), (0.125, 0.125), "matern32", 1.0, 30, 10, 5)]


def dpc_problem(case):
    """(C, A = J^T J, Omega) of a case: J = (G diag(exp(-0.15 j))) G' with G (q x q), G' (q x N) and Omega (N x (k + p)) standard
    normal from rng(0), in that order"""
    shape, spacing, family, ell, q, k, p = case
    spacing = unit_spacing(shape) if spacing is None else spacing
    pts = ft.points(shape, spacing)
    N = pts.shape[0]
    r = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    Cm = ft.phi(family, r / ell)
    rng = np.random.default_rng(0)
    G, G2 = rng.standard_normal((q, q)), rng.standard_normal((q, N))
    J = (G * np.exp(-0.15 * np.arange(q))[None, :]) @ G2
    Omega = rng.standard_normal((N, k + p))
    return Cm, J.T @ J, Omega


def fix_signs(U, Uref):
    """U with every column's sign set to agree with Uref's"""
    s = np.sign(np.sum(U * Uref, axis=0))
    s[s == 0] = 1.0
    return U * s[None, :]


def dpc_reference(case):
    """numpy doublePassC against the oracle's doublePassG with R = inv(C) for the same Omega: the record the device test scales its
    tolerances from.  Returns dict(d, U, E, d_ref, U_ref, R, dd, dU, defect, EtU)."""
    Cm, A, Omega = dpc_problem(case)
    k = case[5]
    R = np.linalg.inv(Cm)
    R = 0.5 * (R + R.T)

    class _Solve:
        def solve(self, y, x):
            y[...] = Cm @ x

    d_ref, U_ref = hl.double_pass_g(hl.DenseOperator(A), hl.DenseOperator(R), _Solve(), Omega, k)
    d, U, E = double_pass_c(A, Cm, Omega, k)
    U = fix_signs(U, U_ref)
    E = fix_signs(E, U_ref)
    return dict(C=Cm, A=A, Omega=Omega, R=R, d=d, U=U, E=E, d_ref=d_ref, U_ref=U_ref,
                dd=float(np.max(np.abs(d - d_ref) / np.abs(d_ref))), dU=float(np.abs(U - U_ref).max()),
                defect=float(np.abs(U.T @ R @ U - np.eye(k)).max()), EtU=float(np.abs(E.T @ U - np.eye(k)).max()))
