"""Box Whittle-Matern priors (``BoxSpectralCovariance``, hfmi_boxcov.hip) without a device: ``hfmi_boxcov_plan_predict`` -- the planner
the apply of ``hfmi_op_box`` itself asks -- against a Python statement of the plan (tests/helpers/boxcov_plan_twin.py) and against what
the kernel needs; the host formulas (``modes``, ``spectrum``, ``weights``, ``to_dense``) against the sparse form R = A W^-1 A assembled
with scipy from 1-D stiffness pieces; and the argument rules."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import boxcov_plan_twin as tw                     # noqa: E402

import hippyflow_amd as hf                        # noqa: E402
from hippyflow_amd import BoxSpectralCovariance   # noqa: E402
from hippyflow_amd import _lib as L               # noqa: E402

N_, P_ = tw.NEUMANN, tw.PERIODIC
PLAN_CASES = [((2,), (N_,)), ((3,), (N_,)), ((17,), (N_,)), ((2049,), (N_,)),
              ((1,), (P_,)), ((8,), (P_,)), ((4096,), (P_,)),
              ((9, 5), (N_, N_)), ((8, 5), (P_, N_)), ((5, 3, 4), (N_, N_, P_)),
              # beyond the issue's list: one node on a Neumann axis, long strided lines (two lines of 4096 side by side), three long axes
              ((1, 9), (N_, N_)), ((5, 8), (N_, P_)), ((3, 2049), (N_, N_)), ((4, 4096), (P_, P_)), ((33, 16, 17), (N_, P_, N_))]


@pytest.mark.parametrize("shape,boundary", PLAN_CASES)
@pytest.mark.parametrize("nvec", [1, 3])
def test_plan_predict_matches_the_twin(shape, boundary, nvec):
    for budget in (0, 1, 1 << 20):
        words = tw.predict(L, shape, boundary, nvec, budget)
        p = tw.plan(shape, boundary, nvec, budget)
        assert words == tw.plan_words(p), (shape, boundary, nvec, budget)
    n = list(shape) + [1] * (3 - len(shape))
    assert p["N"] == int(np.prod(shape)) and p["pair_bytes"] == 16 * p["N"]
    assert len(p["passes"]) == 2 * len(shape) - 1
    for q in p["passes"]:
        nb = n[q["axis"]]
        assert q["L"] == (nb if boundary[q["axis"]] == P_ else max(2 * (nb - 1), 1)) and q["L"] & (q["L"] - 1) == 0
        assert q["lds_total"] <= tw.LDS_BYTES and q["lpw"] <= tw.MAX_LINES and 64 <= q["threads"] <= 512 and q["threads"] % 64 == 0, q
        assert q["lpw"] & (q["lpw"] - 1) == 0 and q["ls"] >= q["L"]
        assert (q["grid_x"] - 1) * q["lpw"] < q["nlines"] <= q["grid_x"] * q["lpw"], q
        # the lines of a pass and their n positions are the N entries of the buffer, each once
        entries = (tw.line_bases(q)[:, None] + np.arange(q["n"])[None, :] * q["stride"]).ravel()
        assert np.array_equal(np.sort(entries), np.arange(p["N"])), q
    assert p["chunk_pairs"] >= 1 and p["chunk_pairs"] * p["nchunks"] >= p["pairs"] > (p["nchunks"] - 1) * p["chunk_pairs"]


def test_plan_counts_the_pairs_knob():
    L.call("hfmi_tuning_set", b"fftcov_pairs", 1)
    try:
        words = tw.predict(L, (9, 5), (N_, N_), 5)
    finally:
        L.call("hfmi_tuning_set", b"fftcov_pairs", 0)
    assert words == tw.plan_words(tw.plan((9, 5), (N_, N_), 5, forced=1)) and words[6] == 1 and words[7] == 3


def test_plan_predict_refuses_bad_grids():
    bad = [((4,), (N_,)), ((2050,), (N_,)), ((4097,), (N_,)), ((6,), (P_,)), ((8192,), (P_,)), ((0,), (N_,)), ((0,), (P_,)), ((5,), (2,)),
           ((5, 6), (N_, N_))]
    for shape, boundary in bad:
        with pytest.raises(L.HfmiError):
            tw.predict(L, shape, boundary, 2)
    words = (C.c_int64 * tw.PLAN_WORDS)()
    n = (C.c_int64 * 4)(5, 5, 5, 5)
    b = (C.c_int * 4)(0, 0, 0, 0)
    for d in (0, 4):
        with pytest.raises(L.HfmiError):
            L.call("hfmi_boxcov_plan_predict", d, C.cast(n, C.c_void_p), C.cast(b, C.c_void_p), 2, 0, words)
    with pytest.raises(L.HfmiError):
        L.call("hfmi_boxcov_plan_predict", 1, C.cast(n, C.c_void_p), C.cast(b, C.c_void_p), -1, 0, words)


def stiffness_1d(n, h, periodic):
    """the two-point stiffness matrix of one axis: (1 / h) tridiag(-1, 2, -1), Neumann ends with 1 on the diagonal, or wrapped"""
    if n == 1:
        return sp.csr_matrix((1, 1))
    K = sp.lil_matrix((n, n))
    for j in range(n - 1 if not periodic else n):
        a, b = j, (j + 1) % n
        K[a, a] += 1.0 / h
        K[b, b] += 1.0 / h
        K[a, b] -= 1.0 / h
        K[b, a] -= 1.0 / h
    return K.tocsr()


def sparse_A(box):
    """A = delta W + gamma K, K the tensor sum of the 1-D stiffness matrices weighted by theta_c and the other axes' w (axis 0 fastest)"""
    d = len(box.grid_shape)
    w1 = [box._axis_weights(c) for c in range(d)]
    K = sp.csr_matrix((box.N, box.N))
    for c in range(d):
        term = sp.identity(1, format="csr")
        for b in range(d):
            piece = stiffness_1d(box.grid_shape[b], float(box.spacing[b]), box.boundary[b] == "periodic") if b == c else sp.diags(w1[b])
            term = sp.kron(piece, term, format="csr")
        K = K + box.theta[c] * term
    return box.delta * sp.diags(box.weights) + box.gamma * K


HOST_CASES = [((9, 5), "neumann"), ((8, 5), ("periodic", "neumann")), ((4, 4), "periodic")]


@pytest.mark.parametrize("shape,boundary", HOST_CASES)
def test_host_formulas_reproduce_the_sparse_form(shape, boundary):
    """symbol "fd", alpha = 2: to_dense("R") = A W^-1 A and to_dense("C") to_dense("R") = I, defect at most 1e-12 max |entry|."""
    box = BoxSpectralCovariance(shape, (0.25, 0.4), gamma=0.7, delta=1.3, alpha=2.0, theta=(1.0, 2.5), boundary=boundary, symbol="fd")
    A = sparse_A(box).toarray()
    R_ref = A @ np.diag(1.0 / box.weights) @ A
    R = box.to_dense("R")
    Cd = box.to_dense("C")
    d1 = np.abs(R - R_ref).max() / np.abs(R_ref).max()
    I = Cd @ R
    d2 = np.abs(I - np.eye(box.N)).max()
    print("R vs A W^-1 A: %.2e   C R - I: %.2e" % (d1, d2))
    assert d1 <= 1e-12
    assert d2 <= 1e-12 * max(1.0, np.abs(I).max())
    # and the modes are W-orthonormal, the factor squares to C, the transposed factor is the transpose
    Phi = box.modes()
    assert np.abs(Phi.conj().T @ (box.weights[:, None] * Phi) - np.eye(box.N)).max() <= 1e-12
    S = box.to_dense("S")
    assert np.abs(S @ S.T - Cd).max() <= 1e-12 * np.abs(Cd).max()
    assert np.abs(box.to_dense("St") - S.T).max() <= 1e-12 * np.abs(S).max()
    assert np.abs(box.to_dense("Sinv") @ S - np.eye(box.N)).max() <= 1e-11


def test_weights_points_and_spectrum_shapes():
    box = BoxSpectralCovariance((5, 3, 4), (0.5, 0.25, 2.0), 1.0, 1.0, boundary=("neumann", "neumann", "periodic"), origin=(1.0, 2.0, 3.0))
    w = box.weights.reshape(4, 3, 5)
    assert w.shape == (4, 3, 5) and box.weights.shape == (60,)
    assert w[1, 1, 2] == 0.5 * 0.25 * 2.0 and w[0, 0, 0] == 0.25 * 0.125 * 2.0 and w[3, 1, 4] == 0.25 * 0.25 * 2.0
    assert np.isclose(box.weights.sum(), (4 * 0.5) * (2 * 0.25) * (4 * 2.0))
    assert box.points.shape == (60, 3) and np.allclose(box.points[1 + 5 * (2 + 3 * 3)], (1.5, 2.5, 9.0))
    lam = box.spectrum()
    assert lam.shape == (5, 3, 4) and lam[0, 0, 0] == 1.0 and np.all(lam > 0.0) and np.all(lam <= 1.0)
    assert lam[0, 0, 1] == lam[0, 0, 3]                 # periodic: modes k and n - k share their eigenvalue
    one = BoxSpectralCovariance((1, 9), 0.5, 1.0, 1.0)
    assert np.array_equal(one.weights, [0.25] + [0.5] * 7 + [0.25])      # a Neumann axis of one node has weight 1


def test_argument_rules_raise_before_any_device_call():
    ok = dict(shape=(9, 5), spacing=0.1, gamma=1.0, delta=1.0)
    BoxSpectralCovariance(**ok)
    bad = [dict(shape=(4, 5)), dict(shape=(9.7, 5)), dict(shape=("9", 5)), dict(shape=(2050,)), dict(shape=(6,), boundary="periodic"), dict(shape=(8192,), boundary="periodic"),
           dict(shape=(0, 5)), dict(shape=(3, 3, 3, 3)), dict(spacing=0.0), dict(spacing=(0.1, np.inf)), dict(spacing=(0.1,)),
           dict(gamma=0.0), dict(gamma=np.nan), dict(delta=-1.0), dict(alpha=0.0), dict(alpha=np.inf), dict(theta=(1.0, 0.0)),
           dict(theta=(1.0, 1.0, 1.0)), dict(boundary="robin"), dict(boundary=("neumann",)), dict(symbol="spectral"),
           dict(origin=(0.0,))]
    for change in bad:
        with pytest.raises(ValueError):
            BoxSpectralCovariance(**{**ok, **change})
    box = BoxSpectralCovariance(**ok)
    with pytest.raises(ValueError):
        box.to_dense("Q")
    with pytest.raises(ValueError):
        hf.BoxSpectralPrior(object())


def test_the_c_abi_declares_the_box():
    header = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    for name in ("hfmi_box_create", "hfmi_box_destroy", "hfmi_box_spectrum", "hfmi_op_box", "hfmi_boxcov_plan_predict"):
        assert name in L.SIGNATURES
        assert re.search(r"HFMI_API int %s\(" % name, header), name
    assert "#define HFMI_BOXCOV_PLAN_WORDS %d" % tw.PLAN_WORDS in header and L.BOXCOV_PLAN_WORDS == tw.PLAN_WORDS
    assert "hfmi_boxcov.hip" in __import__("hippyflow_amd._build", fromlist=["SOURCES"]).SOURCES
