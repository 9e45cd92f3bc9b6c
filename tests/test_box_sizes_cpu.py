"""Box Whittle-Matern priors on axes whose transformed line has odd factors (2^m 3^a 5^b entries, a multiple of 4), without a device:
the position map and the stages of tests/helpers/boxcov_mr_twin.py against ``numpy.fft.fft``, ``hfmi_boxcov_plan_predict`` against the
twin's plan word for word, every legal length launchable as the contiguous and as a strided axis, the refusals in C and in Python, and
the host formulas against the sparse form R = A W^-1 A at sizes that were refused before."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import boxcov_mr_twin as mr                       # noqa: E402
import boxcov_plan_twin as tw                     # noqa: E402

from hippyflow_amd import BoxSpectralCovariance   # noqa: E402
from hippyflow_amd import _lib as L               # noqa: E402

N_, P_ = tw.NEUMANN, tw.PERIODIC
LEGAL = mr.legal_lengths()
MIXED = [v for v in LEGAL if mr.factor(v) is not None]


def test_the_legal_lengths_are_the_issues_list():
    assert len(LEGAL) == 87 and len(MIXED) == 76 and max(MIXED) == 4000
    neumann = (7, 11, 13, 19, 21, 25, 31, 37, 41, 49, 51, 61, 73, 81, 97, 101, 121, 161, 193, 201, 385, 769, 1921, 1945, 2001)
    periodic = (12, 20, 24, 36, 40, 48, 60, 96, 100, 192, 3840, 3888, 4000)
    assert all(2 * (n - 1) in MIXED for n in neumann) and all(n in MIXED for n in periodic)
    # what was legal stays legal, what the existing tests pin as refused stays refused
    assert all(mr.axis_ok(n, N_) for n in [1] + [2 ** m + 1 for m in range(12)]) and all(mr.axis_ok(2 ** m, P_) for m in range(13))
    assert not any(mr.axis_ok(n, N_) for n in (0, 4, 6, 2050, 4097)) and not any(mr.axis_ok(n, P_) for n in (0, 6, 8192))


@pytest.mark.parametrize("length", MIXED)
def test_position_map_is_a_permutation_and_the_stages_are_the_fft(length):
    mode = mr.modes(length)
    assert np.array_equal(np.sort(mode), np.arange(length))
    if length <= 512 or length in (3840, 3888, 4000):
        rng = np.random.default_rng(length)
        x = rng.standard_normal(length) + 1j * rng.standard_normal(length)
        ref = np.fft.fft(x)
        err = np.abs(mr.staged_forward(x) - ref[mode]).max() / np.abs(ref).max()
        print("L = %d: staged transform against numpy's FFT %.2e" % (length, err))
        # about log2 L rounded complex multiply-adds per entry on either side
        assert err <= 8 * np.log2(length) * np.finfo(np.float64).eps


PLAN_CASES = [((7,), (N_,)), ((11,), (N_,)), ((193, 193), (N_, N_)), ((193, 129), (N_, N_)), ((12, 7), (P_, N_)), ((5, 12), (N_, P_)),
              ((25, 20, 7), (N_, P_, N_))]          # 20 nodes are legal on a periodic axis only (Neumann: 38 entries)


@pytest.mark.parametrize("shape,boundary", PLAN_CASES)
@pytest.mark.parametrize("nvec", [1, 3])
def test_plan_predict_matches_the_mixed_radix_twin(shape, boundary, nvec):
    for budget in (0, 1, 1 << 20):
        words = tw.predict(L, shape, boundary, nvec, budget)
        p = mr.plan(shape, boundary, nvec, budget)
        assert words == mr.plan_words(p), (shape, boundary, nvec, budget)
    assert len(p["passes"]) == 2 * len(shape) - 1 and p["N"] == int(np.prod(shape))
    for q in p["passes"]:
        f = mr.factor(q["L"])
        assert (q["n3"], q["n5"]) == (f[:2] if f else (0, 0))
        entries = (tw.line_bases(q)[:, None] + np.arange(q["n"])[None, :] * q["stride"]).ravel()
        assert np.array_equal(np.sort(entries), np.arange(p["N"])), q
    pow2_lines = [v for v in p["P"] if mr.pow2(v)]
    assert p["Pmax"] == max(pow2_lines + [1]) and p["twiddles"] == max(p["Pmax"] // 4, 1)


def test_plans_of_power_of_two_grids_are_unchanged():
    """the mixed-radix twin falls back to the old twin pass for pass, and words 14 and 15 of every pass are zero"""
    for shape, boundary in (((9, 5), (N_, N_)), ((8, 5), (P_, N_)), ((33, 16, 17), (N_, P_, N_))):
        words = tw.predict(L, shape, boundary, 3)
        assert words == tw.plan_words(tw.plan(shape, boundary, 3)) == mr.plan_words(mr.plan(shape, boundary, 3))


@pytest.mark.parametrize("length", LEGAL)
def test_every_legal_length_can_be_launched_contiguous_and_strided(length):
    """as the only axis, as axis 0 of a wide grid, as the strided axis beside 3 and beside 64 nodes; Neumann where the length is even"""
    sides = [(length, P_)] + ([(length // 2 + 1, N_)] if length % 2 == 0 else [])
    for n, side in sides:
        for shape, boundary in (((n,), (side,)), ((n, 64), (side, P_)), ((3, n), (N_, side)), ((64, n), (P_, side))):
            words = tw.predict(L, shape, boundary, 2)
            assert words == mr.plan_words(mr.plan(shape, boundary, 2)), (shape, boundary)
            for i in range(words[8]):
                q = dict(zip(mr.PASS_FIELDS, words[tw.HEAD_WORDS + i * tw.PASS_WORDS:]))
                assert q["lds_total"] <= tw.LDS_BYTES and 64 <= q["threads"] <= tw.MAX_THREADS and q["threads"] % 64 == 0, q
                assert 1 <= q["lpw"] <= tw.MAX_LINES and q["lpw"] & (q["lpw"] - 1) == 0 and q["ls"] >= q["L"], q
                assert q["lds"] == 16 * (q["lpw"] * q["ls"] + max(q["L"] // 4, 1)), q
                assert (q["grid_x"] - 1) * q["lpw"] < q["nlines"] <= q["grid_x"] * q["lpw"], q
                if q["stride"] > 1 and q["nlines"] >= 4:
                    assert q["lpw"] >= min(4, mr.pow2floor(tw.STRIDED_ELEMS // q["L"])), q


REFUSED = [((8,), (N_,)), ((15,), (N_,)), ((23,), (N_,)), ((28,), (P_,)), ((18,), (P_,)), ((4100,), (P_,)), ((2161,), (N_,)),
           ((7, 8), (N_, N_)), ((12, 28), (P_, P_))]
ACCEPTED = [((7,), (N_,)), ((2001,), (N_,)), ((12,), (P_,)), ((4000,), (P_,))]
NAMES = {N_: "neumann", P_: "periodic"}


@pytest.mark.parametrize("shape,boundary", REFUSED)
def test_refused_in_c_and_in_python(shape, boundary):
    assert not all(mr.axis_ok(n, b) for n, b in zip(shape, boundary))
    with pytest.raises(L.HfmiError) as e:
        tw.predict(L, shape, boundary, 2)
    assert e.value.code == -1 and "2, 3 and 5" in str(e.value)
    with pytest.raises(ValueError, match="2, 3 and 5"):
        BoxSpectralCovariance(shape, 0.1, 1.0, 1.0, boundary=[NAMES[b] for b in boundary])


@pytest.mark.parametrize("shape,boundary", ACCEPTED)
def test_accepted_in_c_and_in_python(shape, boundary):
    assert all(mr.axis_ok(n, b) for n, b in zip(shape, boundary))
    words = tw.predict(L, shape, boundary, 2)
    assert words[0] == 1 and words[1] == shape[0] and words[13] == tw.line_len(shape[0], boundary[0])
    box = BoxSpectralCovariance(shape, 0.1, 1.0, 1.0, boundary=[NAMES[b] for b in boundary])
    assert box.N == shape[0] and box.spectrum().shape == shape


def stiffness_1d(n, h, periodic):
    """the two-point stiffness matrix of one axis, as tests/test_box_prior_cpu.py builds it"""
    if n == 1:
        return sp.csr_matrix((1, 1))
    K = sp.lil_matrix((n, n))
    for j in range(n if periodic else n - 1):
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


HOST_CASES = [((7,), "neumann"), ((12,), "periodic"), ((7, 5), "neumann")]


@pytest.mark.parametrize("shape,boundary", HOST_CASES)
def test_host_formulas_reproduce_the_sparse_form_at_the_new_sizes(shape, boundary):
    """symbol "fd", alpha = 2: to_dense("R") = A W^-1 A and to_dense("C") to_dense("R") = I, defect at most 1e-12 max |entry|, as
    tests/test_box_prior_cpu.py holds (9, 5) to."""
    d = len(shape)
    box = BoxSpectralCovariance(shape, (0.25, 0.4)[:d], gamma=0.7, delta=1.3, alpha=2.0, theta=(1.0, 2.5)[:d], boundary=boundary, symbol="fd")
    A = sparse_A(box).toarray()
    R_ref = A @ np.diag(1.0 / box.weights) @ A
    R, Cd = box.to_dense("R"), box.to_dense("C")
    d1 = np.abs(R - R_ref).max() / np.abs(R_ref).max()
    I = Cd @ R
    d2 = np.abs(I - np.eye(box.N)).max()
    print("R vs A W^-1 A: %.2e   C R - I: %.2e" % (d1, d2))
    assert d1 <= 1e-12
    assert d2 <= 1e-12 * max(1.0, np.abs(I).max())
    S = box.to_dense("S")
    assert np.abs(S @ S.T - Cd).max() <= 1e-12 * np.abs(Cd).max()
