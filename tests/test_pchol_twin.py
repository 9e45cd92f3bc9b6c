"""CPU suite of the pivoted Cholesky factor of kernel covariances (hfmi_pchol_*, hippyflow_amd/csrc/hfmi_pchol.hip): the numpy twin
(tests/helpers/pchol_twin.py) against ``kernel_cov_host`` on the cases of the GPU suite, under the same order-free properties
(tests/helpers/pchol_checks.py); the premises of the GPU suite's comparisons with the twin (pivot gaps, the rel_tol threshold); the C-ABI
bookkeeping of the new entry points; and the unchanged default of ``KLEProjector``."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import pchol_checks as pc                            # noqa: E402
import pchol_twin as twin                            # noqa: E402

from hippyflow_amd import _lib, projectors           # noqa: E402

_cache = {}


def twin_factor(case, rel_tol=0.0):
    key = (case, rel_tol)
    if key not in _cache:
        N, d, family, ell, nugget, max_rank = case
        _cache[key] = twin.factor_kernel(pc.case_points(case), family, pc.SIGMA, ell, nugget, max_rank, rel_tol)
    return _cache[key]


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_twin_properties(case):
    f = twin_factor(case)
    assert (twin.MAX_RANK, twin.REL_TOL, twin.FLOOR) == (pc.MAX_RANK, pc.REL_TOL, pc.FLOOR)
    pc.check_properties(case, f.L, f.pivots, f.trace, f.rank, f.stop_reason, "twin")


def test_twin_floor_case_rank():
    f = twin_factor(pc.FLOOR_CASE)
    assert f.stop_reason == twin.FLOOR and f.rank == 9


@pytest.mark.parametrize("case", pc.PIVOTS_COMPARABLE, ids=pc.case_id)
def test_pivot_gaps_allow_a_comparison(case):
    """where the GPU suite compares pivots with the twin, the best diagonal entry is ahead of the next distinct one by >= MIN_GAP"""
    f = twin_factor(case)
    assert f.rank > 1 and f.gaps[1:].min() >= pc.MIN_GAP, f.gaps[1:].min()


def test_rel_tol_stop():
    full, f = twin_factor(pc.REL_TOL_CASE), twin_factor(pc.REL_TOL_CASE, pc.REL_TOL_VALUE)
    assert full.gaps[1:].min() >= pc.MIN_GAP
    thr = pc.REL_TOL_VALUE * full.trace[0]
    first = int(np.argmax(full.trace <= thr))
    assert full.trace[first] <= thr and 0 < first < full.rank
    assert f.stop_reason == twin.REL_TOL and f.rank == first
    assert np.array_equal(f.pivots, full.pivots[:first]) and np.array_equal(f.L, full.L[:, :first])
    # the threshold is not a coin toss between the twin and the device
    assert np.abs(full.trace[first - 1:first + 1] - thr).min() > 1e-9 * thr


def test_twin_walks_the_generic_algorithm():
    """a 4 x 4 matrix by hand: pivots by the largest diagonal entry, ties to the lowest index"""
    A = np.array([[4.0, 2.0, 2.0, 0.0], [2.0, 4.0, 0.0, 2.0], [2.0, 0.0, 4.0, 2.0], [0.0, 2.0, 2.0, 4.0]])
    f = twin.factor(lambda p: A[:, p].copy(), 4, 4.0, 4)
    assert f.pivots.tolist() == [0, 3, 1] and f.rank == 3        # rank(A) = 3: the last diagonal entry is below the floor
    assert f.stop_reason in (twin.REL_TOL, twin.FLOOR)
    np.testing.assert_allclose(f.L @ f.L.T, A, atol=1e-14)
    g = twin.factor(lambda p: A[:, p].copy(), 4, 4.0, 2)
    assert g.stop_reason == twin.MAX_RANK and np.array_equal(g.L, f.L[:, :2])


def test_abi_bookkeeping():
    header = open(os.path.join(ROOT, "include", "hfmi.h")).read()
    names = ("hfmi_pchol_create", "hfmi_pchol_info", "hfmi_pchol_read", "hfmi_pchol_factor", "hfmi_pchol_destroy")
    for name in names:
        proto = re.search(r"HFMI_API int %s\(([^;]*)\);" % name, header)
        assert proto, name
        # a block only as const: no row in the block contract tables
        for param in proto.group(1).split(","):
            assert "hfmi_block" not in param or re.search(r"\bconst\s+hfmi_block\b", param), (name, param)
        assert name in _lib.SIGNATURES
    for value, word in enumerate(_lib.PCHOL_STOP_REASONS):
        assert re.search(r"#define HFMI_PCHOL_%s %d\b" % (word.upper(), value), header)
    assert (twin.MAX_RANK, twin.REL_TOL, twin.FLOOR) == tuple(range(3))
    assert _lib.SIGNATURES["hfmi_pchol_create"][1:3] == [ctypes.c_int, ctypes.c_double]
    src = open(os.path.join(ROOT, "hippyflow_amd", "csrc", "hfmi_pchol.hip")).read()
    assert int(re.search(r"#define PC_CHUNK (\d+)", src).group(1)) == _lib.PC_CHUNK
    assert int(re.search(r"#define PC_THREADS (\d+)", src).group(1)) == pc.ROWS_PER_TILE
    assert "hfmi_pchol.hip" in __import__("hippyflow_amd._build", fromlist=["SOURCES"]).SOURCES
    lib_path = os.path.join(ROOT, "hippyflow_amd", "libhfmi.so")
    if not os.path.exists(lib_path):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, name) for name in names)


def test_public_names_and_projector_default():
    import hippyflow_amd as hf
    assert callable(hf.pivoted_cholesky) and inspect.isclass(hf.PivotedCholesky)
    for name in ("eig", "eigenvalue_error_bound", "sample", "L", "residual_trace"):
        assert hasattr(hf.PivotedCholesky, name)
    assert hf.KLEProjector.kernel_factor_rank is None and hf.KLEProjector.randomized_eigensolver == "double_pass"
    # an attribute, not a parameter key: the parameter list keeps the reference's keys
    assert "kernel_factor_rank" not in projectors.KLEParameterList()
    src = inspect.getsource(hf.KLEProjector.construct_input_subspace)
    assert src.index("kernel_factor_rank is not None") < src.index("_draw_omega")      # the default path is entered untouched
