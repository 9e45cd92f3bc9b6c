"""CPU suite: the rules of the sparse SPD solves (hippyflow_amd/csrc/hfmi_spsolve_rules.h) through ``hfmi_cheb_rules_predict`` and
``hfmi_lanczos_bracket_predict`` -- the functions cheb_solve, cheb_estimate, launch_cheb_step and the V-cycle's smoother themselves ask,
without a device -- against tests/helpers/spsolve_rules_twin.py, the expressions they replaced."""
import ctypes as C
import itertools
import math
import types

import numpy as np
import pytest
import scipy.sparse as sp

from hippyflow_amd import _lib as L
from tests.helpers import amg_vcycle_twin
from tests.helpers import spsolve_rules_twin as tw

_D = C.POINTER(C.c_double)


def predict(lmin, lmax, rel_tol=1e-13, max_iter=500, nrows=1000, k=6, resid=0, knobs=(0, 0, 1), nsteps=0):
    words = (C.c_int64 * tw.WORDS)()
    coef = (C.c_double * (2 + 2 * nsteps))()
    L.call("hfmi_cheb_rules_predict", float(lmin), float(lmax), float(rel_tol), int(max_iter), int(nrows), int(k), int(resid),
           (C.c_int * 3)(*knobs), nsteps, coef, words)
    return list(words), np.array(coef)


def bracket(rz, pap, gersh):
    rz, pap = np.ascontiguousarray(rz, dtype=np.float64), np.ascontiguousarray(pap, dtype=np.float64)
    refusal, values = C.c_int(-1), (C.c_double * 4)()
    L.call("hfmi_lanczos_bracket_predict", len(pap), rz.ctypes.data_as(_D), pap.ctypes.data_as(_D), float(gersh), C.byref(refusal), values)
    return (refusal.value,) + tuple(values)


# ------------------------------------------------------------------ coefficients
INTERVALS = [(0.5, 2.0)] + [(lmax / 4, lmax) for lmax in (1.1, 1.9, 2.7)] + [(1.0, 1.0 + 1e-13), (2e-4, 2.0)]


@pytest.mark.parametrize("lmin,lmax", INTERVALS)
def test_coefficients_equal_the_parent_expressions(lmin, lmax):
    _, coef = predict(lmin, lmax, nsteps=200)
    inv_theta, spread, steps = tw.coefficients(lmin, lmax, 200)
    assert coef[0] == inv_theta and coef[1] == float(spread)
    assert spread == ((lmin, lmax) != (1.0, 1.0 + 1e-13))
    got = coef[2:].reshape(-1, 2)[:len(steps)]
    assert len(steps) == (200 if spread else 0) and not coef[2 + 2 * len(steps):].any()
    if spread:
        assert np.max(np.abs(got - np.array(steps)) / np.abs(np.array(steps))) <= 1e-14


@pytest.mark.parametrize("degree", range(1, 17))
def test_coefficients_reproduce_the_vcycle_twin(degree):
    """the recurrence run with the predicted coefficients is amg_vcycle_twin.chebyshev, from x0 = 0 and from an x0"""
    rng = np.random.default_rng(degree)
    n = 12
    A = sp.diags([np.full(n - 1, -0.3), np.linspace(1.0, 2.0, n), np.full(n - 1, -0.3)], [-1, 0, 1], format="csr")
    level = types.SimpleNamespace(A=A, inv_diag=1.0 / A.diagonal(), lmin=0.4, lmax=1.6)
    b = rng.standard_normal((n, 3))
    _, coef = predict(level.lmin, level.lmax, nsteps=degree - 1)
    dinv = level.inv_diag[:, None]
    for x0 in (np.zeros_like(b), rng.standard_normal((n, 3))):
        xp, x = x0, x0 + coef[0] * (dinv * (b - A @ x0))
        for c1, c2 in coef[2:].reshape(-1, 2):
            x, xp = x + c1 * (x - xp) + c2 * (dinv * (b - A @ x)), x
        ref = amg_vcycle_twin.chebyshev(level, b, x0, degree)
        assert np.linalg.norm(x - ref) <= 1e-13 * np.linalg.norm(ref), degree


# ------------------------------------------------------------------ plans
def _interval_planning(n, rel_tol=1e-13):
    """lmin for lmax = 2 whose planned step count is n, well away from the integer boundary of the log quotient"""
    lo, hi = 1e-8, 1.999                       # the quotient falls as lmin grows
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if tw.log_quotient(mid, 2.0, rel_tol) > n - 1.5:
            lo = mid
        else:
            hi = mid
    return lo


def test_plans_equal_the_parent_on_a_grid():
    lmins = [0.5, 0.45, 0.1, 0.02, 2e-4, 1.9999, 2.0 - 1e-13, _interval_planning(200), _interval_planning(201), _interval_planning(27)]
    seen = set()
    for lmin, rel_tol, max_iter in itertools.product(lmins, (1e-13, 1e-8, 1e-3), (1, 2, 26, 27, 28, 40, 199, 200, 201, 500, 4000)):
        q = tw.log_quotient(lmin, 2.0, rel_tol) if 2.0 - lmin > 1e-9 else 0.5
        assert abs(q - round(q)) > 1e-9, (lmin, rel_tol)
        planned, to_cg, budgets = tw.solve_plan(lmin, 2.0, rel_tol, max_iter)
        w, _ = predict(lmin, 2.0, rel_tol, max_iter)
        assert (w[tw.PLANNED], w[tw.TO_CG], w[tw.ROUNDS]) == (planned, int(to_cg), len(budgets)), (lmin, rel_tol, max_iter)
        assert w[tw.BUDGET0:tw.BUDGET0 + 4] == budgets + [0] * (4 - len(budgets)), (lmin, rel_tol, max_iter)
        if not to_cg:
            assert 1 + sum(budgets) <= max(max_iter, planned)
        seen.add((planned, max_iter, to_cg))
    # the thresholds themselves: 200 steps are Chebyshev's, 201 are CG's; planned == max_iter runs, planned == max_iter + 1 does not
    assert (200, 500, False) in seen and (201, 500, True) in seen and (200, 200, False) in seen and (200, 199, True) in seen
    assert (27, 27, False) in seen and (27, 26, True) in seen and (201, 201, True) in seen


# ------------------------------------------------------------------ brackets
def _fem(N):                                   # the matrices of tests/test_gpu_kernels.py::_fem
    h = 1.0 / (N - 1)
    main = np.full(N, 4 * h / 6)
    main[[0, -1]] = 2 * h / 6
    M = sp.diags([np.full(N - 1, h / 6), main, np.full(N - 1, h / 6)], [-1, 0, 1], format="csr")
    kd = np.full(N, 2 / h)
    kd[[0, -1]] = 1 / h
    K = sp.diags([np.full(N - 1, -1 / h), kd, np.full(N - 1, -1 / h)], [-1, 0, 1], format="csr")
    return M, K


def _gershgorin(A):
    """Gershgorin's bound on the spectrum of D^-1 A from the circles of the symmetrically scaled D^-1/2 A D^-1/2 (the same spectrum);
    for these matrices it lies above 1.05 x the largest Ritz value, so the widening rule decides lmax"""
    d = 1.0 / np.sqrt(A.diagonal())
    return float(np.max(np.asarray(abs(sp.diags(d) @ A @ sp.diags(d)).sum(axis=1)).ravel()))


def _gershgorin_rows(A):
    """the bound hfmi_csr_create computes: max_i sum_j |a_ij| / a_ii; it binds (1.5 for the mass matrices)"""
    return float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / A.diagonal()))


@pytest.fixture(scope="module")
def cg_runs():
    runs = {}
    for name, A in (("mass 50", _fem(50)[0]), ("mass 1500", _fem(1500)[0]), ("stiff 1500", (_fem(1500)[0] + 1e-4 * _fem(1500)[1]).tocsr())):
        rz, pap = tw.jacobi_cg_products(A, np.random.default_rng(1).standard_normal(A.shape[0]))
        runs[name] = (rz, pap, _gershgorin(A), _gershgorin_rows(A))
    return runs


@pytest.mark.parametrize("name", ["mass 50", "mass 1500", "stiff 1500"])
def test_bracket_of_a_jacobi_cg_run(cg_runs, name):
    rz, pap, gersh, gersh_rows = cg_runs[name]
    assert len(pap) >= 3
    assert bracket(rz, pap, gersh_rows)[0] == tw.OK and bracket(rz, pap, gersh_rows)[3:] == tw.bracket(rz, pap, gersh_rows)[3:]
    assert bracket(rz, pap, gersh_rows)[4] == gersh_rows                   # the bound of the library's own matrices binds
    refusal, tmin, tmax, lmin, lmax = bracket(rz, pap, gersh)
    assert refusal == tw.OK
    a, b = tw.lanczos_matrix(list(rz[:-1] / pap), list(rz[1:] / rz[:-1]))
    ev = np.linalg.eigvalsh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
    print(name, "Ritz values against eigvalsh:", abs(tmin - ev[0]) / ev[0], abs(tmax - ev[-1]) / ev[-1])
    assert abs(tmin - ev[0]) <= 1e-12 * ev[0] and abs(tmax - ev[-1]) <= 1e-12 * ev[-1]
    t_ref = tw.bracket(rz, pap, gersh)
    assert abs(tmin - t_ref[1]) <= 1e-13 * tmin and abs(tmax - t_ref[2]) <= 1e-13 * tmax
    assert lmin == 0.9 * tmin and lmax == (min(gersh, 1.05 * tmax) if min(gersh, 1.05 * tmax) >= tmax else tmax * (1.0 + 1e-9))      # the widening, exactly
    w, _ = predict(lmin, lmax, rel_tol=1e-13, max_iter=500)
    if name.startswith("mass"):
        assert lmin <= 0.5 and 1.5 <= lmax                      # the spectrum of D^-1 M for P1 elements
        assert (w[tw.PLANNED], w[tw.TO_CG]) == (27, 0)
    else:
        assert (w[tw.PLANNED], w[tw.TO_CG]) == (476, 1)


def test_bracket_refusals(cg_runs):
    rz, pap, gersh, _ = cg_runs["mass 50"]
    assert bracket(rz[:3], pap[:2], gersh)[0] == tw.TOO_SHORT == tw.bracket(rz[:3], pap[:2], gersh)[0]
    assert bracket(rz[:1], pap[:0], gersh)[0] == tw.TOO_SHORT
    assert bracket(rz[:4], pap[:3], gersh)[0] == tw.OK
    for bad in (0.0, -1.0, float("nan")):
        p = pap.copy()
        p[4] = bad
        assert bracket(rz, p, gersh)[0] == tw.NOT_SPD == tw.bracket(rz, p, gersh)[0]
    r = rz.copy()
    r[5] = float("inf")
    assert bracket(r, pap, gersh)[0] == tw.NOT_SPD == tw.bracket(r, pap, gersh)[0]
    for g in (0.0, -2.0, float("nan")):
        assert bracket(rz, pap, g)[0] == tw.NO_GERSHGORIN == tw.bracket(rz, pap, g)[0]
        assert bracket(rz, np.zeros_like(pap), g)[0] == tw.NO_GERSHGORIN        # Gershgorin is asked first, as in cheb_estimate
    # a Gershgorin bound below the largest Ritz value (it cannot be, for an SPD matrix): the bracket still holds the Ritz value
    refusal, tmin, tmax, lmin, lmax = bracket(rz, pap, 1.2)
    assert refusal == tw.OK and tmax > 1.2 and lmax == tmax * (1.0 + 1e-9)
    assert (refusal, lmin, lmax) == tw.bracket(rz, pap, 1.2)[:1] + (0.9 * tmin, tmax * (1.0 + 1e-9))


# ------------------------------------------------------------------ step plans
def test_step_plans_equal_the_parent_and_cover_every_row():
    checked = 0
    for threadmap, unr in itertools.product((0, 1), (0, 1, 2, 3, 4, 8)):
        for nrows, resid, k in itertools.product((1, 3, 4, 5, 1000, 6001), (0, 1), range(1, 301)):
            w, _ = predict(0.5, 2.0, nrows=nrows, k=k, resid=resid, knobs=(0, threadmap, unr))
            wave, u, grid = tw.step_plan(nrows, k, resid, threadmap, unr)
            assert (w[tw.WAVE], w[tw.UNR], w[tw.GRID]) == (wave, u, grid), (nrows, k, resid, threadmap, unr)
            assert grid % 8 == 0 and grid >= 8
            rows_per_workgroup = 4 * u if wave else (256 // k if k <= 256 else 1)
            assert grid * rows_per_workgroup >= nrows > (grid - 8) * rows_per_workgroup
            assert w[tw.KNOB0:tw.KNOB0 + 3] == [0, threadmap, unr if unr in (2, 4) else 1]
            if wave:
                assert k % 2 == 0 and k <= 128 and not threadmap and u in (1, 2, 4) and (u == 1 or not resid)
            checked += 1
    assert checked == 12 * 6 * 2 * 300


def test_bad_arguments_and_bindings():
    for bad in ((0.0, 2.0), (-1.0, 2.0), (2.0, 1.0), (float("nan"), 1.0)):
        with pytest.raises(L.HfmiError):
            predict(*bad)
    with pytest.raises(L.HfmiError):
        predict(0.5, 2.0, k=0)
    assert "hfmi_cheb_rules_predict" in L.SIGNATURES and "hfmi_lanczos_bracket_predict" in L.SIGNATURES
