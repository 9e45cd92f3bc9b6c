"""The decisions of the sparse SPD solves as the drivers made them before hippyflow_amd/csrc/hfmi_spsolve_rules.h existed, restated
in Python with one comment per rule naming the line of the parent commit (6a365d6: hfmi_cheb.hip, hfmi_amg.hip) it restates.
tests/test_spsolve_rules_cpu.py holds ``hfmi_cheb_rules_predict`` / ``hfmi_lanczos_bracket_predict`` (include/hfmi.h) to this twin."""
import math

import numpy as np

WORDS = 13
PLANNED, TO_CG, ROUNDS, BUDGET0, WAVE, UNR, GRID, KNOB0 = 0, 1, 2, 3, 7, 8, 9, 10
OK, NO_GERSHGORIN, NOT_SPD, TOO_SHORT, TMIN, TMAX = range(6)


def coefficients(lmin, lmax, nsteps):
    """1 / theta, spread, [(c1, c2)] of the steps after the first"""
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)     # hfmi_cheb.hip:344, hfmi_amg.hip:249
    spread = delta > 1e-12 * theta                              # hfmi_cheb.hip:359
    out = []
    if spread:
        rho = delta / theta                                     # hfmi_cheb.hip:360, hfmi_amg.hip:250
        for _ in range(nsteps):
            rho_new = 1.0 / (2.0 * theta / delta - rho)         # hfmi_cheb.hip:375, hfmi_amg.hip:264
            out.append((rho_new * rho, 2.0 * rho_new / delta))  # hfmi_cheb.hip:376, hfmi_amg.hip:265
            rho = rho_new                                       # hfmi_cheb.hip:377, hfmi_amg.hip:266
    return 1.0 / theta, spread, out                             # hfmi_cheb.hip:357, hfmi_amg.hip:256, 259


def log_quotient(lmin, lmax, rel_tol):
    sk = math.sqrt(lmax / lmin)
    c = (sk - 1.0) / (sk + 1.0)                                 # hfmi_cheb.hip:363
    return math.log(2.0 / rel_tol) / -math.log(c)               # hfmi_cheb.hip:364


def solve_plan(lmin, lmax, rel_tol, max_iter):
    """(planned, to_cg, [budget of every round that runs]) of cheb_solve"""
    _, spread, _ = coefficients(lmin, lmax, 0)
    planned = 1                                                 # hfmi_cheb.hip:361
    if spread:
        planned = int(math.ceil(log_quotient(lmin, lmax, rel_tol))) + 1        # hfmi_cheb.hip:364
    if planned > max_iter or planned > 200:                     # hfmi_cheb.hip:366
        return planned, True, []
    budgets, steps = [], 1                                      # hfmi_cheb.hip:358
    budget = planned - 1                                        # hfmi_cheb.hip:372
    for _ in range(4):                                          # hfmi_cheb.hip:373
        budgets.append(budget)
        steps += budget                                         # hfmi_cheb.hip:374
        if not spread:                                          # hfmi_cheb.hip:405
            break
        budget = max(2, planned // 3)                           # hfmi_cheb.hip:406
        if steps + budget > max_iter:                           # hfmi_cheb.hip:407
            break
    return planned, False, budgets


def sturm_count(a, b, x):                                       # hfmi_cheb.hip:240-250
    cnt = 0
    q = a[0] - x
    if q < 0:
        cnt += 1
    for i in range(1, len(a)):
        if q == 0.0:
            q = 1e-300
        q = a[i] - x - b[i - 1] * b[i - 1] / q
        if q < 0:
            cnt += 1
    return cnt


def tridiag_extremes(a, b):                                     # hfmi_cheb.hip:251-271
    m = len(a)
    lo = hi = a[0]
    for i in range(m):
        rad = (abs(b[i - 1]) if i > 0 else 0.0) + (abs(b[i]) if i + 1 < m else 0.0)
        lo, hi = min(lo, a[i] - rad), max(hi, a[i] + rad)
    ends = []
    for target in (1, m):
        l, h = lo, hi
        it = 0
        while it < 200 and h - l > 1e-14 * max(abs(l), abs(h)):
            mid = 0.5 * (l + h)
            if sturm_count(a, b, mid) >= target:
                h = mid
            else:
                l = mid
            it += 1
        ends.append(0.5 * (l + h))
    return ends[0], ends[1]


def lanczos_matrix(alpha, beta):                                # hfmi_cheb.hip:316-320
    m = len(alpha)
    a = [1.0 / alpha[i] + (beta[i - 1] / alpha[i - 1] if i > 0 else 0.0) for i in range(m)]
    b = [math.sqrt(beta[i]) / alpha[i] for i in range(m - 1)]
    return a, b


def bracket(rz, pap, gersh_lmax):
    """(refusal, tmin, tmax, lmin, lmax) of cheb_estimate for the inner products of a scalar CG run (rz: m + 1 values, pap: m)"""
    if not gersh_lmax > 0.0:                                    # hfmi_cheb.hip:280
        return NO_GERSHGORIN, 0.0, 0.0, 0.0, 0.0
    alpha, beta = [], []
    for i in range(len(pap)):
        if not pap[i] > 0.0 or not math.isfinite(rz[i + 1]):    # hfmi_cheb.hip:308
            return NOT_SPD, 0.0, 0.0, 0.0, 0.0
        alpha.append(rz[i] / pap[i])                            # hfmi_cheb.hip:309
        beta.append(rz[i + 1] / rz[i])                          # hfmi_cheb.hip:310
    if len(alpha) < 3:                                          # hfmi_cheb.hip:315
        return TOO_SHORT, 0.0, 0.0, 0.0, 0.0
    tmin, tmax = tridiag_extremes(*lanczos_matrix(alpha, beta))  # hfmi_cheb.hip:322
    if not tmin > 0.0:                                          # hfmi_cheb.hip:323
        return TMIN, tmin, tmax, 0.0, 0.0
    if not tmax >= tmin:                                        # hfmi_cheb.hip:323
        return TMAX, tmin, tmax, 0.0, 0.0
    lmin = 0.9 * tmin                                           # hfmi_cheb.hip:325
    lmax = min(gersh_lmax, 1.05 * tmax)                         # hfmi_cheb.hip:326
    if lmax < tmax:                                             # hfmi_cheb.hip:327
        lmax = tmax * (1.0 + 1e-9)
    return OK, tmin, tmax, lmin, lmax


def step_plan(nrows, k, resid, threadmap, unr):
    """(wave, rows per wave, workgroups) of launch_cheb_step; unr as the environment gave it (any integer)"""
    if k % 2 == 0 and k <= 128 and not threadmap:               # hfmi_cheb.hip:203
        u = 1 if resid or unr not in (2, 4) else unr            # hfmi_cheb.hip:209-212
        gw = (nrows + 4 * u - 1) // (4 * u)                     # hfmi_cheb.hip:206, 209, 212
        return 1, u, (gw + 7) // 8 * 8                          # hfmi_cheb.hip:207
    rows_per_pass = 256 // k if k <= 256 else 1                 # hfmi_cheb.hip:217
    g = (nrows + rows_per_pass - 1) // rows_per_pass            # hfmi_cheb.hip:218
    return 0, 1, (g + 7) // 8 * 8                               # hfmi_cheb.hip:219


def jacobi_cg_products(A, rhs, iters=60):
    """r.z (one more than iterations) and p.Ap of a scalar Jacobi-CG run in numpy: cheb_estimate's loop (hfmi_cheb.hip:289-313)"""
    dinv = 1.0 / A.diagonal()
    r = rhs.copy()
    z = dinv * r
    p = z.copy()
    rz = [float(r @ z)]
    pap = []
    for _ in range(iters):
        if not rz[-1] > 1e-28 * rz[0]:
            break
        ap = A @ p
        pap.append(float(p @ ap))
        r = r - (rz[-1] / pap[-1]) * ap
        z = dinv * r
        rz.append(float(r @ z))
        p = z + (rz[-1] / rz[-2]) * p
    return np.array(rz), np.array(pap)
