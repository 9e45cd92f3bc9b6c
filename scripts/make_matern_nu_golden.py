"""Writes tests/golden/matern_nu_phi.npz: the Matern correlation of smoothness nu,
phi_nu(a) = 2^(1-nu) / Gamma(nu) a^nu K_nu(a), correctly rounded to fp64 from mpmath at 50 digits, and for every nu the table words
of the device evaluation (csrc/hfmi_kcov_nu.h) computed by mpmath, which the tables of ``hfmi_kernel_matern_tables`` (long double
on the host) are held to.  The tests read the file; only this script needs mpmath.

  nu:      0.125, 0.3, 0.5, 0.75, 1, 1 + 2^-30, 1.25, 1.4999, 1.5, 2, 2.000001, 2.5, 3.2, 4.5, 6, 7.49, 8
           (both ends, the ties mu = -1/2, the integers mu = 0, a tiny |mu|, a near-tie)
  a:       {0}, geomspace(1e-9, 2, 120), 2 and its three fp64 neighbours on either side, linspace(1.5, 2.5, 121),
           geomspace(2, 700, 150), 750 and 1e4: 402 for each nu
  phi:     (nu, a), 1 at a = 0 (values below the smallest subnormal round to 0)
  tables:  (nu, 162) words in the layout of tests/helpers/matern_nu_twin.py

Usage:  python scripts/make_matern_nu_golden.py
"""
import os

import mpmath as mp
import numpy as np

NSER = 16
NCHEB = 25
WORDS = 16 + 6 * NSER + 2 * NCHEB

NUS = (0.125, 0.3, 0.5, 0.75, 1.0, 1.0 + 2.0 ** -30, 1.25, 1.4999, 1.5, 2.0, 2.000001, 2.5, 3.2, 4.5, 6.0, 7.49, 8.0)


def abscissae():
    near = [2.0]
    lo = hi = 2.0
    for _ in range(3):
        lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 3.0)
        near += [lo, hi]
    return np.concatenate([[0.0], np.geomspace(1e-9, 2.0, 120), np.sort(near), np.linspace(1.5, 2.5, 121), np.geomspace(2.0, 700.0, 150),
                           [750.0, 1e4]])


def phi_exact(nu, a):
    """phi_nu at the fp64 numbers nu and a, as an mpf"""
    nu, x = mp.mpf(float(nu)), mp.mpf(float(a))
    if x == 0:
        return mp.mpf(1)
    return mp.mpf(2) ** (1 - nu) / mp.gamma(nu) * x ** nu * mp.besselk(nu, x)


def tables(nu):
    """the table words of smoothness nu (an fp64 number) as mpf's; the C++ builder states the same quantities in long double"""
    nu = mp.mpf(float(nu))
    n = int(mp.floor(nu + mp.mpf(1) / 2))
    mu = nu - n
    T = [mp.mpf(0)] * WORDS
    rg = lambda z: mp.rgamma(z)          # noqa: E731
    if mu == 0:
        g1 = -mp.euler
        c0 = mp.mpf(1)
    else:
        g1 = (rg(1 - mu) - rg(1 + mu)) / (2 * mu)
        c0 = mu * mp.pi / mp.sin(mu * mp.pi)
    g2 = (rg(1 - mu) + rg(1 + mu)) / 2
    hp = mp.gamma(1 + mu) / 2
    hq = mp.gamma(1 - mu) / 2
    T[0], T[1], T[2], T[3], T[4], T[5] = mp.mpf(n), mu, hp, hq, c0 * g1, c0 * g2
    T[6] = 2 / mp.gamma(nu)
    T[7] = mp.mpf(2) ** (1 - nu) / mp.gamma(nu)
    T[8] = mp.sqrt(2 * nu)
    T[9] = nu
    # f_k = A_k f_0 + B_k p_0 + C_k q_0,  p_k = P_k p_0,  q_k = Q_k q_0
    A, B, C, P, Q = mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(1), mp.mpf(1)
    fact = mp.mpf(1)
    for k in range(NSER):
        if k > 0:
            den = k * k - mu * mu
            A, B, C = k * A / den, (k * B + P) / den, (k * C + Q) / den
            P, Q = P / (k - mu), Q / (k + mu)
            fact *= k
        T[16 + k] = A / fact
        T[16 + NSER + k] = hp * B / fact
        T[16 + 2 * NSER + k] = C / fact
        T[16 + 3 * NSER + k] = -k * A / fact
        T[16 + 4 * NSER + k] = hp * (P - k * B) / fact
        T[16 + 5 * NSER + k] = -k * C / fact
    # Chebyshev interpolants of sqrt(a) e^a K_mu(a) and of the same with mu + 1, in t = 2 / a on [0, 1], at the 25 roots of T_25
    nodes = [(1 + mp.cos(mp.pi * (k + mp.mpf(1) / 2) / NCHEB)) / 2 for k in range(NCHEB)]
    for which in range(2):
        order = mu + which
        f = [mp.sqrt(2 / t) * mp.exp(2 / t) * mp.besselk(order, 2 / t) for t in nodes]
        for j in range(NCHEB):
            c = 2 * sum(f[k] * mp.cos(mp.pi * j * (k + mp.mpf(1) / 2) / NCHEB) for k in range(NCHEB)) / NCHEB
            T[16 + 6 * NSER + which * NCHEB + j] = c / 2 if j == 0 else c
    return T


def main():
    mp.mp.dps = 50
    a = abscissae()
    nus = np.array(NUS)
    phi = np.empty((nus.size, a.size))
    tab = np.empty((nus.size, WORDS))
    for i, nu in enumerate(nus):
        phi[i] = [float(phi_exact(nu, v)) for v in a]
        tab[i] = [float(w) for w in tables(nu)]
        print("nu = %.10g done" % nu, flush=True)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "matern_nu_phi.npz")
    np.savez(out, nu=nus, a=a, phi=phi, tables=tab)
    print("wrote", os.path.normpath(out), nus.size, "x", a.size, "values")


if __name__ == "__main__":
    main()
