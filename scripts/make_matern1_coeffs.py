"""Coefficients of the Matern-1 correlation phi(a) = a K_1(a) (hippyflow_amd/csrc/hfmi_kcov_k1.h and its numpy twin
tests/helpers/matern1_twin.py), computed with mpmath at 50 digits and printed as literals to paste into both.

  a <= 2:  phi = 1 + y (2 ln(a / 2) S1(y) - S2(y)),  y = a^2 / 4,
           S1 = sum_k y^k / (k! (k+1)!),  S2 = sum_k (psi(k+1) + psi(k+2)) y^k / (k! (k+1)!),  k < NSER
  a >  2:  phi = sqrt(a) exp(-a) g(2 / a),  g(t) = sum_j c_j T_j(2 t - 1)  the Chebyshev interpolant of sqrt(a) e^a K_1(a) on t in [0, 1]

Usage:  python scripts/make_matern1_coeffs.py          prints the three tables (C initialisers; the same digits serve numpy)
"""
import mpmath as mp

NSER = 14        # terms of the two power series
DEG = 24         # degree of the Chebyshev interpolant
NODES = 96       # Chebyshev-Gauss nodes the coefficients are computed from (aliasing from degree > 2 NODES - DEG: far below 1e-30)


def series_tables():
    s1, s2 = [], []
    for k in range(NSER):
        den = mp.factorial(k) * mp.factorial(k + 1)
        s1.append(1 / den)
        s2.append((mp.digamma(k + 1) + mp.digamma(k + 2)) / den)
    return s1, s2


def g(t):
    """sqrt(a) e^a K_1(a) at a = 2 / t; sqrt(pi / 2) at t = 0"""
    if t == 0:
        return mp.sqrt(mp.pi / 2)
    a = 2 / t
    return mp.sqrt(a) * mp.besselk(1, a) * mp.exp(a)


def cheb_table():
    th = [mp.pi * (mp.mpf(k) + mp.mpf(1) / 2) / NODES for k in range(NODES)]
    f = [g((mp.cos(x) + 1) / 2) for x in th]
    c = []
    for j in range(DEG + 1):
        s = mp.fsum(f[k] * mp.cos(j * th[k]) for k in range(NODES))
        c.append(2 * s / NODES)
    c[0] /= 2        # g = c_0 + sum_{j >= 1} c_j T_j
    return c


def literal(x):
    return mp.nstr(x, 20, strip_zeros=False, min_fixed=-1, max_fixed=1)


def main():
    mp.mp.dps = 50
    s1, s2 = series_tables()
    c = cheb_table()
    for name, tab in (("K1_S1", s1), ("K1_S2", s2), ("K1_CHEB", c)):
        print("%s[%d] = {" % (name, len(tab)))
        for v in tab:
            print("    %s," % literal(v))
        print("};")


if __name__ == "__main__":
    main()
