"""Writes tests/golden/matern1_phi.npz: the Matern-1 correlation phi(a) = a K_1(a), correctly rounded to fp64 from mpmath at 40
digits, on the abscissae the tests of the device function and its numpy twin share.  The tests read the file; only this script
needs mpmath.

  a:    {0}, geomspace(1e-12, 2, 600), linspace(1.5, 2.5, 401) (across the switch of the two evaluation schemes at a = 2),
        geomspace(2, 700, 600), 750 and 1e4
  phi:  a K_1(a), 1 at a = 0 (values below the smallest subnormal round to 0)

Usage:  python tests/golden/make_matern1_golden.py
"""
import os

import mpmath as mp
import numpy as np


def abscissae():
    return np.concatenate([[0.0], np.geomspace(1e-12, 2.0, 600), np.linspace(1.5, 2.5, 401), np.geomspace(2.0, 700.0, 600), [750.0, 1e4]])


def main():
    mp.mp.dps = 40
    a = abscissae()
    phi = np.empty_like(a)
    for i, v in enumerate(a):
        if v == 0.0:
            phi[i] = 1.0
        else:
            x = mp.mpf(float(v))          # the fp64 abscissa, exactly
            phi[i] = float(x * mp.besselk(1, x))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "matern1_phi.npz")
    np.savez(out, a=a, phi=phi)
    print("wrote", out, a.size, "abscissae")


if __name__ == "__main__":
    main()
