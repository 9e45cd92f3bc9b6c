"""numpy twin of the device function ``kcov_k1_phi`` (hippyflow_amd/csrc/hfmi_kcov_k1.h): the Matern-1 correlation
phi(a) = a K_1(a), phi(0) = 1, with the same operations in the same order.  What differs on the device: the compiler contracts
``x * y + z`` into one fma, and ``log`` / ``exp`` / ``sqrt`` are the device's.  The tables are the output of
scripts/make_matern1_coeffs.py (mpmath, 50 digits), pasted here and into the header.

  a <= 2:  phi = 1 + y (2 ln(a / 2) S1(y) - S2(y)),  y = a^2 / 4, both series by Horner from the highest term
  a >  2:  phi = sqrt(a) exp(-a) g(2 / a),  g by Clenshaw's recurrence in u = 2 t - 1, t = 2 / a
"""
import numpy as np

EPS = np.finfo(np.float64).eps

K1_S1 = (
    1.0000000000000000000,
    5.0000000000000000000e-1,
    8.3333333333333333333e-2,
    6.9444444444444444444e-3,
    3.4722222222222222222e-4,
    1.1574074074074074074e-5,
    2.7557319223985890653e-7,
    4.9209498614260519022e-9,
    6.8346525853139609753e-11,
    7.5940584281266233059e-13,
    6.9036894801151120963e-15,
    5.2300677879659940123e-17,
    3.3526075563884577002e-19,
    1.8420920639497020331e-21,
)
K1_S2 = (
    -1.5443132980306572121e-1,
    6.7278433509846713939e-1,
    1.8157516696085563434e-1,
    1.9182189839330562121e-2,
    1.1153594919665281061e-3,
    4.1422476892711430696e-5,
    1.0715459140911808686e-6,
    2.0452860035938779413e-8,
    3.0020487465891878859e-10,
    3.4959287296928819208e-12,
    3.3099147352502720680e-14,
    2.5986411321011287351e-16,
    1.7195232826992565241e-18,
    9.7212075188236180165e-21,
)
K1_CHEB = (
    1.3603130952422213347,
    1.0392373657681723844e-1,
    -2.8578168596227793868e-3,
    1.9521551847135163111e-4,
    -1.9361979741660829600e-5,
    2.4064849478372171171e-6,
    -3.5019606030878125421e-7,
    5.7410841254500492923e-8,
    -1.0345762465678097027e-8,
    2.0150497551970346161e-9,
    -4.1903547593419255842e-10,
    9.2183151876053141258e-11,
    -2.1299678384277910216e-11,
    5.1396396734823435404e-12,
    -1.2891739609498229352e-12,
    3.3484196660522431201e-13,
    -8.9767051820101460692e-14,
    2.4771544242195986813e-14,
    -7.0198370892147688513e-15,
    2.0387031662398608799e-15,
    -6.0570472706430178228e-16,
    1.8380935752430454256e-16,
    -5.6894628491936483743e-17,
    1.7940510478863572914e-17,
    -5.7567444820733024503e-18,
)


def _small(a):
    """the series side; a > 0"""
    y = 0.25 * (a * a)
    s1 = np.full_like(a, K1_S1[-1])
    s2 = np.full_like(a, K1_S2[-1])
    for k in range(len(K1_S1) - 2, -1, -1):
        s1 = s1 * y + K1_S1[k]
        s2 = s2 * y + K1_S2[k]
    lg = np.log(0.5 * a)
    return y * ((2.0 * lg) * s1 - s2) + 1.0


def _large(a):
    """the scaled side; a > 2"""
    t = 2.0 / a
    u2 = 4.0 * t - 2.0          # 2 u, u = 2 t - 1
    b1 = np.zeros_like(a)
    b2 = np.zeros_like(a)
    for j in range(len(K1_CHEB) - 1, 0, -1):
        b1, b2 = (u2 * b1 - b2) + K1_CHEB[j], b1
    g = ((0.5 * u2) * b1 - b2) + K1_CHEB[0]
    return (np.sqrt(a) * np.exp(-a)) * g


def phi(a):
    """a K_1(a) for an array of a >= 0; exactly 1 at a = 0"""
    a = np.asarray(a, dtype=np.float64)
    out = np.ones_like(a)
    lo = (a > 0.0) & (a <= 2.0)
    hi = a > 2.0
    with np.errstate(under="ignore"):
        out[lo] = _small(a[lo])
        out[hi] = _large(a[hi])
    return out
