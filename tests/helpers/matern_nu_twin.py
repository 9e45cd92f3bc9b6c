"""numpy twin of the device function ``kcov_nu_phi`` (hippyflow_amd/csrc/hfmi_kcov_nu.h): the Matern correlation of any smoothness,
phi_nu(a) = 2^(1-nu) / Gamma(nu) a^nu K_nu(a), phi_nu(0) = 1, with the same operations in the same order.  What differs on the device:
the compiler contracts ``x * y + z`` into one fma, and ``log`` / ``exp`` / ``sqrt`` are the device's.  The tables are an ARGUMENT:
the words of ``hfmi_kernel_matern_tables`` (or the mpmath tables of scripts/make_matern_nu_golden.py, which have the same layout).

  n = floor(nu + 1/2),  mu = nu - n in [-1/2, 1/2)
  a <= 2:  Temme's series on the scaled S_j = (a/2)^(mu+j) K_(mu+j):  S_0 = PA(y) wf0 + PB(y) + PC(y) wq0,  S_1 likewise from QA, QB, QC,
           y = a^2 / 4;  S_(j+1) = y S_(j-1) + (mu + j) S_j;  phi = (2 / Gamma(nu)) S_n
  a >  2:  G_0, G_1 = sqrt(a) e^a K_mu, K_(mu+1) by Clenshaw in t = 2 / a;  H_0 = G_0, H_1 = a G_1,  H_(j+1) = a^2 H_(j-1) + 2 (mu + j) H_j;
           phi = ((cc H_n) a^(mu - 1/2)) e^(-a)
"""
import numpy as np

EPS = np.finfo(np.float64).eps

# layout of the table words (HFMI_MATERN_TABLE_WORDS of include/hfmi.h)
NSER = 16
NCHEB = 25
W_N, W_MU, W_HP, W_HQ, W_G1, W_G2, W_CS, W_CC, W_CA, W_NU = range(10)
W_PA = 16
W_PB, W_PC, W_QA, W_QB, W_QC = (W_PA + NSER * i for i in range(1, 6))
W_CH0 = W_PA + 6 * NSER
W_CH1 = W_CH0 + NCHEB
WORDS = W_CH1 + NCHEB          # 162
A_MAX = 1.0e5                  # abscissae are clamped here: exp(-a) is +0 long before, and a^(2 n) stays finite


def _horner(T, off, y):
    s = np.full_like(y, T[off + NSER - 1])
    for k in range(NSER - 2, -1, -1):
        s = s * y + T[off + k]
    return s


def _small(T, a):
    """the series side; 0 < a <= 2"""
    n, mu = int(T[W_N]), T[W_MU]
    y = 0.25 * (a * a)
    L = np.log(0.5 * a)
    s = -(mu * L)
    w = np.exp(mu * L)
    iw = np.exp(s)
    s2 = s * s
    # sinh(s) / s: its series below 1/4 (the difference of the exponentials cancels there), the exponentials beyond
    ser = 1.0 + s2 * (1.0 / 6.0 + s2 * (1.0 / 120.0 + s2 * (1.0 / 5040.0 + s2 * (1.0 / 362880.0 + s2 * (1.0 / 39916800.0)))))
    with np.errstate(divide="ignore", invalid="ignore"):
        big = (iw - w) / (2.0 * s)
    shs = np.where(np.abs(s) < 0.25, ser, big)
    ch = 0.5 * (iw + w)
    wf0 = w * (ch * T[W_G1] - (L * shs) * T[W_G2])
    wq0 = (w * w) * T[W_HQ]
    S0 = (_horner(T, W_PA, y) * wf0 + _horner(T, W_PC, y) * wq0) + _horner(T, W_PB, y)
    if n == 0:
        return T[W_CS] * S0
    S1 = (_horner(T, W_QA, y) * wf0 + _horner(T, W_QC, y) * wq0) + _horner(T, W_QB, y)
    for j in range(1, n):
        S0, S1 = S1, y * S0 + (mu + j) * S1
    return T[W_CS] * S1


def _clenshaw(T, off, u2):
    b1 = np.zeros_like(u2)
    b2 = np.zeros_like(u2)
    for j in range(NCHEB - 1, 0, -1):
        b1, b2 = (u2 * b1 - b2) + T[off + j], b1
    return ((0.5 * u2) * b1 - b2) + T[off]


def _large(T, a):
    """the scaled side; a > 2"""
    n, mu = int(T[W_N]), T[W_MU]
    a = np.minimum(a, A_MAX)
    t = 2.0 / a
    u2 = 4.0 * t - 2.0          # 2 u, u = 2 t - 1
    H0 = _clenshaw(T, W_CH0, u2)
    if n > 0:
        H1 = a * _clenshaw(T, W_CH1, u2)
        a2 = a * a
        for j in range(1, n):
            H0, H1 = H1, a2 * H0 + (2.0 * (mu + j)) * H1
        H0 = H1
    pw = np.exp((mu - 0.5) * np.log(a))
    return ((T[W_CC] * H0) * pw) * np.exp(-a)


def phi(T, a):
    """phi_nu(a) for an array of a >= 0 with the table words T; exactly 1 at a = 0"""
    T = np.asarray(T, dtype=np.float64)
    assert T.shape == (WORDS,)
    a = np.asarray(a, dtype=np.float64)
    out = np.ones_like(a)
    lo = (a > 0.0) & (a <= 2.0)
    hi = a > 2.0
    with np.errstate(under="ignore"):
        out[lo] = _small(T, a[lo])
        out[hi] = _large(T, a[hi])
    return out
