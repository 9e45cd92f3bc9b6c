// Host-side tables of the Matern family of any smoothness (HFMI_KERNEL_MATERN; the device evaluation is hfmi_kcov_nu.h, which states
// the scheme).  Everything that depends on nu is computed here, once per operator, in long double; no device and no context.
//
//   n = floor(nu + 1/2),  mu = nu - n in [-1/2, 1/2)
//   words 0..9:  n, mu, Gamma(1 + mu) / 2, Gamma(1 - mu) / 2, c0 Gamma_1(mu), c0 Gamma_2(mu) (c0 = mu pi / sin(mu pi)), 2 / Gamma(nu),
//                2^(1 - nu) / Gamma(nu), sqrt(2 nu), nu;  10..15: zero
//   16..111:     six polynomials in y = a^2 / 4 of KNU_NSER terms each.  Temme's recurrences f_k = (k f_(k-1) + p_(k-1) + q_(k-1)) / (k^2 - mu^2),
//                p_k = p_(k-1) / (k - mu), q_k = q_(k-1) / (k + mu) are linear in (f_0, p_0, q_0): f_k = A_k f_0 + B_k p_0 + C_k q_0, p_k = P_k p_0.
//                With w = (a/2)^mu:  w K_mu = PA w f_0 + PB + PC w q_0 and (a/2) w K_(mu+1) = QA w f_0 + QB + QC w q_0, where
//                PA_k = A_k / k!, PB_k = hp B_k / k!, PC_k = C_k / k!, QA_k = -k A_k / k!, QB_k = hp (P_k - k B_k) / k!, QC_k = -k C_k / k!
//                and hp = w p_0 = Gamma(1 + mu) / 2 does not depend on a.
//   112..161:    the Chebyshev coefficients (c_0 halved) of the degree-24 interpolants of sqrt(a) e^a K_mu(a) and sqrt(a) e^a K_(mu+1)(a) in
//                t = 2 / a on [0, 1], at the roots of T_25; the values come from Steed's continued fraction (a >= 2 at every node).
// scripts/make_matern_nu_golden.py computes the same words by mpmath at 50 digits; tests/test_matern_nu_cpu.py compares.
#include <math.h>

#include "hfmi_internal.h"
#include "hfmi_kcov_nu.h"

// Gamma_1(mu) = (1 / Gamma(1 - mu) - 1 / Gamma(1 + mu)) / (2 mu).  With 1 / Gamma(z) = sum_k c_k z^k and Gamma(1 + z) = z Gamma(z) it is
// -(c_2 + c_4 mu^2 + c_6 mu^4 + ...), which is what is summed below 1/10 (the next term, c_20 mu^18, is under 1e-29 there; mu = 0 is the
// limit -gamma_Euler and no special case).  Beyond, the difference loses at most four bits of the 64.
static long double knu_gamma1(long double mu) {
  static const long double c[9] = {0.5772156649015328606065121L,    -0.04200263503409523552900393L,   -0.0421977345555443367482083L,
                                   0.00721894324666309954239501L,   -0.00021524167411495097281573L,   -0.00002013485478078823865568939L,
                                   0.00000113302723198169588237413L, 6.116095104481415817862499e-9L,  -1.181274570487020144588127e-9L};
  if (fabsl(mu) < 0.1L) {
    const long double m2 = mu * mu;
    long double s = c[8];
    for (int k = 7; k >= 0; --k) s = s * m2 + c[k];
    return -s;
  }
  return (1.0L / tgammal(1.0L - mu) - 1.0L / tgammal(1.0L + mu)) / (2.0L * mu);
}

// sqrt(x) e^x K_mu(x) and the same of order mu + 1 for x >= 2, |mu| <= 1/2: Steed's algorithm for the second continued fraction
// (Temme 1975; the x >= 2 branch of the classical bessik), without the factor sqrt(pi / 2x) e^-x it ends with
static void knu_steed_scaled(long double mu, long double x, long double* g0, long double* g1) {
  const long double a1 = 0.25L - mu * mu;
  long double b = 2.0L * (1.0L + x), d = 1.0L / b, h = d, delh = d, q1 = 0.0L, q2 = 1.0L, q = a1, c = a1, a = -a1;
  long double s = 1.0L + q * delh;
  for (int i = 2; i < 100000; ++i) {
    a -= 2 * (i - 1);
    c = -a * c / i;
    const long double qnew = (q1 - b * q2) / a;
    q1 = q2;
    q2 = qnew;
    q += c * qnew;
    b += 2.0L;
    d = 1.0L / (b + a * d);
    delh = (b * d - 1.0L) * delh;
    h += delh;
    const long double dels = q * delh;
    s += dels;
    if (fabsl(dels) <= 1e-21L * fabsl(s) && fabsl(delh) <= 1e-21L * fabsl(h)) break;
  }
  h = a1 * h;
  const long double k0 = sqrtl(M_PIl / 2.0L) / s;
  *g0 = k0;
  *g1 = k0 * (mu + x + 0.5L - h) / x;
}

extern "C" int hfmi_kernel_matern_tables(double nu_in, double* words) {
  if (!words) HFMI_FAIL(HFMI_ERR_INVALID, "kernel_matern_tables: null argument");
  if (!isfinite(nu_in) || nu_in < HFMI_MATERN_NU_MIN || nu_in > HFMI_MATERN_NU_MAX)
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_matern_tables: the smoothness nu = %g does not lie in [1/8, 8]", nu_in);
  const long double nu = nu_in;
  const int n = (int)floorl(nu + 0.5L);
  const long double mu = nu - n;      // exact: nu is an fp64 number
  long double T[KNU_WORDS];
  for (int i = 0; i < KNU_WORDS; ++i) T[i] = 0.0L;
  const long double rp = 1.0L / tgammal(1.0L + mu), rm = 1.0L / tgammal(1.0L - mu);
  const long double c0 = fabsl(mu) < 1e-12L ? 1.0L : mu * M_PIl / sinl(mu * M_PIl);
  const long double hp = 0.5L / rp;
  T[KNU_W_N] = n;
  T[KNU_W_MU] = mu;
  T[KNU_W_HP] = hp;
  T[KNU_W_HQ] = 0.5L / rm;
  T[KNU_W_G1] = c0 * knu_gamma1(mu);
  T[KNU_W_G2] = c0 * 0.5L * (rm + rp);
  T[KNU_W_CS] = 2.0L / tgammal(nu);
  T[KNU_W_CC] = exp2l(1.0L - nu) / tgammal(nu);
  T[KNU_W_CA] = sqrtl(2.0L * nu);
  T[KNU_W_NU] = nu;
  long double A = 1.0L, B = 0.0L, C = 0.0L, P = 1.0L, Q = 1.0L, fact = 1.0L;
  for (int k = 0; k < KNU_NSER; ++k) {
    if (k > 0) {
      const long double den = (long double)k * k - mu * mu;
      A = k * A / den, B = (k * B + P) / den, C = (k * C + Q) / den;
      P /= k - mu, Q /= k + mu;
      fact *= k;
    }
    T[KNU_W_PA + k] = A / fact;
    T[KNU_W_PB + k] = hp * B / fact;
    T[KNU_W_PC + k] = C / fact;
    T[KNU_W_QA + k] = -k * A / fact;
    T[KNU_W_QB + k] = hp * (P - k * B) / fact;
    T[KNU_W_QC + k] = -k * C / fact;
  }
  long double f0[KNU_NCHEB], f1[KNU_NCHEB];
  for (int k = 0; k < KNU_NCHEB; ++k) {
    const long double t = 0.5L * (1.0L + cosl(M_PIl * (k + 0.5L) / KNU_NCHEB));
    knu_steed_scaled(mu, 2.0L / t, &f0[k], &f1[k]);
  }
  for (int j = 0; j < KNU_NCHEB; ++j) {
    long double s0 = 0.0L, s1 = 0.0L;
    for (int k = 0; k < KNU_NCHEB; ++k) {
      const long double cs = cosl(M_PIl * j * (k + 0.5L) / KNU_NCHEB);
      s0 += f0[k] * cs, s1 += f1[k] * cs;
    }
    const long double sc = (j == 0 ? 1.0L : 2.0L) / KNU_NCHEB;
    T[KNU_W_CH0 + j] = sc * s0;
    T[KNU_W_CH1 + j] = sc * s1;
  }
  for (int i = 0; i < KNU_WORDS; ++i) words[i] = (double)T[i];
  return HFMI_OK;
}
