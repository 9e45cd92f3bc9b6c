// The Matern correlation of any smoothness 1/8 <= nu <= 8 (HFMI_KERNEL_MATERN):
//   phi_nu(a) = 2^(1-nu) / Gamma(nu) a^nu K_nu(a),  a = sqrt(2 nu) r / ell,  phi_nu(0) = 1.
// nu is constant per operator, so everything that depends on it is computed once on the host (hfmi_matern_tables.hip, long double) into
// KNU_WORDS doubles that the operator owns on the device; this function does only Horner, Clenshaw, log, exp and sqrt.  Like Matern-1 the
// family has parameter types of its own (kcov_nu_params and its cross twin, hfmi_kcov_eval.h): the instances of the other families take
// the argument blocks and compile to the code they always did.  nu = 1/2, 3/2, 5/2 and 1 run this general evaluation here and agree with
// the named families to rounding; the named families stay the fast ones.
//
//   n = floor(nu + 1/2),  mu = nu - n in [-1/2, 1/2)
//   a <= 2:  Temme's series, on the scaled S_j = (a/2)^(mu+j) K_(mu+j).  y = a^2 / 4, L = ln(a / 2), w = exp(mu L), s = -mu L:
//              w f_0 = w (cosh(s) g1 - L (sinh(s) / s) g2),  w q_0 = w^2 Gamma(1 - mu) / 2,  w p_0 = Gamma(1 + mu) / 2 (folded into PB, QB)
//              S_0 = PA(y) w f_0 + PB(y) + PC(y) w q_0,  S_1 = QA(y) w f_0 + QB(y) + QC(y) w q_0      (six 16-term polynomials, Horner)
//              S_(j+1) = y S_(j-1) + (mu + j) S_j   (no division, all terms positive from j = 1 on),  phi = (2 / Gamma(nu)) S_n
//            Only (a/2)^mu with |mu| <= 1/2 goes through exp(. ln .); a^nu never does.  sinh(s) / s is its series below |s| = 1/4.
//   a >  2:  G_0, G_1 = sqrt(a) e^a K_mu(a), K_(mu+1)(a) by degree-24 Chebyshev interpolants in t = 2 / a on [0, 1] (Clenshaw),
//              H_0 = G_0, H_1 = a G_1,  H_(j+1) = a^2 H_(j-1) + 2 (mu + j) H_j,  phi = ((cc H_n) a^(mu - 1/2)) e^(-a)
//            H_n is multiplied into the normalisation BEFORE e^(-a): the small factors first go subnormal at nu = 8, a = 700.  a is clamped
//            at 1e5, where e^(-a) has long been +0, so that a^(2 n) stays finite: a large a gives +0, never 0 * inf.
// n is uniform over the launch, so the recurrence loops do not diverge; the two sides of a = 2 do, as for Matern-1.
// tests/helpers/matern_nu_twin.py is the same arithmetic in numpy (64 eps of 40-digit values over 17 values of nu, 0 < a <= 700).
#pragma once

#define KNU_NSER 16
#define KNU_NCHEB 25
#define KNU_W_N 0
#define KNU_W_MU 1
#define KNU_W_HP 2
#define KNU_W_HQ 3
#define KNU_W_G1 4
#define KNU_W_G2 5
#define KNU_W_CS 6
#define KNU_W_CC 7
#define KNU_W_CA 8
#define KNU_W_NU 9
#define KNU_W_PA 16
#define KNU_W_PB (KNU_W_PA + KNU_NSER)
#define KNU_W_PC (KNU_W_PB + KNU_NSER)
#define KNU_W_QA (KNU_W_PC + KNU_NSER)
#define KNU_W_QB (KNU_W_QA + KNU_NSER)
#define KNU_W_QC (KNU_W_QB + KNU_NSER)
#define KNU_W_CH0 (KNU_W_QC + KNU_NSER)
#define KNU_W_CH1 (KNU_W_CH0 + KNU_NCHEB)
#define KNU_WORDS (KNU_W_CH1 + KNU_NCHEB)      // 162 = HFMI_MATERN_TABLE_WORDS
#define KNU_A_MAX 1.0e5

// The tables are read through the constant address space: the address is uniform and the memory is never written while a kernel runs, so
// every word arrives by a scalar load into a scalar register pair and costs no vector register.  knu_here passes the pointer through an
// empty statement where a group of words is used; without it the compiler hoists all 162 loads out of the slab loop of k_kcov, where
// they do not fit the scalar file (what k1_const of hfmi_kcov_k1.h records for literals).  The empty statement emits no instruction.
typedef const __attribute__((address_space(4))) double* knu_tab;
__device__ __forceinline__ knu_tab knu_here(knu_tab T) {
  asm volatile("" : "+s"(T));
  return T;
}

__device__ __forceinline__ double knu_horner(knu_tab T, double y) {
  T = knu_here(T);
  double s = T[KNU_NSER - 1];
#pragma unroll
  for (int k = KNU_NSER - 2; k >= 0; --k) s = s * y + T[k];
  return s;
}
__device__ __forceinline__ double knu_clenshaw(knu_tab T, double u2) {
  T = knu_here(T);
  double b1 = 0.0, b2 = 0.0;
#pragma unroll
  for (int j = KNU_NCHEB - 1; j >= 1; --j) {
    const double b0 = (u2 * b1 - b2) + T[j];
    b2 = b1;
    b1 = b0;
  }
  return ((0.5 * u2) * b1 - b2) + T[0];
}

// tab: the KNU_WORDS table words on the device; n: the integer part of the order (word 0), passed beside them so that it is a scalar
__device__ __forceinline__ double kcov_nu_phi(const double* tab, int n, double a) {
  const knu_tab T = (knu_tab)tab;
  if (a == 0.0) return 1.0;        // the diagonal, entry 0 of a grid's column, duplicate points
  const knu_tab Th = knu_here(T);
  const double mu = Th[KNU_W_MU];
  if (a <= 2.0) {
    const double y = 0.25 * (a * a);
    const double L = log(0.5 * a);
    const double s = -(mu * L);
    const double w = exp(mu * L), iw = exp(s);
    const double s2 = s * s;
    const double ser =
        1.0 + s2 * (1.0 / 6.0 + s2 * (1.0 / 120.0 + s2 * (1.0 / 5040.0 + s2 * (1.0 / 362880.0 + s2 * (1.0 / 39916800.0)))));
    const double shs = fabs(s) < 0.25 ? ser : (iw - w) / (2.0 * s);
    const double ch = 0.5 * (iw + w);
    const double wf0 = w * (ch * Th[KNU_W_G1] - (L * shs) * Th[KNU_W_G2]);
    const double wq0 = (w * w) * Th[KNU_W_HQ];
    double S0 = (knu_horner(T + KNU_W_PA, y) * wf0 + knu_horner(T + KNU_W_PC, y) * wq0) + knu_horner(T + KNU_W_PB, y);
    if (n > 0) {
      double S1 = (knu_horner(T + KNU_W_QA, y) * wf0 + knu_horner(T + KNU_W_QC, y) * wq0) + knu_horner(T + KNU_W_QB, y);
#pragma unroll 1
      for (int j = 1; j < n; ++j) {
        const double S2 = y * S0 + (mu + (double)j) * S1;
        S0 = S1;
        S1 = S2;
      }
      S0 = S1;
    }
    return Th[KNU_W_CS] * S0;
  }
  a = fmin(a, KNU_A_MAX);
  const double t = 2.0 / a;
  const double u2 = 4.0 * t - 2.0;      // 2 u, u = 2 t - 1
  double H0 = knu_clenshaw(T + KNU_W_CH0, u2);
  if (n > 0) {
    double H1 = a * knu_clenshaw(T + KNU_W_CH1, u2);
    const double a2 = a * a;
#pragma unroll 1
    for (int j = 1; j < n; ++j) {
      const double H2 = a2 * H0 + (2.0 * (mu + (double)j)) * H1;
      H0 = H1;
      H1 = H2;
    }
    H0 = H1;
  }
  const double pw = exp((mu - 0.5) * log(a));
  return ((Th[KNU_W_CC] * H0) * pw) * exp(-a);      // exp underflows to +0 for large a: finite and not negative
}
