// The Matern-1 correlation phi(a) = a K_1(a), phi(0) = 1 (HFMI_KERNEL_MATERN1): the kernel of the squared operator
// (delta - gamma div Theta grad)^2 in two dimensions.  K_1 is a modified Bessel function, which the branch-free
// (1 + p1 a + p2 a^2) exp(-g) of the other families cannot produce, so the family has parameter types of its own (kcov_k1_params and its
// cross twin, hfmi_kcov_eval.h): the instances of the other families take the argument blocks and compile to the code they always did.
//
//   a <= 2:  phi = 1 + y (2 ln(a / 2) S1(y) - S2(y)),  y = a^2 / 4,  S1 = sum y^k / (k! (k+1)!),  S2 = sum (psi(k+1) + psi(k+2)) y^k / (k! (k+1)!)
//            (the exact power series of K_1, 14 terms by Horner; at a = 2 the result is 0.28 of its leading term)
//   a >  2:  phi = sqrt(a) exp(-a) g(2 / a),  g the degree-24 Chebyshev interpolant of sqrt(a) e^a K_1(a) in t = 2 / a on [0, 1], by Clenshaw
//
// The two sides diverge within a wave, so a wave that holds both pays for both: about 100 fp64 VALU instructions and log, exp, sqrt and one
// division per entry.  The tables come from scripts/make_matern1_coeffs.py (mpmath, 50 digits); tests/helpers/matern1_twin.py is the same
// arithmetic in numpy and is held to 40-digit values (tests/golden/matern1_phi.npz).
#pragma once

#define K1_NSER 14
#define K1_NCHEB 25

// A table entry as a scalar register pair, materialised where it is used.  Left to itself the compiler hoists all 53 constants out of the
// slab loop of k_kcov; they do not fit the scalar file beside the kernel's own, and the overflow costs ~45 VGPRs (spills from 6 column
// tiles on).  The empty statement emits no instruction.
__device__ __forceinline__ double k1_const(double c) {
  asm volatile("" : "+s"(c));
  return c;
}

__device__ __forceinline__ double kcov_k1_phi(double a) {
  constexpr double S1[K1_NSER] = {
      1.0000000000000000000,     5.0000000000000000000e-1,  8.3333333333333333333e-2,  6.9444444444444444444e-3,  3.4722222222222222222e-4,
      1.1574074074074074074e-5,  2.7557319223985890653e-7,  4.9209498614260519022e-9,  6.8346525853139609753e-11, 7.5940584281266233059e-13,
      6.9036894801151120963e-15, 5.2300677879659940123e-17, 3.3526075563884577002e-19, 1.8420920639497020331e-21};
  constexpr double S2[K1_NSER] = {
      -1.5443132980306572121e-1, 6.7278433509846713939e-1,  1.8157516696085563434e-1,  1.9182189839330562121e-2,  1.1153594919665281061e-3,
      4.1422476892711430696e-5,  1.0715459140911808686e-6,  2.0452860035938779413e-8,  3.0020487465891878859e-10, 3.4959287296928819208e-12,
      3.3099147352502720680e-14, 2.5986411321011287351e-16, 1.7195232826992565241e-18, 9.7212075188236180165e-21};
  constexpr double CH[K1_NCHEB] = {
      1.3603130952422213347,      1.0392373657681723844e-1,   -2.8578168596227793868e-3,  1.9521551847135163111e-4,  -1.9361979741660829600e-5,
      2.4064849478372171171e-6,   -3.5019606030878125421e-7,  5.7410841254500492923e-8,   -1.0345762465678097027e-8, 2.0150497551970346161e-9,
      -4.1903547593419255842e-10, 9.2183151876053141258e-11,  -2.1299678384277910216e-11, 5.1396396734823435404e-12, -1.2891739609498229352e-12,
      3.3484196660522431201e-13,  -8.9767051820101460692e-14, 2.4771544242195986813e-14,  -7.0198370892147688513e-15, 2.0387031662398608799e-15,
      -6.0570472706430178228e-16, 1.8380935752430454256e-16,  -5.6894628491936483743e-17, 1.7940510478863572914e-17, -5.7567444820733024503e-18};
  if (a == 0.0) return 1.0;        // the diagonal, entry 0 of a grid's column, duplicate points: not 0 * ln 0
  if (a <= 2.0) {
    const double y = 0.25 * (a * a);
    double s1 = S1[K1_NSER - 1], s2 = S2[K1_NSER - 1];
#pragma unroll
    for (int k = K1_NSER - 2; k >= 0; --k) {
      s1 = s1 * y + k1_const(S1[k]);
      s2 = s2 * y + k1_const(S2[k]);
    }
    const double lg = log(0.5 * a);
    return y * ((2.0 * lg) * s1 - s2) + 1.0;
  }
  const double t = 2.0 / a;
  const double u2 = 4.0 * t - 2.0;      // 2 u, u = 2 t - 1
  double b1 = 0.0, b2 = 0.0;
#pragma unroll
  for (int j = K1_NCHEB - 1; j >= 1; --j) {
    const double b0 = (u2 * b1 - b2) + k1_const(CH[j]);
    b2 = b1;
    b1 = b0;
  }
  const double g = ((0.5 * u2) * b1 - b2) + CH[0];
  return (sqrt(a) * exp(-a)) * g;       // exp underflows to +0 for large a: finite and not negative
}
