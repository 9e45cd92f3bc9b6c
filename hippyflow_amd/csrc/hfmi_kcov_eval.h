// One entry of a kernel covariance, C_ij = sigma^2 phi(|x_i - x_j| / ell) + nugget delta_ij: the parameters and the evaluation shared by
// the matrix-free apply (hfmi_kcov.hip) and the pivoted Cholesky factorisation (hfmi_pchol.hip), so that both see the same matrix.  The
// rectangular apply K(T, S) reads its rows' coordinates from a second point set (kcov_cross_params) and puts the nugget on source i + diag_offset.
#pragma once
#include "hfmi_internal.h"

struct kcov_params {
  const double *x0, *x1, *x2;   // one coordinate array per dimension (x1, x2 alias x0 when d is smaller: never read)
  int64_t N;
  int d;
  double inv_ell;
  double ca;                // a = ca * |x_i - x_j| / ell
  double p1, p2;            // phi = (1 + p1 a + p2 a^2) exp(-g)
  double g1, g2;            // g = a (g1 + g2 a)
  double sigma2, nugget;
};

// what the rectangular apply K(T, S) adds: the rows' (targets') coordinates.  A type of its own, so that the square instances of k_kcov
// and the factorisation's kernels take the argument block they always took and compile to the code they always were.
struct kcov_cross_params : kcov_params {
  const double *t0, *t1, *t2;   // target coordinates, M per array (t1, t2 alias t0 when d is smaller: never read)
  int64_t M;
  int64_t diag_offset;          // target i is source i + diag_offset; -1: no target is a source (no nugget anywhere)
};

// x: d arrays of N doubles on the device; HFMI_ERR_INVALID for an unknown family (hfmi_kcov.hip)
int kcov_params_init(kcov_params* out, const double* x, int64_t N, int d, int family, double sigma, double ell, double nugget);

// the entry for a point pair at squared distance r2 = |x_i - x_j|^2 (summed by the caller as dx * dx, then one fma per further coordinate);
// same_index: i == j as point INDICES (the nugget sits on the index, not on the distance)
__device__ __forceinline__ double kcov_entry(const kcov_params& P, double r2, bool same_index) {
  const double a = P.ca * sqrt(r2) * P.inv_ell;
  const double poly = fma(a, fma(P.p2, a, P.p1), 1.0);
  const double g = a * fma(P.g2, a, P.g1);
  double v = P.sigma2 * poly * exp(-g);
  if (same_index) v += P.nugget;
  return v;
}

// HFMI_KERNEL_MATERN1, phi = a K_1(a) (hfmi_kcov_k1.h): the same blocks under types of their own, so that the evaluation is chosen by
// overload and the instances of the four polynomial-times-exponential families are the code they were.  ca = sqrt(2); p1 .. g2 are unused.
struct kcov_k1_params : kcov_params {};
struct kcov_k1_cross_params : kcov_cross_params {};

#include "hfmi_kcov_k1.h"

__device__ __forceinline__ double kcov_k1_entry(const kcov_params& P, double r2, bool same_index) {
  const double a = P.ca * sqrt(r2) * P.inv_ell;
  double v = P.sigma2 * kcov_k1_phi(a);
  if (same_index) v += P.nugget;
  return v;
}
__device__ __forceinline__ double kcov_entry(const kcov_k1_params& P, double r2, bool same_index) { return kcov_k1_entry(P, r2, same_index); }
__device__ __forceinline__ double kcov_entry(const kcov_k1_cross_params& P, double r2, bool same_index) { return kcov_k1_entry(P, r2, same_index); }

// HFMI_KERNEL_MATERN, any smoothness nu (hfmi_kcov_nu.h): again types of their own, which add the operator's table words on the device and
// the integer part n of the order.  ca = sqrt(2 nu); p1 .. g2 are unused.
struct kcov_nu_params : kcov_params {
  const double* tab;   // KNU_WORDS doubles (hfmi_kernel_matern_tables), owned by the operator
  int n;               // floor(nu + 1/2)
};
struct kcov_nu_cross_params : kcov_cross_params {
  const double* tab;
  int n;
};

#include "hfmi_kcov_nu.h"

template <class PT>
__device__ __forceinline__ double kcov_nu_entry(const PT& P, double r2, bool same_index) {
  const double a = P.ca * sqrt(r2) * P.inv_ell;
  double v = P.sigma2 * kcov_nu_phi(P.tab, P.n, a);
  if (same_index) v += P.nugget;
  return v;
}
__device__ __forceinline__ double kcov_entry(const kcov_nu_params& P, double r2, bool same_index) { return kcov_nu_entry(P, r2, same_index); }
__device__ __forceinline__ double kcov_entry(const kcov_nu_cross_params& P, double r2, bool same_index) { return kcov_nu_entry(P, r2, same_index); }

// the parameter block of a family as the type its instances take: kcov_params_init, then the same bytes
template <class PT>
inline int kcov_params_init_as(PT* out, const double* x, int64_t N, int d, int family, double sigma, double ell, double nugget) {
  kcov_params base;
  HFMI_TRY(kcov_params_init(&base, x, N, d, family, sigma, ell, nugget));
  static_cast<kcov_params&>(*out) = base;
  return HFMI_OK;
}
// the same for the general Matern family, with ca = sqrt(2 nu) as the table builder rounded it, the table and n
template <class PT>
inline int kcov_nu_params_init_as(PT* out, const double* x, int64_t N, int d, int family, double sigma, double ell, double nugget,
                                  const kcov_nu_ref& nu) {
  if (family != HFMI_KERNEL_MATERN || !nu.tab || !(nu.nu >= HFMI_MATERN_NU_MIN && nu.nu <= HFMI_MATERN_NU_MAX))
    HFMI_FAIL(HFMI_ERR_INVALID, "kernel_cov: the general Matern family needs its smoothness and tables");
  HFMI_TRY(kcov_params_init_as(out, x, N, d, family, sigma, ell, nugget));
  out->ca = nu.ca;
  out->tab = nu.tab;
  out->n = (int)floor(nu.nu + 0.5);
  return HFMI_OK;
}
