// The rules of the sparse SPD solves, host only: no HIP, no context.  cheb_solve / cheb_estimate / launch_cheb_step (hfmi_cheb.hip) and
// the smoother of the V-cycle (hfmi_amg.hip) ask them and launch what they say.  hfmi_cheb_rules_predict / hfmi_lanczos_bracket_predict
// (include/hfmi.h) evaluate them without a device; tests/test_spsolve_rules_cpu.py holds them to the expressions they replaced.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

// ------------------------------------------------------------------ A/B switches, environment read once per process
struct spsolve_knobs {
  int pcg;         // HFMI_PCG: always the block CG, never Chebyshev
  int threadmap;   // HFMI_CHEB_THREADMAP: the thread-per-entry step kernel for every k
  int unr;         // HFMI_CHEB_UNR: rows per wave of the wave-per-row step, 2 or 4; anything else 1 (measured best on config 2: 53.5 us
                   // a step; 2: 54.4, 4: 63.0, 8: 104 -- profiles/r04c_cheb_unr.txt)
};
inline spsolve_knobs spsolve_knobs_make(int pcg, int threadmap, int unr) {
  return spsolve_knobs{pcg != 0, threadmap != 0, (unr == 2 || unr == 4) ? unr : 1};
}
inline const spsolve_knobs& spsolve_knobs_ref() {
  static const spsolve_knobs kn = [] {
    auto flag = [](const char* name) {            // on when set to anything but "" or "0"
      const char* e = getenv(name);
      return e && e[0] && !(e[0] == '0' && e[1] == 0);
    };
    return spsolve_knobs_make(flag("HFMI_PCG"), flag("HFMI_CHEB_THREADMAP"), getenv("HFMI_CHEB_UNR") ? atoi(getenv("HFMI_CHEB_UNR")) : 1);
  }();
  return kn;
}

// ------------------------------------------------------------------ the three-term Chebyshev recurrence on [lmin, lmax]
//   theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma;  x_1 = x_0 + D^-1 (b - A x_0) / theta
//   rho' = 1 / (2 sigma - rho);  x_{n+1} = x_n + c1 (x_n - x_{n-1}) + c2 D^-1 (b - A x_n), c1 = rho' rho, c2 = 2 rho' / delta;  rho = rho'
struct cheb_recurrence {
  double theta, delta, rho;
  cheb_recurrence(double lmin, double lmax) : theta(0.5 * (lmax + lmin)), delta(0.5 * (lmax - lmin)), rho(delta / theta) {}
  double inv_theta() const { return 1.0 / theta; }
  bool spread() const { return delta > 1e-12 * theta; }   // else D^-1 A is a multiple of the identity: x_1 is the answer, next() is not asked
  void next(double* c1, double* c2) {
    const double rho_new = 1.0 / (2.0 * theta / delta - rho);
    *c1 = rho_new * rho;
    *c2 = 2.0 * rho_new / delta;
    rho = rho_new;
  }
};

// ------------------------------------------------------------------ the plan of one Chebyshev solve
// The error after n steps is at most 2 c^n / (1 + c^2n), c = (sqrt(kappa) - 1) / (sqrt(kappa) + 1): `planned` steps reach rel_tol.  A
// spectrum that needs more than CHEB_MAX_PLANNED (or max_iter) steps needs more than CG's superlinear convergence would: to_cg, for
// good.  Otherwise up to CHEB_ROUNDS rounds of budget[r] steps, each followed by a look at the true residual; `planned` counts x_1.
constexpr int CHEB_ROUNDS = 4, CHEB_MAX_PLANNED = 200;
struct cheb_plan {
  int planned;
  bool to_cg;
  int rounds, budget[CHEB_ROUNDS];
};
inline cheb_plan cheb_solve_plan(double lmin, double lmax, double rel_tol, int max_iter) {
  cheb_plan p = {};
  const bool spread = cheb_recurrence(lmin, lmax).spread();
  p.planned = 1;
  if (spread) {
    const double sk = sqrt(lmax / lmin), c = (sk - 1.0) / (sk + 1.0);
    p.planned = (int)ceil(log(2.0 / rel_tol) / -log(c)) + 1;
  }
  p.to_cg = p.planned > max_iter || p.planned > CHEB_MAX_PLANNED;
  if (p.to_cg) return p;
  p.budget[p.rounds++] = p.planned - 1;
  const int later = std::max(2, p.planned / 3);
  for (int steps = p.planned; spread && p.rounds < CHEB_ROUNDS && steps + later <= max_iter; steps += later) p.budget[p.rounds++] = later;
  return p;
}

// ------------------------------------------------------------------ the bracket of the spectrum of D^-1 A
// The coefficients of one scalar Jacobi-CG run are the Lanczos matrix of D^-1 A, whose extreme eigenvalues approach those of D^-1 A
// from inside; Gershgorin's circles bound them from above.
enum lanczos_refusal { LANCZOS_OK = 0, LANCZOS_NO_GERSHGORIN, LANCZOS_NOT_SPD, LANCZOS_TOO_SHORT, LANCZOS_TMIN, LANCZOS_TMAX };
inline bool gersh_usable(double gersh_lmax) { return gersh_lmax > 0.0; }    // 0 = a row without a positive diagonal entry
struct lanczos_run {
  std::vector<double> alpha, beta;
  // the inner products of one CG iteration: r.z before it, p.Ap, r.z after it; false: not SPD, the run ends without a bracket
  bool push(double rz, double pap, double rz_new) {
    if (!(pap > 0.0) || !std::isfinite(rz_new)) return false;
    alpha.push_back(rz / pap);
    beta.push_back(rz_new / rz);
    return true;
  }
};
// extreme eigenvalues of the symmetric tridiagonal matrix (a, b) by bisection on the Sturm count
inline int sturm_count(const std::vector<double>& a, const std::vector<double>& b, double x) {
  int cnt = 0;
  double q = a[0] - x;
  if (q < 0) ++cnt;
  for (size_t i = 1; i < a.size(); ++i) {
    if (q == 0.0) q = 1e-300;
    q = a[i] - x - b[i - 1] * b[i - 1] / q;
    if (q < 0) ++cnt;
  }
  return cnt;
}
inline void tridiag_extremes(const std::vector<double>& a, const std::vector<double>& b, double* smallest, double* largest) {
  double lo = a[0], hi = a[0];
  for (size_t i = 0; i < a.size(); ++i) {
    const double rad = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < a.size() ? fabs(b[i]) : 0.0);
    lo = std::min(lo, a[i] - rad);
    hi = std::max(hi, a[i] + rad);
  }
  const int m = (int)a.size();
  double l = lo, h = hi;
  for (int it = 0; it < 200 && h - l > 1e-14 * std::max(fabs(l), fabs(h)); ++it) {   // smallest: first x with count >= 1
    const double mid = 0.5 * (l + h);
    if (sturm_count(a, b, mid) >= 1) h = mid; else l = mid;
  }
  *smallest = 0.5 * (l + h);
  l = lo; h = hi;
  for (int it = 0; it < 200 && h - l > 1e-14 * std::max(fabs(l), fabs(h)); ++it) {   // largest: last x with count < m
    const double mid = 0.5 * (l + h);
    if (sturm_count(a, b, mid) >= m) h = mid; else l = mid;
  }
  *largest = 0.5 * (l + h);
}
struct cheb_bracket {
  lanczos_refusal refusal;
  double tmin, tmax, lmin, lmax;     // the Ritz values and the bracket made of them
};
inline cheb_bracket lanczos_bracket(const std::vector<double>& alpha, const std::vector<double>& beta, double gersh_lmax) {
  cheb_bracket r = {};
  const size_t m = alpha.size();
  if (!gersh_usable(gersh_lmax)) return r.refusal = LANCZOS_NO_GERSHGORIN, r;
  if (m < 3) return r.refusal = LANCZOS_TOO_SHORT, r;
  std::vector<double> a(m), b(m - 1);
  for (size_t i = 0; i < m; ++i) {
    a[i] = 1.0 / alpha[i] + (i > 0 ? beta[i - 1] / alpha[i - 1] : 0.0);
    if (i + 1 < m) b[i] = sqrt(beta[i]) / alpha[i];
  }
  tridiag_extremes(a, b, &r.tmin, &r.tmax);
  if (!(r.tmin > 0.0)) return r.refusal = LANCZOS_TMIN, r;
  if (!(r.tmax >= r.tmin)) return r.refusal = LANCZOS_TMAX, r;
  // Ritz values lie inside the spectrum: widen them; never above Gershgorin's bound
  r.lmin = 0.9 * r.tmin;
  r.lmax = std::min(gersh_lmax, 1.05 * r.tmax);
  if (r.lmax < r.tmax) r.lmax = r.tmax * (1.0 + 1e-9);
  return r;
}

// ------------------------------------------------------------------ which step kernel, on which grid
// wave: k_cheb_step_wave<resid, unr>, one wave per `unr` rows, 4 waves a workgroup (k even, <= 128); else k_cheb_step<resid>, the
// thread map of hfmi_rm_dev.h.  The grid is whole bands of workgroups for the 8 XCDs.
struct cheb_step_launch {
  bool wave;
  int unr;
  int64_t grid;
};
inline int rm_rows_per_pass(int k) { return k <= 256 ? 256 / k : 1; }
inline cheb_step_launch cheb_step_plan(int64_t nrows, int k, bool resid, const spsolve_knobs& kn) {
  cheb_step_launch L = {};
  L.wave = (k & 1) == 0 && k <= 128 && !kn.threadmap;
  L.unr = (L.wave && !resid) ? kn.unr : 1;
  const int64_t rows_per_group = L.wave ? 4 * L.unr : rm_rows_per_pass(k);
  L.grid = ((nrows + rows_per_group - 1) / rows_per_group + 7) / 8 * 8;
  return L;
}

// ------------------------------------------------------------------ hfmi_cheb_rules_predict's record
constexpr int CHEB_RULES_WORDS = 13;
inline void cheb_rules_words(const cheb_plan& p, const cheb_step_launch& L, const spsolve_knobs& kn, int64_t* w) {
  const int64_t v[CHEB_RULES_WORDS] = {p.planned, p.to_cg, p.rounds, p.budget[0], p.budget[1],  p.budget[2], p.budget[3],
                                       L.wave,    L.unr,   L.grid,   kn.pcg,      kn.threadmap, kn.unr};
  std::copy(v, v + CHEB_RULES_WORDS, w);
}
