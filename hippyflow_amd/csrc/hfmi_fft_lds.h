// The in-LDS complex fp64 line transform of the grid kernel covariances (hfmi_fftcov.hip) and the box Whittle-Matern priors
// (hfmi_boxcov.hip): the one home of the double2 arithmetic, the quarter twiddle table and its lookups, the radix-4 / radix-2 stages and
// the radix-3 / radix-5 stage.  The pass bodies of both units keep their own ends (line map, load, multiply, store) and call these.
//
// A workgroup holds `lpw` lines of L entries at x + j ls, and the twiddles exp(-2 pi i k / L), k < max(L / 4, 1), at ltw.  The forward
// transform is decimation in frequency, in place: natural order in, digit-reversed order out; the inverse is decimation in time, takes
// that order and is unnormalised.  Every stage ends in a barrier.  The power-of-two stages come in two kinds, chosen at compile time:
//   plain    the whole line, L = 2^logQ: the line of an item is found by shifts, the twiddle step is 1, lookups are below L / 2;
//   BLOCKED  the L / Q blocks of Q = 2^logQ entries of a mixed-radix line L = 3^a 5^b Q (hfmi_boxcov_plan.h): the line of an item is found
//            by dividing, w_Q^k = w_L^(k odd) with odd = L / Q, and the lookups range over the whole circle.
// With Q = L the blocked index arithmetic is the plain one; what differs is under `if constexpr`, so a plain instance has no division.
// The bank layout of these stages (the pad of fftcov_pass_shape, the strides B / r of the odd stages) has NOT been measured.
#pragma once
#include <math.h>

#include <vector>

#include "hfmi_internal.h"

__device__ __forceinline__ double2 fft_add(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double2 fft_sub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ double2 fft_mul(double2 a, double2 b) { return double2{fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)}; }
// a * conj(b)
__device__ __forceinline__ double2 fft_mulc(double2 a, double2 b) { return double2{fma(a.x, b.x, a.y * b.y), fma(a.y, b.x, -a.x * b.y)}; }

// exp(-2 pi i k / L) for k < L / 2 from the quarter table (qm = max(L / 4, 1) entries, a power of two): the second quarter is -i times the first
__device__ __forceinline__ double2 fft_twiddle(const double2* ltw, int k, int qm) {
  const double2 t = ltw[k & (qm - 1)];
  return k >= qm ? double2{t.y, -t.x} : t;
}
// exp(-2 pi i k / L) for k < L from the quarter table (qm = L / 4 entries, any L that is a multiple of 4): the other quarters are the
// first times -i, -1, i
__device__ __forceinline__ double2 fft_twiddle_full(const double2* ltw, int k, int qm) {
  const bool half = k >= 2 * qm;
  if (half) k -= 2 * qm;
  const bool quarter = k >= qm;
  if (quarter) k -= qm;
  double2 t = ltw[k];
  if (quarter) t = double2{t.y, -t.x};
  if (half) t = double2{-t.x, -t.y};
  return t;
}

// item idx of a loop over `lpw` lines with `per` items each -> line j and item u of that line; plain: per = 2^logper
template <bool BLOCKED>
__device__ __forceinline__ void fft_split(int idx, int per, int logper, int& j, int& u) {
  if constexpr (BLOCKED) {
    j = idx / per;
    u = idx - j * per;
  } else {
    j = idx >> logper;
    u = idx & (per - 1);
  }
}
// the twiddle of a power-of-two stage at table index k (already times odd on a blocked line)
template <bool BLOCKED>
__device__ __forceinline__ double2 fft_stage_twiddle(const double2* ltw, int k, int qm) {
  if constexpr (BLOCKED) return fft_twiddle_full(ltw, k, qm);
  else return fft_twiddle(ltw, k, qm);
}

// Forward power-of-two stages on every block of Q = 2^logQ entries.  Two radix-2 stages are done per trip through LDS (four entries per
// thread, a radix-4 step written as its two radix-2 stages); an odd logQ starts with one radix-2 stage.  qm: entries of the quarter table.
template <bool BLOCKED>
__device__ __forceinline__ void fft_pow2_forward(double2* x, const double2* ltw, int qm, int L, int logQ, int lpw, int ls, int tid, int nt) {
  const int total = BLOCKED ? lpw * L : lpw << logQ;
  const int odd = BLOCKED ? L >> logQ : 1;     // the step of the block's twiddles in the line's table
  int lh = logQ - 1;
  if (logQ & 1) {          // one radix-2 stage, h = Q / 2
    const int h = 1 << lh, items = total >> 1;
    for (int idx = tid; idx < items; idx += nt) {
      int j, u;
      fft_split<BLOCKED>(idx, BLOCKED ? L >> 1 : h, lh, j, u);
      const int off = u & (h - 1);
      double2* xi = x + j * ls + (BLOCKED ? (u >> lh) << logQ : 0) + off;
      const double2 a = xi[0], b = xi[h];
      xi[0] = fft_add(a, b);
      xi[h] = fft_mul(fft_sub(a, b), fft_stage_twiddle<BLOCKED>(ltw, off * odd, qm));
    }
    --lh;
    __syncthreads();
  }
  for (; lh >= 1; lh -= 2) {   // stages h = 2^lh and q = h / 2
    const int lq = lh - 1, q = 1 << lq, items = total >> 2;
    for (int idx = tid; idx < items; idx += nt) {
      int j, r;
      fft_split<BLOCKED>(idx, L >> 2, logQ - 2, j, r);
      const int off = r & (q - 1);
      double2* xi = x + j * ls + ((r >> lq) << (lq + 2)) + off;
      const int k1 = (off << (logQ - 2 - lq)) * odd;
      const double2 w1 = ltw[k1], w1q = double2{w1.y, -w1.x}, w2 = fft_stage_twiddle<BLOCKED>(ltw, 2 * k1, qm);
      const double2 x0 = xi[0], x1 = xi[q], x2 = xi[2 * q], x3 = xi[3 * q];
      const double2 a = fft_add(x0, x2), b = fft_mul(fft_sub(x0, x2), w1);
      const double2 c = fft_add(x1, x3), d = fft_mul(fft_sub(x1, x3), w1q);
      xi[0] = fft_add(a, c);
      xi[q] = fft_mul(fft_sub(a, c), w2);
      xi[2 * q] = fft_add(b, d);
      xi[3 * q] = fft_mul(fft_sub(b, d), w2);
    }
    __syncthreads();
  }
}

// Inverse power-of-two stages on every block of Q = 2^logQ entries: the transposed stages of fft_pow2_forward in reverse order with
// conjugate twiddles, the twiddle first, unnormalised.
template <bool BLOCKED>
__device__ __forceinline__ void fft_pow2_inverse(double2* x, const double2* ltw, int qm, int L, int logQ, int lpw, int ls, int tid, int nt) {
  const int total = BLOCKED ? lpw * L : lpw << logQ;
  const int odd = BLOCKED ? L >> logQ : 1;
  for (int lq = 0; lq + 1 < logQ; lq += 2) {   // stages q = 2^lq and 2 q
    const int q = 1 << lq, items = total >> 2;
    for (int idx = tid; idx < items; idx += nt) {
      int j, r;
      fft_split<BLOCKED>(idx, L >> 2, logQ - 2, j, r);
      const int off = r & (q - 1);
      double2* xi = x + j * ls + ((r >> lq) << (lq + 2)) + off;
      const int k1 = (off << (logQ - 2 - lq)) * odd;
      const double2 w1 = ltw[k1], w1q = double2{w1.y, -w1.x}, w2 = fft_stage_twiddle<BLOCKED>(ltw, 2 * k1, qm);
      const double2 y0 = xi[0], y1 = xi[q], y2 = xi[2 * q], y3 = xi[3 * q];
      double2 t = fft_mulc(y1, w2);
      const double2 a = fft_add(y0, t), c = fft_sub(y0, t);
      t = fft_mulc(y3, w2);
      const double2 b = fft_add(y2, t), d = fft_sub(y2, t);
      t = fft_mulc(b, w1);
      xi[0] = fft_add(a, t);
      xi[2 * q] = fft_sub(a, t);
      t = fft_mulc(d, w1q);
      xi[q] = fft_add(c, t);
      xi[3 * q] = fft_sub(c, t);
    }
    __syncthreads();
  }
  if (logQ & 1) {          // the radix-2 stage h = Q / 2
    const int lh = logQ - 1, h = 1 << lh, items = total >> 1;
    for (int idx = tid; idx < items; idx += nt) {
      int j, u;
      fft_split<BLOCKED>(idx, BLOCKED ? L >> 1 : h, lh, j, u);
      const int off = u & (h - 1);
      double2* xi = x + j * ls + (BLOCKED ? (u >> lh) << logQ : 0) + off;
      const double2 a = xi[0], t = fft_mulc(xi[h], fft_stage_twiddle<BLOCKED>(ltw, off * odd, qm));
      xi[0] = fft_add(a, t);
      xi[h] = fft_sub(a, t);
    }
    __syncthreads();
  }
}

// -i a (the forward transform's rotation); INV: i a
template <bool INV>
__device__ __forceinline__ double2 fft_rot(double2 a) {
  return INV ? double2{-a.y, a.x} : double2{a.y, -a.x};
}
// v[t] = sum_s v[s] w_R^(s t), w_R = exp(-2 pi i / R); INV: the conjugate
template <int R, bool INV>
__device__ __forceinline__ void fft_dft(double2* v) {
  if (R == 3) {
    const double s3 = 0.86602540378443864676;     // sin(2 pi / 3)
    const double2 t1 = fft_add(v[1], v[2]), d = fft_sub(v[1], v[2]);
    const double2 t2 = double2{fma(-0.5, t1.x, v[0].x), fma(-0.5, t1.y, v[0].y)};
    const double2 e = fft_rot<INV>(double2{s3 * d.x, s3 * d.y});
    v[0] = fft_add(v[0], t1);
    v[1] = fft_add(t2, e);
    v[2] = fft_sub(t2, e);
  } else {
    const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;     // cos(2 pi / 5), cos(4 pi / 5)
    const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;      // sin(2 pi / 5), sin(4 pi / 5)
    const double2 a1 = fft_add(v[1], v[4]), a2 = fft_add(v[2], v[3]), b1 = fft_sub(v[1], v[4]), b2 = fft_sub(v[2], v[3]);
    const double2 r1 = double2{fma(c2, a2.x, fma(c1, a1.x, v[0].x)), fma(c2, a2.y, fma(c1, a1.y, v[0].y))};
    const double2 r2 = double2{fma(c1, a2.x, fma(c2, a1.x, v[0].x)), fma(c1, a2.y, fma(c2, a1.y, v[0].y))};
    const double2 e1 = fft_rot<INV>(double2{fma(s2, b2.x, s1 * b1.x), fma(s2, b2.y, s1 * b1.y)});
    const double2 e2 = fft_rot<INV>(double2{fma(-s1, b2.x, s2 * b1.x), fma(-s1, b2.y, s2 * b1.y)});
    v[0] = fft_add(v[0], fft_add(a1, a2));
    v[1] = fft_add(r1, e1);
    v[4] = fft_sub(r1, e1);
    v[2] = fft_add(r2, e2);
    v[3] = fft_sub(r2, e2);
  }
}
// One radix-R stage on the blocks of B entries of every line, in place: thread item (line j, block, q < sub = B / R) holds the R entries
// block + q + s sub.  Forward: the R-point sums, then times w_B^(q t); INV: times the conjugate twiddle, then the conjugate sums.
template <int R, bool INV>
__device__ __forceinline__ void fft_odd_stage(double2* x, const double2* ltw, int L, int B, int lpw, int ls, int tid, int nt) {
  const int sub = B / R, per = L / R, items = lpw * per, step = L / B, qm = L >> 2;
  for (int idx = tid; idx < items; idx += nt) {
    const int j = idx / per, u = idx - j * per;
    const int blk = u / sub, q = u - blk * sub;
    double2* xi = x + j * ls + blk * B + q;
    double2 v[R];
#pragma unroll
    for (int s = 0; s < R; ++s) v[s] = xi[s * sub];
    if (INV) {
#pragma unroll
      for (int t = 1; t < R; ++t) v[t] = fft_mulc(v[t], fft_twiddle_full(ltw, q * t * step, qm));
    }
    fft_dft<R, INV>(v);
    if (!INV) {
#pragma unroll
      for (int t = 1; t < R; ++t) v[t] = fft_mul(v[t], fft_twiddle_full(ltw, q * t * step, qm));
    }
#pragma unroll
    for (int s = 0; s < R; ++s) xi[s * sub] = v[s];
  }
  __syncthreads();
}

// ------------------------------------------------------------------ host
// the twiddle table exp(-2 pi i k / P), k < count, on the device: long double on the host, rounded once
static inline int fft_twiddles_upload(dev_buf<double2>& tw, int P, int count) {
  std::vector<double2> t((size_t)count);
  const long double two_pi = 2.0L * acosl(-1.0L);
  for (int k = 0; k < count; ++k) {
    const long double a = -two_pi * (long double)k / (long double)P;
    t[k] = double2{(double)cosl(a), (double)sinl(a)};
  }
  OWN_TRY(tw.alloc(t.size()));
  HIP_TRY(hipMemcpy(tw, t.data(), t.size() * sizeof(double2), hipMemcpyHostToDevice));
  return HFMI_OK;
}

// Chunks of `nvec` columns (fftcov_plan_chunks, the tuning key "fftcov_pairs") and a work buffer that holds one.  The buffer grows to
// the chunk, the larger one first, so that when the device has no room for it the call runs in the chunks the buffer at hand holds
// (same results).  `entries`: complex entries of one pair's array, chunks.pair_bytes / 16.
static inline int fft_fit_work(hfmi_ctx* ctx, dev_buf<double2>& work, fftcov_plan& chunks, int64_t entries, int nvec) {
  fftcov_plan_chunks(chunks, nvec, 0, fftcov_pairs_knob());
  const int held = (int)(work.bytes() / (sizeof(double2) * (size_t)entries));
  if (chunks.chunk_pairs > held) {
    dev_buf<double2> bigger;
    if (bigger.alloc((size_t)chunks.chunk_pairs * (size_t)entries) == 0) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      work = std::move(bigger);
    } else {
      fftcov_plan_chunks(chunks, nvec, 0, held);
    }
  }
  return HFMI_OK;
}
