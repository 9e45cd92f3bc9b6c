// Launch plan of the box Whittle-Matern operators W^a T_s W^b (hfmi_op_box, hfmi_boxcov.hip).  Host only, plain C++17, nothing from HIP.
// hfmi_boxcov_plan_predict (include/hfmi.h) writes the same struct out without a device and tests/test_box_prior_cpu.py holds it to a
// Python statement of the rules (tests/helpers/boxcov_plan_twin.py).
//
// The grid: axis c has n_c nodes and a side, Neumann or periodic.  A Neumann axis is transformed as the mirrored line of
// P_c = 2 (n_c - 1) entries (1 when n_c = 1; n_c - 1 a power of two), which makes the complex FFT a DCT-I of each part; a periodic axis
// is its own line, P_c = n_c (a power of two).  The work buffer of one pair of columns is a complex array of EXTENTS E_c = n_c on both
// kinds of axis, axis 0 fastest: N = prod n_c entries, never prod P_c.  On the time side of an axis its entries are the n_c nodes.  On
// the frequency side a Neumann axis holds the modes 0 .. n_c - 1 in natural order (the transform of a mirrored line is even, so these
// are all of it) and a periodic axis the P_c positions in the digit-reversed order the forward stages leave, as hfmi_fftcov_plan.h.
//
// Passes of an apply in d dimensions (2 d - 1, as hfmi_fftcov_plan.h): forward along 0 .. d - 2, ONE pass along d - 1 that transforms
// forward, multiplies by the operator's table and transforms back while the line sits in LDS, inverse along d - 2 .. 0.  The pass
// along axis 0 that comes first scatters from the input block (times W^b), the one that comes last gathers into the output block
// (times W^a); d = 1 is one pass that does both.  Every line of every pass exists (nothing is padded): a pass along axis a has
// N / n_a lines, line l starts at entry (l mod stride) + (l div stride) stride n_a with stride = prod_{b < a} n_b.  Strides are not
// powers of two, so the line map divides.
//
// What a pass does at the ends of a line (n = n_a, P = P_a, brev = bit reversal of log2 P bits):
//   time-side load (a pass with the forward stages)       Neumann: n entries, entry j to LDS j and, for 1 <= j <= n - 2, to LDS P - j;
//                                                         periodic: P entries
//   frequency-side store (forward stages, no inverse)     Neumann: buffer[k] = LDS[brev(k)], k < n; periodic: buffer[p] = LDS[p]
//   frequency-side load (inverse stages, no forward)      Neumann: buffer[k] to LDS[brev(k)] and, for 0 < k < n - 1, to LDS[brev(P - k)];
//                                                         periodic: LDS[p] = buffer[p]
//   time-side store (a pass with the inverse stages)      the first n positions
//   fused multiply                                        LDS position p times the table at the mode of p: min(brev(p), P - brev(p)) on
//                                                         a Neumann axis, p itself (storage order) on a periodic one
// Workgroup shape (lines per workgroup, LDS line stride and padding, threads, dynamic LDS, grid): fftcov_pass_shape of
// hfmi_fftcov_plan.h from (P_a, stride, lines).  Pairs per chunk: fftcov_plan_chunks with 16 N bytes per pair and the tuning key
// "fftcov_pairs".
#pragma once
#include <stdint.h>
#include <string.h>

#include "hfmi_fftcov_plan.h"

constexpr int BOXCOV_NEUMANN = 0, BOXCOV_PERIODIC = 1;      // HFMI_BOX_NEUMANN / HFMI_BOX_PERIODIC of include/hfmi.h
constexpr int BOXCOV_MAX_NEUMANN = 2049;                    // nodes of a Neumann axis: P = 4096
constexpr int BOXCOV_MAX_PERIODIC = 4096;
constexpr int BOXCOV_MAX_PASSES = 5;
constexpr int BOXCOV_STATIC_LDS = (8 + 4) * FFTCOV_MAX_LINES;   // k_boxcov_pass: line bases (8 bytes) and end counts (4 bytes)

struct boxcov_pass {
  int axis, flags;        // FFTCOV_FWD | FFTCOV_MUL | FFTCOV_INV | FFTCOV_SCATTER | FFTCOV_GATHER
  int L, logL;            // line length in LDS, P_axis
  int mirror;             // 1: a Neumann axis of more than one node
  int n;                  // extent of the axis in the work buffer, n_axis
  int64_t stride;         // entries between consecutive positions of a line: prod n_b, b < axis
  int64_t span;           // entries between the lines l and l + stride: stride n_axis
  int64_t nlines;         // N / n_axis
  int lpw, loglpw, ls, threads, lds;
  int64_t grid_x;
};
struct boxcov_plan {
  int d;
  int64_t n[3];
  int boundary[3];
  int P[3];
  int64_t N;
  int npasses;
  boxcov_pass pass[BOXCOV_MAX_PASSES];
  int twiddles, Pmax;     // the table exp(-2 pi i k / Pmax), k < max(Pmax / 4, 1)
  fftcov_plan chunks;     // pair_bytes, pairs, chunk_pairs, nchunks (fftcov_plan_chunks)
};

inline bool boxcov_pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }
// the rule of an axis: Neumann n = 1 or n - 1 a power of two, n <= 2049; periodic n a power of two, n <= 4096
inline bool boxcov_axis_ok(int64_t n, int boundary) {
  if (boundary == BOXCOV_NEUMANN) return n == 1 || (n >= 2 && n <= BOXCOV_MAX_NEUMANN && boxcov_pow2(n - 1));
  if (boundary == BOXCOV_PERIODIC) return n >= 1 && n <= BOXCOV_MAX_PERIODIC && boxcov_pow2(n);
  return false;
}
inline int boxcov_line_len(int64_t n, int boundary) { return boundary == BOXCOV_NEUMANN ? (n > 1 ? (int)(2 * (n - 1)) : 1) : (int)n; }

inline boxcov_pass boxcov_make_pass(const boxcov_plan& p, int axis, int flags) {
  boxcov_pass q;
  memset(&q, 0, sizeof(q));
  q.axis = axis;
  q.flags = flags;
  q.L = p.P[axis];
  q.logL = fftcov_log2(q.L);
  q.n = (int)p.n[axis];
  q.mirror = p.boundary[axis] == BOXCOV_NEUMANN && q.n > 1;
  q.stride = 1;
  for (int b = 0; b < axis; ++b) q.stride *= p.n[b];
  q.span = q.stride * q.n;
  q.nlines = p.N / q.n;
  fftcov_pass s;          // the workgroup shape is the FFT route's rule
  memset(&s, 0, sizeof(s));
  s.L = q.L, s.stride = q.stride, s.nlines = q.nlines;
  fftcov_pass_shape(s);
  q.lpw = s.lpw, q.loglpw = s.loglpw, q.ls = s.ls, q.threads = s.threads, q.lds = s.lds, q.grid_x = s.grid_x;
  return q;
}

// the caller has checked d and every axis (boxcov_axis_ok)
inline boxcov_plan boxcov_plan_passes(int d, const int64_t* n, const int* boundary) {
  boxcov_plan p;
  memset(&p, 0, sizeof(p));
  p.d = d;
  p.N = 1;
  p.Pmax = 1;
  for (int c = 0; c < 3; ++c) {
    p.n[c] = c < d ? n[c] : 1;
    p.boundary[c] = c < d ? boundary[c] : BOXCOV_NEUMANN;
    p.P[c] = boxcov_line_len(p.n[c], p.boundary[c]);
    p.N *= p.n[c];
    if (p.P[c] > p.Pmax) p.Pmax = p.P[c];
  }
  p.twiddles = p.Pmax / 4 > 1 ? p.Pmax / 4 : 1;
  p.chunks.pair_bytes = 16 * p.N;
  int np = 0;
  for (int a = 0; a < d - 1; ++a) p.pass[np++] = boxcov_make_pass(p, a, FFTCOV_FWD | (a == 0 ? FFTCOV_SCATTER : 0));
  p.pass[np++] = boxcov_make_pass(p, d - 1, FFTCOV_FWD | FFTCOV_MUL | FFTCOV_INV | (d == 1 ? FFTCOV_SCATTER | FFTCOV_GATHER : 0));
  for (int a = d - 2; a >= 0; --a) p.pass[np++] = boxcov_make_pass(p, a, FFTCOV_INV | (a == 0 ? FFTCOV_GATHER : 0));
  p.npasses = np;
  return p;
}

// what k_boxcov_pass can be launched with (hfmi_box_create refuses a grid with a pass that fails this)
inline bool boxcov_pass_launchable(const boxcov_pass& q) {
  return q.lds + BOXCOV_STATIC_LDS <= FFTCOV_LDS_BYTES && q.lpw <= FFTCOV_MAX_LINES && q.threads <= FFTCOV_MAX_THREADS && q.grid_x >= 1 &&
         q.grid_x <= 0x7fffffff;
}

// ------------------------------------------------------------------ hfmi_boxcov_plan_predict's record
// words[BOXCOV_PLAN_WORDS]: a head of 16 words, then 16 per pass.
//   head   0 d  1-3 n_c  4 N  5 pairs  6 pairs per chunk  7 chunks  8 passes  9 bytes per pair  10 twiddles  11 max P_c
//          12 static LDS of k_boxcov_pass  13-15 P_c
//   pass   0 axis  1 flags  2 line length  3 mirror  4 extent  5 stride  6 span  7 lines  8 lines per workgroup  9 LDS line stride
//          10 threads  11 dynamic LDS  12 static + dynamic LDS  13 grid x  14-15 zero
constexpr int BOXCOV_HEAD_WORDS = 16;
constexpr int BOXCOV_PASS_WORDS = 16;
constexpr int BOXCOV_PLAN_WORDS = BOXCOV_HEAD_WORDS + BOXCOV_MAX_PASSES * BOXCOV_PASS_WORDS;
inline void boxcov_plan_words(const boxcov_plan& p, int64_t* w) {
  memset(w, 0, sizeof(int64_t) * BOXCOV_PLAN_WORDS);
  const int64_t head[BOXCOV_HEAD_WORDS] = {p.d, p.n[0], p.n[1], p.n[2], p.N, p.chunks.pairs, p.chunks.chunk_pairs, p.chunks.nchunks,
                                           p.npasses, p.chunks.pair_bytes, p.twiddles, p.Pmax, BOXCOV_STATIC_LDS, p.P[0], p.P[1], p.P[2]};
  memcpy(w, head, sizeof(head));
  for (int i = 0; i < p.npasses; ++i) {
    const boxcov_pass& q = p.pass[i];
    const int64_t v[BOXCOV_PASS_WORDS] = {q.axis, q.flags, q.L, q.mirror, q.n, q.stride, q.span, q.nlines,
                                          q.lpw, q.ls, q.threads, q.lds, q.lds + BOXCOV_STATIC_LDS, q.grid_x, 0, 0};
    memcpy(w + BOXCOV_HEAD_WORDS + i * BOXCOV_PASS_WORDS, v, sizeof(v));
  }
}
