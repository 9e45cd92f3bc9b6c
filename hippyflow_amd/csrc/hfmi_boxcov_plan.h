// Launch plan of the box Whittle-Matern operators W^a T_s W^b (hfmi_op_box, hfmi_boxcov.hip).  Host only, plain C++17, nothing from HIP.
// hfmi_boxcov_plan_predict (include/hfmi.h) writes the same struct out without a device and tests/test_box_prior_cpu.py holds it to a
// Python statement of the rules (tests/helpers/boxcov_plan_twin.py; tests/helpers/boxcov_mr_twin.py for the mixed-radix lines).
//
// The grid: axis c has n_c nodes and a side, Neumann or periodic.  A Neumann axis is transformed as the mirrored line of
// P_c = 2 (n_c - 1) entries (1 when n_c = 1), which makes the complex FFT a DCT-I of each part; a periodic axis is its own line,
// P_c = n_c.  THE RULE OF AN AXIS (boxcov_axis_ok): P_c is a power of two (Neumann n_c = 1 or 2^m + 1, periodic 2^m), or P_c is a
// multiple of 4 with no prime factor but 2, 3 and 5; and P_c <= 4096, i.e. n_c <= 2049 Neumann and <= 4096 periodic.  A line with an odd
// factor is a MIXED-RADIX line, P = 3^a 5^b Q with the power-of-two tail Q >= 4.  Out of the rule: any other prime factor, P_c not a
// multiple of 4 (Neumann 4, 6, 8 nodes; periodic 6, 18), longer lines.
// The work buffer of one pair of columns is a complex array of EXTENTS E_c = n_c on both
// kinds of axis, axis 0 fastest: N = prod n_c entries, never prod P_c.  On the time side of an axis its entries are the n_c nodes.  On
// the frequency side a Neumann axis holds the modes 0 .. n_c - 1 in natural order (the transform of a mirrored line is even, so these
// are all of it) and a periodic axis the P_c positions in the STORAGE order the forward stages leave: position p holds mode(p), the
// digit reversal of hfmi_fftcov_plan.h on a power-of-two line and the position map below on a mixed-radix one (k_boxcov_table follows it).
//
// Passes of an apply in d dimensions (2 d - 1, as hfmi_fftcov_plan.h): forward along 0 .. d - 2, ONE pass along d - 1 that transforms
// forward, multiplies by the operator's table and transforms back while the line sits in LDS, inverse along d - 2 .. 0.  The pass
// along axis 0 that comes first scatters from the input block (times W^b), the one that comes last gathers into the output block
// (times W^a); d = 1 is one pass that does both.  Every line of every pass exists (nothing is padded): a pass along axis a has
// N / n_a lines, line l starts at entry (l mod stride) + (l div stride) stride n_a with stride = prod_{b < a} n_b.  Strides are not
// powers of two, so the line map divides.
//
// The stages of a mixed-radix line (k_boxcov_pass_mr; a power-of-two line runs k_boxcov_pass; the stages of both, and of k_fftcov_pass,
// are written once, in hfmi_fft_lds.h: a power-of-two line is the case of one block, Q = P, with no odd stage).  Forward,
// decimation in frequency: one radix-r stage per odd factor, all 3s and then all 5s, on blocks of B = P, P / r, ... entries, then the
// radix-4 / radix-2 stages on the 3^a 5^b blocks of Q entries that remain.  The radix-r stage on the block at b0, sub = B / r, q < sub, t < r:
//     y[b0 + t sub + q] = (sum_s x[b0 + q + s sub] w_r^(s t)) w_B^(q t),     w_M = exp(-2 pi i / M).
// The inverse runs the transposed stages in reverse order with conjugate twiddles (twiddle first, then the r-point sums), unnormalised.
// THE POSITION MAP: after the forward stages position p holds mode(p); over a block with leading odd factor r,
// mode(p) = p div sub + r mode_sub(p mod sub), and on the tail mode_sub is the reversal of log2 Q bits.  boxcov_mr_modes builds
// mode(p) and its inverse pos(m) on the host; hfmi_box_create uploads both per distinct mixed-radix length, so no kernel loops over digits.
//
// What a pass does at the ends of a line (n = n_a, P = P_a; pos = the inverse of the position map, bit reversal of log2 P bits on a
// power-of-two line):
//   time-side load (a pass with the forward stages)       Neumann: n entries, entry j to LDS j and, for 1 <= j <= n - 2, to LDS P - j;
//                                                         periodic: P entries
//   frequency-side store (forward stages, no inverse)     Neumann: buffer[k] = LDS[pos(k)], k < n; periodic: buffer[p] = LDS[p]
//   frequency-side load (inverse stages, no forward)      Neumann: buffer[k] to LDS[pos(k)] and, for 0 < k < n - 1, to LDS[pos(P - k)];
//                                                         periodic: LDS[p] = buffer[p]
//   time-side store (a pass with the inverse stages)      the first n positions
//   fused multiply                                        LDS position p times the table at the mode of p: min(mode(p), P - mode(p)) on
//                                                         a Neumann axis, p itself (storage order) on a periodic one
// Twiddles: the power-of-two lines share ONE quarter table exp(-2 pi i k / Pmax2), k < max(Pmax2 / 4, 1), over the largest power-of-two
// P_c (Pmax2 = 1 when there is none), read with the step Pmax2 / P.  Every distinct mixed-radix length P has a quarter table of its own,
// exp(-2 pi i k / P), k < P / 4 (P is a multiple of 4, so the other three quarters are this one times -i, -1, i, exactly); every twiddle
// of its stages is an entry of it: w_B^(q t) = w_P^(q t P / B) and the tail's w_Q^k = w_P^(k P / Q).
// Workgroup shape (lines per workgroup, LDS line stride and padding, threads, dynamic LDS, grid) of a power-of-two line: fftcov_pass_shape
// of hfmi_fftcov_plan.h from (P_a, stride, lines).  Of a mixed-radix line (boxcov_mr_shape), the same rule with every quotient rounded
// down to a power of two: lines per workgroup = pow2floor(2048 / P), at least 1; on a strided axis at least min(4, pow2floor(8192 / P));
// at most 256; halved while half of them still cover all lines.  Padding between lines, threads (64 per 64 radix-4 butterflies of the
// tail, 64 .. 512) and the dynamic LDS 16 (lpw (P + pad) + P / 4) as there.  The quarter table is what lets the longest mixed-radix
// line ride two abreast on a strided axis: 2 x (4000 + 8) + 1000 entries are 144256 bytes, 147328 with the static tables, within the
// 160 KiB; a full table (4000 more entries) would not fit.  Pairs per chunk: fftcov_plan_chunks with 16 N bytes per pair and the tuning
// key "fftcov_pairs".
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
  int L, logL;            // line length in LDS, P_axis; its log2 (a power-of-two line)
  int n3, n5, logQ;       // a mixed-radix line: L = 3^n3 5^n5 2^logQ; n3 = n5 = 0 on a power-of-two line, which k_boxcov_pass runs
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
  int twiddles, Pmax;     // the power-of-two lines' table exp(-2 pi i k / Pmax), k < max(Pmax / 4, 1); Pmax: the largest power-of-two P_c
  fftcov_plan chunks;     // pair_bytes, pairs, chunk_pairs, nchunks (fftcov_plan_chunks)
};

inline bool boxcov_pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }
inline int boxcov_line_len(int64_t n, int boundary) { return boundary == BOXCOV_NEUMANN ? (n > 1 ? (int)(2 * (n - 1)) : 1) : (int)n; }
// L = 3^n3 5^n5 2^logQ with logQ >= 2 and an odd factor: a mixed-radix line
inline bool boxcov_mr_factor(int64_t L, int* n3, int* n5, int* logQ) {
  int a = 0, b = 0, m = 0;
  if (L < 4 || L % 4) return false;
  for (; L % 3 == 0; L /= 3) ++a;
  for (; L % 5 == 0; L /= 5) ++b;
  for (; L % 2 == 0; L /= 2) ++m;
  if (L != 1 || a + b == 0) return false;
  *n3 = a, *n5 = b, *logQ = m;
  return true;
}
// the rule of an axis (the head comment): at least one node, P_c <= 4096, P_c a power of two or a mixed-radix line
inline bool boxcov_axis_ok(int64_t n, int boundary) {
  if (boundary != BOXCOV_NEUMANN && boundary != BOXCOV_PERIODIC) return false;
  if (n < 1 || n > (boundary == BOXCOV_NEUMANN ? BOXCOV_MAX_NEUMANN : BOXCOV_MAX_PERIODIC)) return false;
  const int L = boxcov_line_len(n, boundary);
  int n3, n5, logQ;
  return boxcov_pow2(L) || boxcov_mr_factor(L, &n3, &n5, &logQ);
}

// mode[p]: the mode that position p of a mixed-radix line of L entries holds after the forward stages; pos[m]: its inverse
inline void boxcov_mr_modes(int L, int* mode, int* pos) {
  int n3 = 0, n5 = 0, logQ = 0;
  boxcov_mr_factor(L, &n3, &n5, &logQ);
  for (int p = 0; p < L; ++p) {
    int m = 0, mul = 1, B = L, rest = p;
    for (int s = 0; s < n3 + n5; ++s) {
      const int r = s < n3 ? 3 : 5, sub = B / r;
      m += mul * (rest / sub);
      mul *= r, rest %= sub, B = sub;
    }
    int rev = 0;
    for (int bit = 0; bit < logQ; ++bit) rev |= ((rest >> bit) & 1) << (logQ - 1 - bit);
    mode[p] = m + mul * rev;
    pos[mode[p]] = p;
  }
}

inline int boxcov_pow2floor(int v) {
  int f = 1;
  while (2 * f <= v) f *= 2;
  return f;
}
// the workgroup shape of a mixed-radix pass whose L, stride and nlines are set (the head comment)
inline void boxcov_mr_shape(boxcov_pass& q) {
  int lpw = boxcov_pow2floor(FFTCOV_ELEMS / q.L);
  if (q.stride > 1) {
    int wide = boxcov_pow2floor(FFTCOV_STRIDED_ELEMS / q.L);
    if (wide > 4) wide = 4;
    if (lpw < wide) lpw = wide;
  }
  if (lpw > FFTCOV_MAX_LINES) lpw = FFTCOV_MAX_LINES;
  while (lpw > 1 && lpw / 2 >= q.nlines) lpw /= 2;
  q.lpw = lpw;
  q.loglpw = fftcov_log2(lpw);
  const int pad = lpw == 1 ? 0 : (lpw >= 16 || q.L < 16) ? 1 : 16 / lpw;
  q.ls = q.L + pad;
  q.lds = 16 * (lpw * q.ls + q.L / 4);
  const int64_t items = (int64_t)lpw * q.L / 4;
  int threads = (int)((items + 63) / 64 * 64);
  if (threads < 64) threads = 64;
  if (threads > FFTCOV_MAX_THREADS) threads = FFTCOV_MAX_THREADS;
  q.threads = threads;
  q.grid_x = (q.nlines + lpw - 1) / lpw;
}

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
  if (boxcov_mr_factor(q.L, &q.n3, &q.n5, &q.logQ)) {
    boxcov_mr_shape(q);
    return q;
  }
  fftcov_pass s;          // the workgroup shape of a power-of-two line is the FFT route's rule
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
    if (boxcov_pow2(p.P[c]) && p.P[c] > p.Pmax) p.Pmax = p.P[c];
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

// what k_boxcov_pass and k_boxcov_pass_mr (same static tables) can be launched with; hfmi_box_create refuses a grid with a pass that fails this
inline bool boxcov_pass_launchable(const boxcov_pass& q) {
  return q.lds + BOXCOV_STATIC_LDS <= FFTCOV_LDS_BYTES && q.lpw <= FFTCOV_MAX_LINES && q.threads <= FFTCOV_MAX_THREADS && q.grid_x >= 1 &&
         q.grid_x <= 0x7fffffff;
}

// ------------------------------------------------------------------ hfmi_boxcov_plan_predict's record
// words[BOXCOV_PLAN_WORDS]: a head of 16 words, then 16 per pass.
//   head   0 d  1-3 n_c  4 N  5 pairs  6 pairs per chunk  7 chunks  8 passes  9 bytes per pair  10 entries of the power-of-two lines'
//          twiddle table  11 the largest power-of-two P_c, 1 when no axis has one (a mixed-radix line's own table has line length / 4
//          entries and is not counted here)  12 static LDS of k_boxcov_pass and k_boxcov_pass_mr  13-15 P_c
//   pass   0 axis  1 flags  2 line length  3 mirror  4 extent  5 stride  6 span  7 lines  8 lines per workgroup  9 LDS line stride
//          10 threads  11 dynamic LDS  12 static + dynamic LDS  13 grid x  14 radix-3 stages  15 radix-5 stages (both 0: a power-of-two
//          line, launched as k_boxcov_pass)
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
                                          q.lpw, q.ls, q.threads, q.lds, q.lds + BOXCOV_STATIC_LDS, q.grid_x, q.n3, q.n5};
    memcpy(w + BOXCOV_HEAD_WORDS + i * BOXCOV_PASS_WORDS, v, sizeof(v));
  }
}
