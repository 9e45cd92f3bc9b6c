// Launch plan of the FFT apply of a kernel covariance on a regular grid (hfmi_op_kernel_cov_grid, hfmi_fftcov.hip).  Host only, plain
// C++17, nothing from HIP: given the grid and the number of vectors the planner fills a plain struct with the embedding lengths, the
// pass list (axis, direction, fused multiply, fused scatter / gather), and for every pass the lines a workgroup takes, its threads, its
// LDS and its grid; and the pairs of columns per chunk of the work buffer from a byte budget.  The launcher plans, then launches what
// the plan says; hfmi_fftcov_plan_predict (include/hfmi.h) writes the same struct out without a device and tests/test_fftcov_plan_cpu.py
// holds it to a Python statement of the rules (tests/helpers/fftcov_plan_twin.py).
//
// The embedding: axis c of n[c] nodes is padded to P_c = the smallest power of two >= 2 n[c] - 1 (1 when n[c] = 1); the work buffer of
// one pair of columns is a complex P_0 x P_1 x P_2 array, axis 0 fastest.  The transforms run in place and leave every axis in the
// digit-reversed order of a decimation-in-frequency FFT; the spectrum is computed by the same passes and is stored in that order, and
// the inverse passes (decimation in time) take that order and return the natural one: nothing is ever permuted.
//
// Passes of an apply in d dimensions (2 d - 1 of them):  forward along axis 0 with the scatter of W fused into its loads, forward
// along 1 .. d - 2, then ONE pass along axis d - 1 that transforms forward, multiplies by Lambda / P and transforms back while the
// line sits in LDS, inverse along d - 2 .. 1, and inverse along axis 0 with the gather into Y fused into its stores.  d = 1 is one
// pass.  What a pass along axis a moves:  the axes below a are in the frequency domain and full (P_b); the axes above a hold data only
// in their first n_b positions (zero padding before their forward pass, the part nobody reads after their inverse pass), so only
// those lines exist for the pass.  Along a itself a pass that starts with the forward transform loads n_a entries and fills the
// rest of the line with zeros in LDS; a pass that ends with the inverse transform stores n_a entries.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

constexpr int FFTCOV_MAXN = 2048;               // nodes per axis: P_c <= 4096, one line fits the LDS of a workgroup
constexpr int FFTCOV_MAXP = 4096;
constexpr int FFTCOV_LDS_BYTES = 163840;        // LDS of a workgroup on gfx950, static + dynamic
constexpr int FFTCOV_MAX_LINES = 256;           // lines per workgroup: the two static tables of k_fftcov_pass (line base, node base)
constexpr int FFTCOV_STATIC_LDS = 2 * 8 * FFTCOV_MAX_LINES;
constexpr int FFTCOV_MAX_THREADS = 512;
constexpr int FFTCOV_MAX_PASSES = 5;
constexpr int FFTCOV_MAX_PAIRS = 4096;          // pairs per chunk: the y extent of a launch grid
constexpr int64_t FFTCOV_DEFAULT_BUDGET = (int64_t)512 << 20;   // bytes of work buffer an apply may take unless told otherwise
constexpr int FFTCOV_ELEMS = 2048;              // complex entries a workgroup aims to hold (short lines: 2048 / L lines)
constexpr int FFTCOV_STRIDED_ELEMS = 8192;      // ... and may hold so that a strided pass takes 4 adjacent lines (64 contiguous bytes)

enum { FFTCOV_FWD = 1, FFTCOV_MUL = 2, FFTCOV_INV = 4, FFTCOV_SCATTER = 8, FFTCOV_GATHER = 16 };

struct fftcov_pass {
  int axis, flags;
  int L, logL;            // line length P_axis
  int64_t stride;         // entries between consecutive positions of a line: the product of P_b over b < axis
  int64_t nlines;         // lines of the pass (per pair)
  int nload, nstore;      // positions of a line that are read (the rest is zero) and written
  int lpw, loglpw;        // lines per workgroup: consecutive line numbers, i.e. adjacent in memory on a strided axis
  int ls;                 // entries between lines in LDS (L + padding)
  int threads;
  int lds;                // dynamic LDS: lpw * ls entries of 16 bytes + the twiddles max(L / 4, 1)
  int64_t grid_x;         // ceil(nlines / lpw); the launch is grid_x x pairs-of-the-chunk
  // line number -> first entry:  inner = line & (stride - 1), o = line / stride, base = inner + (o % oe0) * os0 + (o / oe0) * os1
  int64_t oe0, os0, os1;
};
struct fftcov_plan {
  int d;
  int64_t n[3];
  int P[3];
  int64_t Ptot;
  int npasses;
  fftcov_pass pass[FFTCOV_MAX_PASSES];
  int twiddles;           // entries of the table: exp(-2 pi i k / Pmax), k < max(Pmax / 4, 1)
  int Pmax;
  int64_t pair_bytes;     // work buffer of one pair: 16 Ptot
  int pairs;              // ceil(nvec / 2)
  int chunk_pairs;        // pairs per chunk
  int nchunks;
};

// tuning key "fftcov_pairs": pairs per chunk, 0 = from the byte budget.  Results do not depend on it.
inline int& fftcov_pairs_knob() {
  static int v = 0;
  return v;
}
inline bool fftcov_knob_set(const char* key, int v) {
  if (strcmp(key, "fftcov_pairs") || v < 0 || v > FFTCOV_MAX_PAIRS) return false;
  fftcov_pairs_knob() = v;
  return true;
}

inline int fftcov_embed_len(int64_t n) {
  int P = 1;
  while (P < 2 * n - 1) P *= 2;
  return P;
}
inline int fftcov_log2(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

inline void fftcov_pass_shape(fftcov_pass& q);

// one pass along `axis`; ext[b]: positions of axis b > axis that hold data (n_b for an apply, P_b for the spectrum's own transform)
inline fftcov_pass fftcov_make_pass(const fftcov_plan& p, int axis, int flags, const int64_t* ext, int nload, int nstore) {
  fftcov_pass q;
  memset(&q, 0, sizeof(q));
  q.axis = axis;
  q.flags = flags;
  q.L = p.P[axis];
  q.logL = fftcov_log2(q.L);
  q.stride = 1;
  for (int b = 0; b < axis; ++b) q.stride *= p.P[b];
  const int64_t e1 = axis < 1 ? ext[1] : 1, e2 = axis < 2 ? ext[2] : 1;
  q.nlines = q.stride * e1 * e2;
  q.nload = nload;
  q.nstore = nstore;
  if (axis == 0) q.oe0 = ext[1], q.os0 = p.P[0], q.os1 = (int64_t)p.P[0] * p.P[1];
  else if (axis == 1) q.oe0 = ext[2], q.os0 = (int64_t)p.P[0] * p.P[1], q.os1 = 0;
  else q.oe0 = 1, q.os0 = 0, q.os1 = 0;
  fftcov_pass_shape(q);
  return q;
}

// the workgroup shape of a pass whose L, stride and nlines are set: lines per workgroup, LDS layout, threads, grid
inline void fftcov_pass_shape(fftcov_pass& q) {
  // lines per workgroup: a power of two, so that a strided group never straddles the inner index when stride >= lpw
  int lpw = FFTCOV_ELEMS / q.L;
  if (lpw < 1) lpw = 1;
  if (q.stride > 1) {
    int wide = FFTCOV_STRIDED_ELEMS / q.L;
    if (wide > 4) wide = 4;
    if (lpw < wide) lpw = wide;
  }
  if (lpw > FFTCOV_MAX_LINES) lpw = FFTCOV_MAX_LINES;
  while (lpw > 1 && lpw / 2 >= q.nlines) lpw /= 2;
  q.lpw = lpw;
  q.loglpw = fftcov_log2(lpw);
  // LDS padding between lines: the loads and stores of a strided pass put lpw adjacent lines side by side, and a power-of-two
  // line stride would land them on the same banks; 16 / lpw entries of 16 bytes spread lpw lines x 16 / lpw positions over 256 bytes
  const int pad = lpw == 1 ? 0 : (lpw >= 16 || q.L < 16) ? 1 : 16 / lpw;
  q.ls = q.L + pad;
  q.lds = 16 * (lpw * q.ls + (q.L / 4 > 1 ? q.L / 4 : 1));
  const int64_t items = (int64_t)lpw * q.L / 4;          // radix-4 butterflies of a step
  int threads = (int)((items + 63) / 64 * 64);
  if (threads < 64) threads = 64;
  if (threads > FFTCOV_MAX_THREADS) threads = FFTCOV_MAX_THREADS;
  q.threads = threads;
  q.grid_x = (q.nlines + lpw - 1) / lpw;
}

// the embedding and the passes; spectrum: the d forward passes over the whole padded array that turn the first column into Lambda
inline fftcov_plan fftcov_plan_passes(int d, const int64_t* n, bool spectrum) {
  fftcov_plan p;
  memset(&p, 0, sizeof(p));
  p.d = d;
  p.Ptot = 1;
  p.Pmax = 1;
  for (int c = 0; c < 3; ++c) {
    p.n[c] = c < d ? n[c] : 1;
    p.P[c] = fftcov_embed_len(p.n[c]);
    p.Ptot *= p.P[c];
    if (p.P[c] > p.Pmax) p.Pmax = p.P[c];
  }
  p.twiddles = p.Pmax / 4 > 1 ? p.Pmax / 4 : 1;
  p.pair_bytes = 16 * p.Ptot;
  int64_t ext[3];
  for (int c = 0; c < 3; ++c) ext[c] = spectrum ? p.P[c] : p.n[c];
  int np = 0;
  if (spectrum) {
    for (int a = 0; a < d; ++a) p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_FWD, ext, p.P[a], p.P[a]);
  } else {
    for (int a = 0; a < d - 1; ++a)
      p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_FWD | (a == 0 ? FFTCOV_SCATTER : 0), ext, (int)p.n[a], p.P[a]);
    p.pass[np++] = fftcov_make_pass(p, d - 1, FFTCOV_FWD | FFTCOV_MUL | FFTCOV_INV | (d == 1 ? FFTCOV_SCATTER | FFTCOV_GATHER : 0), ext,
                                    (int)p.n[d - 1], (int)p.n[d - 1]);
    for (int a = d - 2; a >= 0; --a)
      p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_INV | (a == 0 ? FFTCOV_GATHER : 0), ext, p.P[a], (int)p.n[a]);
  }
  p.npasses = np;
  return p;
}

// pairs per chunk: what the budget holds, at least one, at most all and FFTCOV_MAX_PAIRS; forced > 0 (the tuning key) overrides the budget
inline void fftcov_plan_chunks(fftcov_plan& p, int nvec, int64_t budget_bytes, int forced) {
  p.pairs = (nvec + 1) / 2;
  if (budget_bytes <= 0) budget_bytes = FFTCOV_DEFAULT_BUDGET;
  int64_t c = forced > 0 ? forced : budget_bytes / p.pair_bytes;
  if (c > FFTCOV_MAX_PAIRS) c = FFTCOV_MAX_PAIRS;
  if (c > p.pairs) c = p.pairs;
  if (c < 1) c = 1;
  p.chunk_pairs = (int)c;
  p.nchunks = p.pairs > 0 ? (p.pairs + p.chunk_pairs - 1) / p.chunk_pairs : 0;
}

// ------------------------------------------------------------------ hfmi_fftcov_plan_predict's record
constexpr int FFTCOV_HEAD_WORDS = 16;
constexpr int FFTCOV_PASS_WORDS = 16;
constexpr int FFTCOV_PLAN_WORDS = FFTCOV_HEAD_WORDS + FFTCOV_MAX_PASSES * FFTCOV_PASS_WORDS;
inline void fftcov_plan_words(const fftcov_plan& p, int64_t* w) {
  memset(w, 0, sizeof(int64_t) * FFTCOV_PLAN_WORDS);
  const int64_t head[FFTCOV_HEAD_WORDS] = {p.d, p.P[0], p.P[1], p.P[2], p.Ptot, p.pairs, p.chunk_pairs, p.nchunks,
                                           p.npasses, p.pair_bytes, p.twiddles, p.Pmax, FFTCOV_STATIC_LDS, 0, 0, 0};
  memcpy(w, head, sizeof(head));
  for (int i = 0; i < p.npasses; ++i) {
    const fftcov_pass& q = p.pass[i];
    const int64_t v[FFTCOV_PASS_WORDS] = {q.axis, q.flags, q.L, q.stride, q.nlines, q.nload, q.nstore, q.lpw,
                                          q.ls, q.threads, q.lds, q.lds + FFTCOV_STATIC_LDS, q.grid_x, q.oe0, q.os0, q.os1};
    memcpy(w + FFTCOV_HEAD_WORDS + i * FFTCOV_PASS_WORDS, v, sizeof(v));
  }
}

// ------------------------------------------------------------------ the draw m ~ N(0, C) by circulant embedding (hfmi_grid_sampler_*)
// A draw is the inverse half of an apply fed with coloured noise:  z = IFFT_unnormalised( sqrt(max(Lambda / P, 0)) (xi_1 + i xi_2) ) with
// xi i.i.d. N(0, 1) on the padded grid; Re z and Im z on the nodes are two independent draws (Dietrich-Newsam, Wood-Chan).  Lambda's
// storage order is arbitrary to i.i.d. noise, so nothing is permuted here either.  The square root needs a non-negative spectrum, which the
// minimal embedding often lacks, so the sampler has an embedding of its own:  growth g doubles every P_c with n_c > 1 g times,
// P_c = fftcov_embed_len(n_c) << g, feasible while every P_c <= FFTCOV_MAXP.
//
// Passes of a draw in d dimensions (d of them):  ONE pass along axis d - 1 whose load is GENERATED (FFTCOV_GEN: no operand is read but
// Lambda), runs the inverse stages and stores n_{d-1} positions -- its lines are those of the apply's middle pass, every position of
// the axes below -- then the apply's inverse passes along d - 2 .. 0, the last with the gather fused.  d = 1: generate, inverse, gather.
// Pairs per chunk as fftcov_plan_chunks.
//
// The noise's element map (hfmi_randn_math.h has the probe draw's; oracle/philox.py is the checker of the integer stream): storage
// entries 2 q and 2 q + 1 of pair p's padded array (entry e = s_0 + P_0 (s_1 + P_1 s_2), s_c the storage position along axis c) take one
// Philox output,  x = philox4x32_10(ctr = (q lo, q hi, p, FFTCOV_GEN_STREAM), key = (seed lo, seed hi)),  (z_0 .. z_3) = box_muller4(x):
// entry 2 q is sqrt(max(lambda[2 q], 0)) (z_0 + i z_1), entry 2 q + 1 is sqrt(max(lambda[2 q + 1], 0)) (z_2 + i z_3); prod P_c = 1 has the
// single entry 0.  It depends on (seed, pair, storage position) only: lines per workgroup, chunks and "fftcov_pairs" change no bit.  Adjacent
// storage entries are adjacent positions of a line on the contiguous axis and adjacent lines of a workgroup on a strided one (a strided
// pass takes >= 2 lines, line numbers from an even one), so one thread always holds both and all four normals are used.
//
// Eigenvalues that are negative only by rounding:  floor = FFTCOV_FLOOR_C eps log2(prod P_c) lambda_max; entries in [-floor, 0) become 0
// silently, an embedding whose lambda_min < -floor is indefinite.  FFTCOV_FLOOR_C = 16: in fp64 the squared exponential's spectra that
// are zero to working precision come out (numpy's FFT) at -1.7e-16 (8 x 8, spacing 1/8, ell 0.4, g = 2, 3) and at -5.4e-16 / -0.9e-16
// (33 nodes, spacing 1/32, ell 1, g = 2 / 3) of lambda_max, i.e. 0.04 to 0.27 of eps log2(prod P_c), while the smallest genuine negative
// of the same grids (8 x 8, g = 1: -3.7e-7) is 1.7e8 of them: 16 leaves a factor 60 over the rounding seen, for the device's own
// transform of the column, and 1e7 under anything real (tests/test_grid_sampler_twin_cpu.py asserts a factor 16 and 1e6).
//
// Clipping (the caller asked for it and no growth was definite): all negative entries are set to 0.  The covariance of the draw is then
// C + E, E the restriction of the circulant with the spectrum -min(Lambda, 0): a positive semidefinite circulant, whose entries are
// bounded in magnitude by its constant diagonal  sum |lambda^-| / prod P_c  = minus the sum of the stored negative Lambda / P.  That sum
// is cov_error_bound: |Cov(draw) - C|_ij <= cov_error_bound for every i, j.
enum { FFTCOV_GEN = 32 };
constexpr uint32_t FFTCOV_GEN_STREAM = 0x67726964u;   // "grid": counter word 3 of the noise
constexpr int FFTCOV_MAX_GROWTH = 3;
constexpr double FFTCOV_FLOOR_C = 16.0;

// tuning key "fftcov_min_growth": the growth a sampler's creation tries first (tests and measurements: a larger embedding than the rule takes)
inline int& fftcov_min_growth_knob() {
  static int v = 0;
  return v;
}
inline bool fftcov_sample_knob_set(const char* key, int v) {
  if (strcmp(key, "fftcov_min_growth") || v < 0 || v > FFTCOV_MAX_GROWTH) return false;
  fftcov_min_growth_knob() = v;
  return true;
}

inline bool fftcov_growth_feasible(int d, const int64_t* n, int growth) {
  if (growth < 0 || growth > FFTCOV_MAX_GROWTH) return false;
  for (int c = 0; c < d; ++c)
    if (n[c] > 1 && ((int64_t)fftcov_embed_len(n[c]) << growth) > FFTCOV_MAXP) return false;
  return true;
}
inline double fftcov_floor(int64_t Ptot, double lambda_max) {
  const int l = fftcov_log2(Ptot);
  return FFTCOV_FLOOR_C * 2.220446049250313e-16 * (double)(l > 1 ? l : 1) * lambda_max;
}

// the grown embedding of a sampler: P_c, their product, the twiddle table and the work buffer of one pair; no passes yet
inline fftcov_plan fftcov_grown_embedding(int d, const int64_t* n, int growth) {
  fftcov_plan p;
  memset(&p, 0, sizeof(p));
  p.d = d;
  p.Ptot = 1;
  p.Pmax = 1;
  for (int c = 0; c < 3; ++c) {
    p.n[c] = c < d ? n[c] : 1;
    p.P[c] = p.n[c] > 1 ? fftcov_embed_len(p.n[c]) << growth : 1;
    p.Ptot *= p.P[c];
    if (p.P[c] > p.Pmax) p.Pmax = p.P[c];
  }
  p.twiddles = p.Pmax / 4 > 1 ? p.Pmax / 4 : 1;
  p.pair_bytes = 16 * p.Ptot;
  return p;
}

// the grown embedding and the passes of a draw; spectrum: the d forward passes over the whole padded array, as fftcov_plan_passes
inline fftcov_plan fftcov_sample_plan_passes(int d, const int64_t* n, int growth, bool spectrum) {
  fftcov_plan p = fftcov_grown_embedding(d, n, growth);
  int64_t ext[3];
  for (int c = 0; c < 3; ++c) ext[c] = spectrum ? p.P[c] : p.n[c];
  int np = 0;
  if (spectrum) {
    for (int a = 0; a < d; ++a) p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_FWD, ext, p.P[a], p.P[a]);
  } else {
    p.pass[np++] = fftcov_make_pass(p, d - 1, FFTCOV_GEN | FFTCOV_INV | (d == 1 ? FFTCOV_GATHER : 0), ext, p.P[d - 1], (int)p.n[d - 1]);
    for (int a = d - 2; a >= 0; --a)
      p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_INV | (a == 0 ? FFTCOV_GATHER : 0), ext, p.P[a], (int)p.n[a]);
  }
  p.npasses = np;
  return p;
}

// hfmi_fftcov_sample_plan_predict's record: the words of fftcov_plan_words, word 13 = the growth
inline void fftcov_sample_plan_words(const fftcov_plan& p, int growth, int64_t* w) {
  fftcov_plan_words(p, w);
  w[13] = growth;
}

// ------------------------------------------------------------------ the factor C = S S^T of a sampler's embedding (hfmi_op_grid_factor)
// The embedding circulant Chat of a sampler has a non-negative (or clipped) spectrum, so its symmetric square root is a circulant too,
// applied by the passes of an apply with a ROOT TABLE sqrt(max(lambda, 0) / prod P_c) in place of lambda (lambda: the stored
// Lambda / prod P_c, same order, nothing permuted):  Chat^(1/2) xi = IFFT_unnormalised( root . FFT(xi) ).  With Rn the restriction to
// the nodes,  S = Rn Chat^(1/2)  is N x prod P_c and S S^T = Rn Chat Rn^T = C exactly (C + E with |E_ij| <= cov_error_bound when clipped),
// and  S^T = Chat^(1/2) Rn^T.  A padded vector is an ordinary block of length prod P_c in natural order, entry
// e = s_0 + P_0 (s_1 + P_1 s_2): the scatter / gather path of a pass with NO node map and n0 = P_0 is exactly the direct load / store
// of such a block (FFTCOV_LOAD_FULL / FFTCOV_STORE_FULL say on which side of the pass the block of padded vectors is).
//
// Passes (2 d - 1 per pair of columns, pairs per chunk as fftcov_plan_chunks):
//   S    forward along 0 .. d - 2 over ALL lines (every axis above holds data in its P_b positions), the first loading P_0 positions
//        straight from the input block; the fused pass along d - 1 loads P_{d-1}, multiplies by the root table and stores n_{d-1};
//        then the apply's own inverse passes (lines of the first n_b positions only), the last gathering through the node map.
//   S^T  the apply's own forward passes (scatter through the node map, zero fill); the fused pass along d - 1 loads n_{d-1} and stores
//        P_{d-1}; then inverse along d - 2 .. 0 over ALL lines, the last storing P_0 positions straight into the output block.
// d = 1 is the one fused pass, whose load and store sit on different sides: the only pass that k_fftcov_pass cannot run as it stands
// (one node map serves its load and its store); k_fftcov_factor is the same body with the map dropped on the full side.
enum { FFTCOV_LOAD_FULL = 64, FFTCOV_STORE_FULL = 128 };

inline fftcov_plan fftcov_factor_plan_passes(int d, const int64_t* n, int growth, int transpose) {
  fftcov_plan p = fftcov_grown_embedding(d, n, growth);
  int64_t full[3], data[3];
  for (int c = 0; c < 3; ++c) full[c] = p.P[c], data[c] = p.n[c];
  const int64_t* fwd_ext = transpose ? data : full;   // lines of the forward half / of the inverse half
  const int64_t* inv_ext = transpose ? full : data;
  const int load_side = transpose ? 0 : FFTCOV_LOAD_FULL, store_side = transpose ? FFTCOV_STORE_FULL : 0;
  auto in_len = [&](int a) { return transpose ? (int)p.n[a] : p.P[a]; };     // positions of a line on the input's side of the multiply
  auto out_len = [&](int a) { return transpose ? p.P[a] : (int)p.n[a]; };    // ... and on the output's
  int np = 0;
  for (int a = 0; a < d - 1; ++a)
    p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_FWD | (a == 0 ? FFTCOV_SCATTER | load_side : 0), fwd_ext, in_len(a), p.P[a]);
  p.pass[np++] = fftcov_make_pass(p, d - 1, FFTCOV_FWD | FFTCOV_MUL | FFTCOV_INV | (d == 1 ? FFTCOV_SCATTER | FFTCOV_GATHER | load_side | store_side : 0),
                                  data, in_len(d - 1), out_len(d - 1));
  for (int a = d - 2; a >= 0; --a)
    p.pass[np++] = fftcov_make_pass(p, a, FFTCOV_INV | (a == 0 ? FFTCOV_GATHER | store_side : 0), inv_ext, p.P[a], out_len(a));
  p.npasses = np;
  return p;
}

// hfmi_fftcov_factor_plan_predict's record: the words of fftcov_plan_words, word 13 = the growth, word 14 = transpose
inline void fftcov_factor_plan_words(const fftcov_plan& p, int growth, int transpose, int64_t* w) {
  fftcov_plan_words(p, w);
  w[13] = growth;
  w[14] = transpose;
}

// ------------------------------------------------------------------ split-line passes: embedding axes longer than a workgroup's line
// The long route (hfmi_op_kernel_cov_grid_long, hfmi_grid_sampler_create_long; the factor of its samplers).  Everything above holds for
// it; what it adds is that an embedding axis c with P_c > max_line (tuning key "fftcov_max_line", a power of two in 4 .. 4096, default
// 4096, read by this route alone when it plans) is SPLIT into two sub-axes, P_c = L1 L2, both at most max_line.  Position s of the axis
// is s = L2 n1 + n2: n2 < L2 the LOW sub-axis (the axis's own stride S_c = prod P_b, b < c), n1 < L1 the HIGH one (stride S_c L2).
// Bailey's four-step without transposes:
//   forward   L1-point DFTs along the high sub-axis (one line per n2; decimation in frequency, so position p of a line holds
//             k1 = bitrev_L1(p)), the twiddle exp(-2 pi i n2 k1 / P_c) multiplied in at that pass's store;  then L2-point DFTs along the
//             low sub-axis (one line per k1).  Position L2 p1 + p2 then holds X[bitrev_L1(p1) + L1 bitrev_L2(p2)] = X[bitrev_Pc(L2 p1 + p2)]:
//             exactly the digit-reversed order of one P_c-point pass, so Lambda, the root table, the extremes and the noise's element
//             map are stored as on the old route and nothing is permuted.
//   inverse   L2-point inverse along the low sub-axis, then the conjugate twiddle multiplied in at the LOAD of the L1-point inverse along
//             the high one.
// The twiddle is sincospi(-2 n2 k1 / P_c) on the device: n2 k1 < P_c <= 2^24 and the division by a power of two are exact.
// Split rule: L2 = max_line, L1 = P_c / max_line (>= 2, and <= max_line while P_c <= max_line^2).  The high sub-axis is always strided; the
// shorter its lines the more of them a workgroup takes side by side (fftcov_pass_shape: 2048 / L, at least 4), i.e. the wider the
// contiguous runs of its loads and stores, while the low sub-axis of axis 0 is contiguous at any length.  So the strided part is made as
// short as the LDS line allows the other to be long.
//
// The pass list is the old route's with every split axis taking two passes in place of one: forward along 0 .. d - 1 (a split axis:
// high, then low), the last forward (sub-)pass fused with the multiply and the inverse, inverse back to axis 0 (a split axis: low, then
// high).  2 (d + s) - 1 passes with s split axes, at most 11.  Passes along an axis that is not split are fftcov_make_pass's, launched by
// k_fftcov_pass / k_fftcov_draw as they are; with no split axis the plan IS the old planner's, pass for pass, so applies, draws and
// factors are bit-identical to the old route's.  The pass properties extend to sub-axes:
//   lines that are all padding are skipped   a line number is  inner + S_c (sub + esub o):  inner < S_c the positions below the axis (all
//                                             in the frequency domain), sub < esub the other sub-axis, o the lines of the axes above as
//                                             ever (oe0, os0, os1).  High passes on the time-domain side exist for n2 < esub = min(L2, n_c)
//                                             only (n2 >= n_c is padding at every n1); low passes take all L1 values of k1.
//   zero fill happens in LDS                  as ever: positions that are not loaded are zeros in LDS.
//   loads and stores are limited to n         the axis position of line position p is  p pm + sub sm  (high: pm = L2, sm = 1; low: pm = 1,
//                                             sm = 0) and is loaded / stored while it is below nload / nstore: n_c (or P_c) on a high pass,
//                                             min(L2, n_c) (or L2) on a low one.  The scatter and the gather of axis 0 address node
//                                             o n_0 + that position.
// The generated load of a draw is a low pass when the last axis is split: its lines are whole low lines (a contiguous line of L2 >= 4
// positions, or >= 2 adjacent lines on a strided axis from an even line number), so storage entries 2 q and 2 q + 1 stay in one thread.
// Caps: nodes per axis <= 2^23, every P_c <= max_line^2 (so P_c <= 2^24), growth 0 .. 6 for a sampler.
constexpr int64_t FFTCOV_LONG_MAXN = (int64_t)1 << 23;
constexpr int FFTCOV_LONG_MAX_LINE = 4096;
constexpr int FFTCOV_LONG_MIN_LINE = 4;
constexpr int FFTCOV_LONG_MAX_GROWTH = 6;
constexpr int FFTCOV_LONG_MAX_PASSES = 11;
constexpr int FFTCOV_LONG_STATIC_LDS = FFTCOV_STATIC_LDS + 4 * FFTCOV_MAX_LINES;   // k_fftcov_split adds a table of line offsets
enum { FFTCOV_TW_STORE = 256, FFTCOV_TW_LOAD = 512 };
enum { FFTCOV_WHOLE = 0, FFTCOV_HI = 1, FFTCOV_LO = 2 };
enum { FFTCOV_KIND_APPLY = 0, FFTCOV_KIND_DRAW = 1, FFTCOV_KIND_FACTOR = 2, FFTCOV_KIND_FACTOR_T = 3, FFTCOV_KIND_SPECTRUM = 4 };

struct fftcov_sub {       // what a pass along a sub-axis adds to its fftcov_pass
  int part;               // FFTCOV_WHOLE, FFTCOV_HI, FFTCOV_LO
  int L1, L2;             // the axis's split
  int logP;               // log2 P_axis
  int64_t inner;          // S_axis: positions below the axis, the lowest part of a line number
  int64_t esub;           // values of the other sub-axis that lines exist for
  int64_t sub_stride;     // entries between consecutive values of it
  int pm, sm;             // axis position of (line position p, sub) = p pm + sub sm
};
struct fftcov_long_plan {
  fftcov_plan base;       // embedding, chunks, pair bytes; twiddles / Pmax of the longest LINE; base.npasses = 0
  int max_line;
  int L1[3], L2[3];       // L1 = 1: the axis is not split, L2 = P_c
  int nsplit;
  int npasses;
  fftcov_pass pass[FFTCOV_LONG_MAX_PASSES];
  fftcov_sub sub[FFTCOV_LONG_MAX_PASSES];
};

// tuning key "fftcov_max_line"
inline int& fftcov_max_line_knob() {
  static int v = FFTCOV_LONG_MAX_LINE;
  return v;
}
inline bool fftcov_max_line_ok(int v) { return v >= FFTCOV_LONG_MIN_LINE && v <= FFTCOV_LONG_MAX_LINE && (v & (v - 1)) == 0; }
inline bool fftcov_long_knob_set(const char* key, int v) {
  if (strcmp(key, "fftcov_max_line") || !fftcov_max_line_ok(v)) return false;
  fftcov_max_line_knob() = v;
  return true;
}

// the long route's embedding at a growth: feasible when every P_c <= max_line^2
inline bool fftcov_long_feasible(int d, const int64_t* n, int growth, int max_line) {
  if (growth < 0 || growth > FFTCOV_LONG_MAX_GROWTH || !fftcov_max_line_ok(max_line)) return false;
  for (int c = 0; c < d; ++c) {
    if (n[c] < 1 || n[c] > FFTCOV_LONG_MAXN) return false;
    if (n[c] > 1 && ((int64_t)fftcov_embed_len(n[c]) << growth) > (int64_t)max_line * max_line) return false;
  }
  return true;
}

inline fftcov_long_plan fftcov_long_embedding(int d, const int64_t* n, int growth, int max_line) {
  fftcov_long_plan p;
  memset(&p, 0, sizeof(p));
  p.base = fftcov_grown_embedding(d, n, growth);     // growth 0: fftcov_embed_len of every axis, as fftcov_plan_passes
  p.max_line = max_line;
  int Lmax = 1;
  for (int c = 0; c < 3; ++c) {
    const int P = p.base.P[c];
    p.L1[c] = P > max_line ? P / max_line : 1;
    p.L2[c] = P > max_line ? max_line : P;
    p.nsplit += p.L1[c] > 1;
    if (p.L2[c] > Lmax) Lmax = p.L2[c];
  }
  p.base.Pmax = Lmax;
  p.base.twiddles = Lmax / 4 > 1 ? Lmax / 4 : 1;
  return p;
}

// one pass along (a part of) `axis`.  ext[b], b > axis: positions of the axes above that hold data; ext[axis]: the axis's own positions
// that hold data on the time-domain side of a high pass.  nload / nstore: axis positions on a high pass, line positions otherwise.
inline void fftcov_long_add(fftcov_long_plan& p, int axis, int part, int flags, const int64_t* ext, int64_t nload, int64_t nstore) {
  fftcov_sub s;
  memset(&s, 0, sizeof(s));
  s.part = part;
  s.L1 = p.L1[axis], s.L2 = p.L2[axis];
  s.logP = fftcov_log2(p.base.P[axis]);
  fftcov_pass q;
  if (part == FFTCOV_WHOLE) {
    q = fftcov_make_pass(p.base, axis, flags, ext, (int)nload, (int)nstore);
    s.inner = q.stride, s.esub = 1, s.pm = 1;
  } else {
    memset(&q, 0, sizeof(q));
    q.axis = axis;
    q.flags = flags;
    int64_t S = 1;
    for (int b = 0; b < axis; ++b) S *= p.base.P[b];
    s.inner = S;
    if (part == FFTCOV_HI) {
      q.L = s.L1, q.stride = S * s.L2;
      s.esub = ext[axis] < s.L2 ? ext[axis] : s.L2, s.sub_stride = S, s.pm = s.L2, s.sm = 1;
    } else {
      q.L = s.L2, q.stride = S;
      s.esub = s.L1, s.sub_stride = S * s.L2, s.pm = 1, s.sm = 0;
    }
    q.logL = fftcov_log2(q.L);
    const int64_t e1 = axis < 1 ? ext[1] : 1, e2 = axis < 2 ? ext[2] : 1;
    q.nlines = S * s.esub * e1 * e2;
    q.nload = (int)nload;
    q.nstore = (int)nstore;
    if (axis == 0) q.oe0 = ext[1], q.os0 = p.base.P[0], q.os1 = (int64_t)p.base.P[0] * p.base.P[1];
    else if (axis == 1) q.oe0 = ext[2], q.os0 = (int64_t)p.base.P[0] * p.base.P[1], q.os1 = 0;
    else q.oe0 = 1, q.os0 = 0, q.os1 = 0;
    fftcov_pass_shape(q);
  }
  p.pass[p.npasses] = q;
  p.sub[p.npasses] = s;
  ++p.npasses;
}

// the forward passes along `axis` (first_flags on its first pass, the high one of a split axis); last: the final forward part is
// left out (the fused pass takes it)
inline void fftcov_long_forward(fftcov_long_plan& p, int axis, int first_flags, const int64_t* ext, int64_t in_len, bool last) {
  const int64_t P = p.base.P[axis];
  if (p.L1[axis] == 1) {
    if (!last) fftcov_long_add(p, axis, FFTCOV_WHOLE, FFTCOV_FWD | first_flags, ext, in_len, P);
    return;
  }
  int64_t e[3] = {ext[0], ext[1], ext[2]};
  e[axis] = in_len;
  fftcov_long_add(p, axis, FFTCOV_HI, FFTCOV_FWD | FFTCOV_TW_STORE | first_flags, e, in_len, P);
  const int64_t L2 = p.L2[axis];     // the high pass wrote the lines n2 < min(L2, in_len) only
  if (!last) fftcov_long_add(p, axis, FFTCOV_LO, FFTCOV_FWD, ext, in_len < L2 ? in_len : L2, L2);
}
// the inverse passes along `axis` (last_flags on its last pass, the high one of a split axis); first: the first inverse part is left
// out (the fused or the generated pass took it)
inline void fftcov_long_inverse(fftcov_long_plan& p, int axis, int last_flags, const int64_t* ext, int64_t out_len, bool first) {
  const int64_t P = p.base.P[axis];
  if (p.L1[axis] == 1) {
    if (!first) fftcov_long_add(p, axis, FFTCOV_WHOLE, FFTCOV_INV | last_flags, ext, P, out_len);
    return;
  }
  const int64_t L2 = p.L2[axis];
  if (!first) fftcov_long_add(p, axis, FFTCOV_LO, FFTCOV_INV, ext, L2, out_len < L2 ? out_len : L2);
  int64_t e[3] = {ext[0], ext[1], ext[2]};
  e[axis] = out_len;
  fftcov_long_add(p, axis, FFTCOV_HI, FFTCOV_INV | FFTCOV_TW_LOAD | last_flags, e, P, out_len);
}
// the one pass along the last axis that the two halves share: fused forward-multiply-inverse, or the generated inverse of a draw
inline void fftcov_long_middle(fftcov_long_plan& p, int flags, int extra_whole, const int64_t* ext, int64_t in_len, int64_t out_len) {
  const int a = p.base.d - 1;
  if (p.L1[a] == 1) {
    fftcov_long_add(p, a, FFTCOV_WHOLE, flags | extra_whole, ext, in_len, out_len);
  } else {
    const int64_t L2 = p.L2[a];
    fftcov_long_add(p, a, FFTCOV_LO, flags, ext, in_len < L2 ? in_len : L2, out_len < L2 ? out_len : L2);
  }
}

// The passes of one kind (FFTCOV_KIND_*) of the long route; the caller has checked fftcov_long_feasible.  Apply and factor: as
// fftcov_plan_passes / fftcov_factor_plan_passes; draw: as fftcov_sample_plan_passes; spectrum: the forward passes over the whole array.
inline fftcov_long_plan fftcov_long_plan_passes(int kind, int d, const int64_t* n, int growth, int max_line) {
  fftcov_long_plan p = fftcov_long_embedding(d, n, growth, max_line);
  int64_t full[3], data[3];
  for (int c = 0; c < 3; ++c) full[c] = p.base.P[c], data[c] = p.base.n[c];
  if (kind == FFTCOV_KIND_SPECTRUM) {
    for (int a = 0; a < d; ++a) fftcov_long_forward(p, a, 0, full, full[a], false);
    return p;
  }
  if (kind == FFTCOV_KIND_DRAW) {
    const int a = d - 1;
    const int gather = d == 1 ? FFTCOV_GATHER : 0;
    fftcov_long_middle(p, FFTCOV_GEN | FFTCOV_INV, gather, data, full[a], data[a]);
    if (p.L1[a] > 1) fftcov_long_inverse(p, a, gather, data, data[a], true);
    for (int b = d - 2; b >= 0; --b) fftcov_long_inverse(p, b, b == 0 ? FFTCOV_GATHER : 0, data, data[b], false);
    return p;
  }
  const int transpose = kind == FFTCOV_KIND_FACTOR_T;
  const bool factor = kind == FFTCOV_KIND_FACTOR || transpose;
  const int64_t* fwd_ext = factor && !transpose ? full : data;
  const int64_t* inv_ext = factor && transpose ? full : data;
  const int load_side = factor && !transpose ? FFTCOV_LOAD_FULL : 0, store_side = transpose ? FFTCOV_STORE_FULL : 0;
  auto in_len = [&](int a) { return factor && !transpose ? full[a] : data[a]; };
  auto out_len = [&](int a) { return transpose ? full[a] : data[a]; };
  for (int a = 0; a < d; ++a) fftcov_long_forward(p, a, a == 0 ? FFTCOV_SCATTER | load_side : 0, fwd_ext, in_len(a), a == d - 1);
  fftcov_long_middle(p, FFTCOV_FWD | FFTCOV_MUL | FFTCOV_INV, d == 1 ? FFTCOV_SCATTER | FFTCOV_GATHER | load_side | store_side : 0, data,
                     in_len(d - 1), out_len(d - 1));
  for (int a = d - 1; a >= 0; --a) fftcov_long_inverse(p, a, a == 0 ? FFTCOV_GATHER | store_side : 0, inv_ext, out_len(a), a == d - 1);
  return p;
}

// ------------------------------------------------------------------ hfmi_fftcov_long_plan_predict's record
// words[FFTCOV_LONG_PLAN_WORDS]: a head of 16 words, then 24 per pass.
//   head   0 d  1-3 P_c  4 prod P_c  5 pairs  6 pairs per chunk  7 chunks  8 passes  9 bytes per pair  10 twiddles  11 the longest line
//          12 static LDS of k_fftcov_split  13 growth  14 kind  15 max_line
//   pass   0-15 the words of fftcov_plan_words (word 11: dynamic + the static LDS of the kernel that runs it: k_fftcov_pass's for a whole
//          axis, k_fftcov_split's for a sub-axis)  16 part  17 L1  18 L2  19 inner  20 esub  21 sub_stride  22 pm  23 sm
constexpr int FFTCOV_LONG_HEAD_WORDS = 16;
constexpr int FFTCOV_LONG_PASS_WORDS = 24;
constexpr int FFTCOV_LONG_PLAN_WORDS = FFTCOV_LONG_HEAD_WORDS + FFTCOV_LONG_MAX_PASSES * FFTCOV_LONG_PASS_WORDS;
inline void fftcov_long_plan_words(const fftcov_long_plan& lp, int growth, int kind, int64_t* w) {
  memset(w, 0, sizeof(int64_t) * FFTCOV_LONG_PLAN_WORDS);
  const fftcov_plan& p = lp.base;
  const int64_t head[FFTCOV_LONG_HEAD_WORDS] = {p.d, p.P[0], p.P[1], p.P[2], p.Ptot, p.pairs, p.chunk_pairs, p.nchunks,
                                                lp.npasses, p.pair_bytes, p.twiddles, p.Pmax, FFTCOV_LONG_STATIC_LDS, growth, kind, lp.max_line};
  memcpy(w, head, sizeof(head));
  for (int i = 0; i < lp.npasses; ++i) {
    const fftcov_pass& q = lp.pass[i];
    const fftcov_sub& s = lp.sub[i];
    const int st = s.part == FFTCOV_WHOLE ? FFTCOV_STATIC_LDS : FFTCOV_LONG_STATIC_LDS;
    const int64_t v[FFTCOV_LONG_PASS_WORDS] = {q.axis, q.flags, q.L, q.stride, q.nlines, q.nload, q.nstore, q.lpw,
                                               q.ls, q.threads, q.lds, q.lds + st, q.grid_x, q.oe0, q.os0, q.os1,
                                               s.part, s.L1, s.L2, s.inner, s.esub, s.sub_stride, s.pm, s.sm};
    memcpy(w + FFTCOV_LONG_HEAD_WORDS + i * FFTCOV_LONG_PASS_WORDS, v, sizeof(v));
  }
}
