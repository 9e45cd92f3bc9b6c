// Rules of the interpolated grid covariance  K = W Cg W^T + diag(delta)  (hfmi_op_grid_interp, hfmi_op_kernel_cov_interp; kernels in
// hfmi_interp.hip).  Host only, plain C++17, nothing from HIP: the cell of a point, its weights, the argument checks, the cell
// binning the spread walks and the launch shapes.  hfmi_grid_interp_weights (include/hfmi.h) runs the same functions without a device
// and tests/helpers/interp_twin.py states them in numpy.
//
// Grid: d = 1, 2 or 3 axes of n[c] >= 4 nodes, spacing h[c] > 0, origin o[c]; axis 0 fastest, node g = i0 + n0 (i1 + n1 i2).
//
// Cell and weights of a point x, per axis:  u = (x - o) / h in double and 1 <= u <= n - 2 is required;  c = min(floor(u), n - 3),
// t = u - c in [0, 1] (t = 1 only at u = n - 2).  The four weights on the nodes c - 1 .. c + 2 are Keys' cubic convolution with
// a = -1/2, evaluated in exactly these forms (no contraction into fused multiply-adds):
//   w0 = ((2 - t) t - 1) t / 2     w1 = ((3 t - 5) t t + 2) / 2     w2 = ((4 - 3 t) t + 1) t / 2     w3 = (t - 1) t t / 2
// They sum to 1 and reproduce polynomials up to degree 2.  Row i of W holds the 4^d tensor products on the nodes base_i + s0 + n0
// (s1 + n1 s2), base_i the node of the stencil corner (c_a - 1)_a.  The weights are computed HERE, once, and uploaded: the device never
// recomputes one, so whoever calls these functions holds the operator's weights to the last bit.
//
// STENCIL ORDER of every sum over the 4^d nodes of a point (the gather, the twin): s2 outermost, s1, s0 innermost; the weight of node
// (s0, s1, s2) is (w2[s2] * w1[s1]) * w0[s0] in three dimensions, w1[s1] * w0[s0] in two, w0[s0] in one, and each term enters by one
// fused multiply-add, acc = fma(weight, value, acc), from acc = 0.
//
// Cell binning (what makes the spread free of atomics): the stencil base cell of a point is (c_a - 1)_a in the (n0 - 3) x (n1 - 3) x
// (n2 - 3) array of cells, linear index axis 0 fastest.  A counting sort gives cell_start (ncells + 1 entries) and perm (N entries):
// the points of cell q are perm[cell_start[q] .. cell_start[q + 1] - 1], ASCENDING in point index.  The device holds base, weights and
// delta in that binned order, so neighbouring threads of the gather touch neighbouring grid lines.
//
// SPREAD ORDER (part of the contract): grid node g receives from the at most 4^d cells q with q_a in g_a - 3 .. g_a (clipped to the
// array of cells), visited in ascending linear cell index; inside a cell the points in ascending point index; the node is stencil
// position s_a = g_a - q_a of such a point and the term enters as above.  One thread owns a node, so the result depends on no launch
// shape and two applies are bit-identical.
//
// The diagonal  q_i = (W Cg W^T)_ii = sum over stencil pairs of w_s w_s' c(s - s'): the weights enter only through the per-axis
// autocorrelations  a_a[o] = sum_{s - s' = o} w_a[s] w_a[s'], o = 0 .. 3 (s ascending, first term a product, the rest fused
// multiply-adds; a_a[-o] = a_a[o]), so  q_i = sum over the 7^d offsets o of ((a_2[o2] * a_1[o1]) * a_0[o0]) * c(o), o2 outermost, o0
// innermost, each term one fused multiply-add: 7^d terms in place of 16^d, the same number up to rounding.
//
// The factor  F = [ W S | diag(sqrt(delta)) ],  K = F F^T  (hfmi_op_interp_factor), S the grid factor of a sampler's embedding of
// Ptot = prod P_c padded nodes.  NOISE LAYOUT (part of the contract) of the Ptot + N rows F acts on: rows 0 .. Ptot - 1 the padded-grid
// noise in the grid factor's natural order, entry e = s0 + P0 (s1 + P1 s2); rows Ptot .. Ptot + N - 1 one entry per point in POINT
// order, not the binned order above.  (F Xi)_i = fma(sqrt(delta_i), Xi[Ptot + i], (W S Xi_top)_i), the gather's sum first;
// (F^T X)[Ptot + i] = sqrt(delta_i) X[i], one multiplication, rounded before an accumulating apply adds it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

constexpr int INTERP_THREADS = 256;
constexpr int INTERP_SPREAD_COLS = 4;                           // columns a thread of the spread carries per trip over its cells
constexpr int64_t INTERP_MAX_NODES = (int64_t)1 << 40;          // prod n
constexpr int64_t INTERP_MAXN = (int64_t)1 << 23;               // nodes per axis: the long route's cap (FFTCOV_LONG_MAXN)
constexpr int64_t INTERP_WORK_BUDGET = (int64_t)512 << 20;      // bytes of the internal work block of hfmi_op_kernel_cov_interp
constexpr int INTERP_TABLE = 343;                               // 7^3: the kernel at the signed lattice offsets in [-3, 3]^d

enum { INTERP_OK = 0, INTERP_BAD_D, INTERP_BAD_N, INTERP_BAD_H, INTERP_BAD_ORIGIN, INTERP_BAD_SIZE, INTERP_BAD_POINT };

struct interp_grid {
  int d;
  int64_t n[3];       // 1 on the axes the grid does not have
  double h[3], o[3];
  int64_t nc[3];      // cells per axis, n - 3 (1 on the axes the grid does not have)
  int64_t nnodes, ncells;
};

// the grid's own rules; *axis: the offending axis of INTERP_BAD_N / _H / _ORIGIN
inline int interp_grid_check(int d, const int64_t* n, const double* h, const double* origin, interp_grid* g, int* axis) {
  if (d < 1 || d > 3) return INTERP_BAD_D;
  g->d = d;
  g->nnodes = 1, g->ncells = 1;
  for (int c = 0; c < 3; ++c) {
    g->n[c] = 1, g->nc[c] = 1, g->h[c] = 1.0, g->o[c] = 0.0;
    if (c >= d) continue;
    *axis = c;
    if (n[c] < 4 || n[c] > INTERP_MAXN) return INTERP_BAD_N;
    if (!(h[c] > 0.0) || !isfinite(h[c])) return INTERP_BAD_H;
    if (!isfinite(origin[c])) return INTERP_BAD_ORIGIN;
    g->n[c] = n[c], g->nc[c] = n[c] - 3, g->h[c] = h[c], g->o[c] = origin[c];
    if (g->nnodes > INTERP_MAX_NODES / n[c]) return INTERP_BAD_SIZE;
    g->nnodes *= n[c];
    g->ncells *= n[c] - 3;
  }
  return INTERP_OK;
}

// the cell rule of one axis; false: x is not finite or u = (x - o) / h is outside [1, n - 2]
inline bool interp_cell(double x, double o, double h, int64_t n, int64_t* c, double* t) {
#pragma clang fp contract(off)
  const double u = (x - o) / h;
  if (!isfinite(x) || !(u >= 1.0) || !(u <= (double)(n - 2))) return false;
  int64_t cc = (int64_t)floor(u);
  if (cc > n - 3) cc = n - 3;
  *c = cc;
  *t = u - (double)cc;
  return true;
}

// Keys' cubic convolution, a = -1/2, on the nodes c - 1 .. c + 2
inline void interp_keys(double t, double* w) {
#pragma clang fp contract(off)
  w[0] = ((2.0 - t) * t - 1.0) * t / 2.0;
  w[1] = ((3.0 * t - 5.0) * t * t + 2.0) / 2.0;
  w[2] = ((4.0 - 3.0 * t) * t + 1.0) * t / 2.0;
  w[3] = (t - 1.0) * t * t / 2.0;
}

// points: N x d row-major.  base[i]: the node of the stencil corner of point i; w[(i d + a) 4 + s]: its weights; cell[i] (or null):
// its stencil base cell.  INTERP_BAD_POINT names the first offending point and its axis.
inline int interp_weights(const interp_grid& g, const double* points, int64_t N, int64_t* base, double* w, int64_t* cell, int64_t* bad_point,
                          int* bad_axis) {
  for (int64_t i = 0; i < N; ++i) {
    int64_t b = 0, q = 0, nstride = 1, cstride = 1;
    for (int a = 0; a < g.d; ++a) {
      int64_t c;
      double t;
      if (!interp_cell(points[(size_t)i * g.d + a], g.o[a], g.h[a], g.n[a], &c, &t)) {
        *bad_point = i, *bad_axis = a;
        return INTERP_BAD_POINT;
      }
      interp_keys(t, w + ((size_t)i * g.d + a) * 4);
      b += (c - 1) * nstride;
      q += (c - 1) * cstride;
      nstride *= g.n[a];
      cstride *= g.nc[a];
    }
    base[i] = b;
    if (cell) cell[i] = q;
  }
  return INTERP_OK;
}

// counting sort of the points by cell: cell_start[ncells + 1], perm[N] ascending in point index inside a cell
inline void interp_bin(const int64_t* cell, int64_t N, int64_t ncells, int64_t* cell_start, int64_t* perm) {
  for (int64_t q = 0; q <= ncells; ++q) cell_start[q] = 0;
  for (int64_t i = 0; i < N; ++i) ++cell_start[cell[i] + 1];
  for (int64_t q = 0; q < ncells; ++q) cell_start[q + 1] += cell_start[q];
  std::vector<int64_t> next(cell_start, cell_start + ncells);
  for (int64_t i = 0; i < N; ++i) perm[next[(size_t)cell[i]]++] = i;
}

// Launch shape of the three kernels: INTERP_THREADS threads, x over the items (points in binned order, or grid nodes), grid-stride
// beyond 8 workgroups per compute unit; y over the columns (tiles of `tile` columns), as many as keep about that many workgroups in
// flight.  No result depends on it.
struct interp_launch {
  unsigned gx, gy;
};
inline interp_launch interp_launch_shape(int64_t items, int ncols, int tile, int num_cus) {
  const int64_t cap = 8 * (int64_t)(num_cus > 0 ? num_cus : 1);
  int64_t gx = (items + INTERP_THREADS - 1) / INTERP_THREADS;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  const int64_t tiles = ((int64_t)ncols + tile - 1) / tile;
  int64_t gy = cap / gx;
  if (gy > tiles) gy = tiles;
  if (gy > 65535) gy = 65535;
  if (gy < 1) gy = 1;
  return interp_launch{(unsigned)gx, (unsigned)gy};
}

// columns per chunk of the internal work block (ld rows each) of hfmi_op_kernel_cov_interp: even, so that the pairs the grid apply
// forms are those of one call whatever the chunk; forced_pairs > 0 (the tuning key "fftcov_pairs") overrides the budget
inline int interp_chunk_cols(int64_t ld, int ncols, int forced_pairs) {
  int64_t c = forced_pairs > 0 ? 2 * (int64_t)forced_pairs : INTERP_WORK_BUDGET / (8 * ld) / 2 * 2;
  if (c < 2) c = 2;
  if (c > ncols) c = ncols;
  return (int)c;
}
