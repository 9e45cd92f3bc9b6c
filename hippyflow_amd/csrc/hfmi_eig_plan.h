// Launch plan of the whole-GPU symmetric eigensolver (sym_eig_large, hfmi_eig_blocked.hip).  Host only, plain C++17, nothing from
// HIP: given n, the knobs and the LDS figures of the device, eig_plan_make fills a plain struct with the route, the geometry, the
// workspace as one table of regions and the deflation kernel of every merge level; eig_tri_walk states the launch sequence of the
// tridiagonalisation once and hands every step to a visitor.  The driver's visitor launches what a step says;
// hfmi_eig_plan_predict (include/hfmi.h) runs the same plan and the same walk with a counting visitor, without a device, so that
// tests/test_eig_plan_cpu.py can sweep every n.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

constexpr int EB_NB = 64;          // panel width of the tridiagonalisation and of the block reflectors
constexpr int EB_MAXN = 16384;     // HFMI_EIG_MAXN: v of k_tri_b lives in LDS (128 KB of 160)
constexpr int EB_TS = 128;         // tile of the lower-triangle products (k_tri_bs)
constexpr int EB_UNB_CAP = 2304;   // rows of LDS vectors of k_tri_u: (cap + 63 + 127 rounded to 128) * 24 bytes <= 64 KB
constexpr int EB_MAX_LEVELS = 7;   // at most 128 leaves: the merges' node records (device workspace and pinned copy) hold 64 nodes
constexpr int EB_NODES = 64;
constexpr int EB_NODE_BYTES = 40;  // sizeof(dcl_node)

// ------------------------------------------------------------------ knobs
// The environment switches of the driver, one instance per process, read once when the instance is first used.
// (HFMI_EIG_GEMM belongs to hfmi_dgemm.hip.)
struct eig_knobs {
  bool jacobi;          // HFMI_EIG_LARGE=jacobi: the one-kernel-per-sweep Jacobi, up to n = 4096 (the A/B route of round 4 stops there)
  int wy;               // HFMI_EIG_WY = 256 | 512: width of a block reflector of the back-transformation (0: automatic)
  bool ld_pad;          // off with HFMI_EIG_NO_LD_PAD: no +144 on a power-of-two leading dimension
  int tri_unr;          // HFMI_EIG_TRI_UNR = 4 | 8: 16-byte loads in flight per lane of k_tri_b (A/B)
  int sym_min;          // HFMI_EIG_SYM_MIN: trailing blocks from this size on take the lower-triangle products (0: never)
  int unb_max;          // HFMI_EIG_UNB_MAX: trailing blocks of at most this many rows take one launch per column (0: never)
  bool lower_updates;   // off with HFMI_EIG_FULL_UPDATE (A/B): every rank-2k update over the full block
  int leaf_max;         // HFMI_EIG_LEAF = 64 ... 256: largest leaf handed to the one-workgroup solver (A/B)
  bool timing;          // HFMI_EIG_LARGE_TIMING: phase times on stderr (a stream synchronisation per phase)
};
// on when set to anything but "" or "0" (env_flag of hfmi_internal.h)
inline bool eig_env_flag(const char* name) {
  const char* e = getenv(name);
  return e && e[0] && !(e[0] == '0' && e[1] == 0);
}
inline const eig_knobs& eig_knobs_ref() {
  static const eig_knobs kn = [] {
    auto num = [](const char* name, int unset) {
      const char* e = getenv(name);
      return e ? atoi(e) : unset;
    };
    auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; };
    eig_knobs k;
    const char* route = getenv("HFMI_EIG_LARGE");
    k.jacobi = route && !strcmp(route, "jacobi");
    const int wy = num("HFMI_EIG_WY", 0);
    k.wy = (wy == 256 || wy == 512) ? wy : 0;
    k.ld_pad = !eig_env_flag("HFMI_EIG_NO_LD_PAD");
    k.tri_unr = num("HFMI_EIG_TRI_UNR", 0) == 4 ? 4 : 8;
    const int sm = num("HFMI_EIG_SYM_MIN", 3072);
    k.sym_min = sm <= 0 ? (1 << 30) : (sm > 256 ? sm : 256);
    k.unb_max = clamp(num("HFMI_EIG_UNB_MAX", 2048), 0, EB_UNB_CAP);
    k.lower_updates = !eig_env_flag("HFMI_EIG_FULL_UPDATE");
    const int leaf = num("HFMI_EIG_LEAF", 0);
    k.leaf_max = (leaf >= 64 && leaf <= 256) ? leaf : 128;   // 128: n = 512 / 1024 5.65 / 11.5 ms against 6.06 / 11.9 with 256-row leaves, equal beyond
    k.timing = eig_env_flag("HFMI_EIG_LARGE_TIMING");
    return k;
  }();
  return kn;
}

// ------------------------------------------------------------------ workspace
// Every region of the one workspace, in the order it is laid out: X(name, element, count).  Elements: D double, I int, B byte,
// N node record (EB_NODE_BYTES, 16-byte aligned).  The counts are written in the locals of eig_plan_make.  The region table of the
// plan, the total size and the driver's struct of pointers all expand this list.
#define HFMI_EIG_REGIONS(X)                                                                                                     \
  X(A, D, mat)      /* the matrix; later S of the merges, then Y = V T of the back-transformation */                           \
  X(Vh, D, mat)     /* reflectors (column j = v_j with explicit zeros and the unit entry) */                                   \
  X(Q1, D, mat)     /* eigenvectors of the tridiagonal matrix, ping (Q1 and Q2 are adjacent: one fill) */                      \
  X(Q2, D, mat)     /* ... pong */                                                                                              \
  X(Qg, D, mat)     /* raw upload first, partial products of k_tri_bs, gathered columns of the merges, nothing afterwards */   \
  X(Wp, D, (size_t)ld * EB_NB)                                                                                                  \
  X(W1, D, (size_t)WY * npad)                                                                                                   \
  X(Gm, D, (size_t)nblk * WY * WY)                                                                                              \
  X(Tf, D, (size_t)nblk * WY * WY)                                                                                              \
  X(Tt, D, (size_t)nblk * WY * WY)   /* products in flight while the triangular factors are merged */                          \
  X(colbuf, D, vlen) X(ybuf, D, vlen) X(dvec, D, vlen) X(evec, D, vlen) X(tauv, D, vlen) X(D0, D, vlen) X(D1, D, vlen)          \
  X(Zv, D, vlen) X(Ds, D, vlen) X(Zs, D, vlen) X(dl, D, vlen) X(wvv, D, vlen) X(tauS, D, vlen) X(zhat, D, vlen) X(rc, D, vlen)  \
  X(rs, D, vlen) X(xd, D, vlen) X(xz, D, vlen)                                                                                  \
  X(x1, D, EB_NB) X(x2, D, EB_NB)                                                                                               \
  X(pn, D, EB_MAXN / 64)             /* one partial norm per 64 rows */                                                         \
  X(pvy, D, 2112)                    /* partial sums of v . y: <= 512 workgroups of k_tri_b, <= 2080 tiles of k_tri_bs */       \
  X(pmax, D, (size_t)(npad / 32 + 1) * (npad / 32 + 1))                                                                         \
  X(Col, I, vlen) X(Live, I, vlen) X(Ks, I, vlen) X(Src, I, vlen) X(orgv, I, vlen) X(ra, I, vlen) X(rb, I, vlen)                \
  X(order, I, vlen) X(xkp, I, vlen) X(xli, I, vlen)                                                                             \
  X(xkept, B, vlen / 2 * 4) X(xlv, B, vlen / 2 * 4)                                                                             \
  X(fail, I, 64)                     /* 16 status words (0: secular, 1: scale exponent, 2: non-finite input), 48 spare */       \
  X(nodes, N, EB_NODES)
enum eig_elem { EIG_ELEM_D = 0, EIG_ELEM_I = 1, EIG_ELEM_B = 2, EIG_ELEM_N = 3 };
constexpr int eig_elem_bytes[4] = {8, 4, 1, EB_NODE_BYTES};
constexpr int eig_elem_align[4] = {8, 4, 1, 16};
enum eig_region_id {
#define X(name, T, count) EIG_R_##name,
  HFMI_EIG_REGIONS(X)
#undef X
  EIG_NREGIONS
};
struct eig_region {
  int elem;               // eig_elem
  size_t count, offset;   // elements; bytes from the start of the workspace
  size_t bytes() const { return count * eig_elem_bytes[elem]; }
};

// ------------------------------------------------------------------ kernel instances the driver chooses between
enum eig_inst {
  EIG_K_TRI_A = 0,     // k_tri_a<false>: the last column's products were made by k_tri_b
  EIG_K_TRI_A_SLOTS,   // k_tri_a<true>: ... were left in slots by k_tri_bs
  EIG_K_TRI_B_4_8,     // k_tri_b<UNR, CB>
  EIG_K_TRI_B_8_8,
  EIG_K_TRI_B_8_16,
  EIG_K_TRI_B_8_32,
  EIG_K_TRI_BS_8,      // k_tri_bs<CB>
  EIG_K_TRI_BS_16,
  EIG_K_TRI_BS_32,
  EIG_K_TRI_U_4,       // k_tri_u<UNR>
  EIG_K_TRI_U_8,
  EIG_K_TRI_U_16,
  EIG_K_TRI_U_20,
  EIG_NINST
};
inline bool eig_inst_is_bs(int inst) { return inst >= EIG_K_TRI_BS_8 && inst <= EIG_K_TRI_BS_32; }

// ------------------------------------------------------------------ plan
struct eig_level {     // k_dcl_deflate<MODE> of merge level L (2^L nodes)
  int cap;             // the largest node of the level + 1, rounded up to 64
  int mode;            // 0: everything of a node in LDS (30 bytes per pole); 1: poles and rank-one vector (16); 2: nothing
  int lds;             // dynamic LDS bytes
  bool raise;          // hipFuncAttributeMaxDynamicSharedMemorySize is set to lds before the launch
};
struct eig_plan {
  bool blocked;        // false: n < 3 or the Jacobi route -- nothing below is filled
  int n, nvec;
  int nr;              // rows of a column that exist and are zero beyond n: n rounded up to 128
  int64_t ld;          // leading dimension: nr, or nr + 144 where nr is a power of two
  int npad, WY, nblk, npanels;
  int Lf;              // levels of merges above the 2^Lf leaves
  size_t mat, vlen;    // ld * npad; npad + 128
  eig_region region[EIG_NREGIONS];
  size_t bytes;        // of the workspace
  eig_level level[EB_MAX_LEVELS];      // [L], L < Lf
  int tri_b, tri_bs;   // the eig_inst of the full-column and of the lower-triangle products
  int tri_b_lds_attr;  // > 0: k_tri_b needs hipFuncAttributeMaxDynamicSharedMemorySize raised to this many bytes
  int sym_min, unb_max;
  bool lower_updates;
};

inline eig_plan eig_plan_make(int n, int nvec, const eig_knobs& kn, size_t lds_per_block, size_t defl1_static_lds) {
  eig_plan p;
  memset(&p, 0, sizeof(p));
  p.n = n;
  p.nvec = nvec;
  p.blocked = !((kn.jacobi && n <= 4096) || n < 3);
  if (!p.blocked) return p;
  auto round_up = [](int64_t x, int64_t m) { return (x + m - 1) / m * m; };
  // width of a block reflector of the back-transformation: V^T Z is a WY x nv product over WY / 64 row tiles -- 512 columns from
  // n = 2048 on keep 8 row tiles x nv / 128 column tiles of the pipelined kernel on the chip where 256 would leave half of it idle
  // (back-transformation at n = 2048 / 4096: 1.9 -> 1.6 / 6.5 -> 4.7 ms; profiles/r06_eig_large.txt)
  const int WY = kn.wy ? kn.wy : (n >= 2048 ? 512 : 256);
  // rows of a column: n rounded up to 128.  Leading dimension: the same, except where that is a power of two (n = 4096, 8192,
  // 16384): consecutive columns of a 128 x 128 tile or of a wave's column set then sit a power of two apart and crowd the same
  // HBM channels -- the tile pattern of the lower-triangle products read 6.25 TB/s at ld = 8192 and 6.9-7.0 at 8336 / 8720, 5.5
  // against 6.0-6.2 at n = 4096 (scripts/tile_stride_probe.hip, profiles/r06_tile_stride_probe.txt); 144 = 9 cache lines
  const int nr = (int)round_up(n, 128);
  const int64_t ld = nr + ((kn.ld_pad && nr >= 4096 && (nr & (nr - 1)) == 0) ? 144 : 0);
  const int npad = (int)round_up(n, WY), nblk = npad / WY;
  const size_t mat = (size_t)ld * npad, vlen = (size_t)npad + 128;
  p.nr = nr;
  p.ld = ld;
  p.npad = npad;
  p.WY = WY;
  p.nblk = nblk;
  p.npanels = npad / EB_NB;
  p.mat = mat;
  p.vlen = vlen;
  // ---- workspace: the regions back to back, each on its element's alignment; 256 bytes cover the alignment of the node records
  size_t off = 0, sum = 0;
  int r = 0;
#define X(name, T, cnt)                                                   \
  p.region[r].elem = EIG_ELEM_##T;                                        \
  p.region[r].count = (cnt);                                              \
  off = (size_t)round_up((int64_t)off, eig_elem_align[EIG_ELEM_##T]);     \
  p.region[r].offset = off;                                               \
  off += p.region[r].bytes();                                             \
  sum += p.region[r++].bytes();
  HFMI_EIG_REGIONS(X)
#undef X
  p.bytes = sum + 256;
  // ---- tridiagonalisation: the instances of the products.  CB / 8 partial norms per lane, one per 64 rows from j: beyond
  // n = 8192 the column below j can span 129 of them (j = n - 8193 when n is a multiple of 128), which CB = 16 would drop
  p.tri_bs = n > 8192 ? EIG_K_TRI_BS_32 : n > 4096 ? EIG_K_TRI_BS_16 : EIG_K_TRI_BS_8;
  p.tri_b = n > 8192 ? EIG_K_TRI_B_8_32 : n > 4096 ? EIG_K_TRI_B_8_16 : kn.tri_unr == 8 ? EIG_K_TRI_B_8_8 : EIG_K_TRI_B_4_8;
  // v of the first columns is 128 KB (of 160) beyond n = 8192, 64 KB beyond 4096: more than a kernel gets without asking
  p.tri_b_lds_attr = n > 4096 ? (int)(nr * sizeof(double)) : 0;
  p.sym_min = kn.sym_min;
  p.unb_max = kn.unb_max;
  p.lower_updates = kn.lower_updates;
  // ---- divide and conquer: leaves stay <= 256 rows up to EB_MAXN
  while (((n + (1 << p.Lf) - 1) >> p.Lf) > kn.leaf_max && p.Lf < EB_MAX_LEVELS) ++p.Lf;
  for (int L = 0; L < p.Lf; ++L) {
    const int nn = 1 << L;
    eig_level& lv = p.level[L];
    lv.cap = (int)round_up((n + nn - 1) / nn + 1, 64);
    // MODE 1 keeps 16 bytes per pole in dynamic LDS next to the kernel's static arrays (s_scan and three ints); together they must
    // fit what a workgroup may have on this device.  With 160 KB that ends at cap = 9920 (9984 poles: 159 744 + 4 108 bytes).
    if ((size_t)lv.cap * 16 + defl1_static_lds > lds_per_block) lv.mode = 2;      // nothing of the node in LDS
    else lv.mode = lv.cap > 4160 ? 1 : 0;                                         // 1: the top merge beyond n = 4096
    lv.lds = lv.mode == 2 ? 0 : lv.cap * (lv.mode == 1 ? 16 : 30);
    lv.raise = lv.mode != 2;
  }
  return p;
}

// ------------------------------------------------------------------ the tridiagonalisation walk
struct eig_tri_col {       // a panel column: k_tri_a (finalise column j - 1 of W, form column j), then the products of column j
  int p0, j, jj;
  int ga;                  // workgroups of k_tri_a = partial norms it leaves (npn)
  bool prev_slots;         // the last column's products were left in slots by k_tri_bs: k_tri_a<true>
  int inst;                // eig_inst of the products
  int grid, lds;           // of the products; lds = dynamic bytes
  int nb, ntiles;          // k_tri_bs only: 128-row blocks of the trailing matrix and its lower-triangle tiles
  int npvy;                // partial sums of v . y the products leave
};
struct eig_tri_end {       // a panel end: k_tri_a finalises the last column, then A[t0:, t0:] -= V W^T + W V^T
  int p0, t0, ncols;
  bool prev_slots;
  int lower;               // gemm_desc::lower of the update: 0 = the full block
};
struct eig_tri_ucol {      // a column of the unblocked tail: one k_tri_u
  int j, inst, grid, lds;
  int has_prev;            // 0 on the first column of the tail (j = j_unb): no reflector is pending
  int ybuf;                // which of the two y buffers holds y of the last step (the other takes this step's)
};
// Calls v.column / v.panel_end / v.mirror / v.tail_column / v.tail in launch order; each returns 0 or an error, which ends the walk.
template <class V>
int eig_tri_walk(const eig_plan& p, V&& v) {
  const int n = p.n, nr = p.nr;
  auto min_i = [](int a, int b) { return a < b ? a : b; };
  auto max_i = [](int a, int b) { return a > b ? a : b; };
  // the lower-triangle products serve trailing blocks of sym_min ... 8192 rows (64 slots of 128 rows, 2080 tiles); the first columns of a
  // larger matrix take the full-column products
  auto uses_bs = [&](int j) { return n - j - 1 >= p.sym_min && (nr - ((j + 1) & ~(EB_TS - 1))) / EB_TS <= 64; };
  bool prev_slots = false;      // the last column's products were left in slots by k_tri_bs
  bool upper_valid = true;      // the upper triangle of the trailing block is up to date
  int j_unb = -1;               // first column of the unblocked tail
  int s = 0;
  auto make_upper_valid = [&](int t0) {
    if (upper_valid) return 0;
    upper_valid = true;
    return v.mirror(t0);
  };
  for (int p0 = 0; p0 < n - 2; p0 += EB_NB) {
    if (n - p0 <= p.unb_max) {
      j_unb = p0;
      if ((s = make_upper_valid(p0))) return s;
      break;
    }
    const int ncols = min_i(EB_NB, n - 2 - p0);
    for (int jj = 0; jj < ncols; ++jj) {
      eig_tri_col c;
      c.p0 = p0;
      c.j = p0 + jj;
      c.jj = jj;
      c.ga = (n - c.j + 63) / 64;
      c.prev_slots = prev_slots;
      if (uses_bs(c.j)) {
        // large trailing block: the lower triangle only (k_tri_bs); the next k_tri_a adds the partial vectors
        const int rs2 = (c.j + 1) & ~(EB_TS - 1);
        c.inst = p.tri_bs;
        c.nb = (nr - rs2) / EB_TS;
        c.ntiles = c.nb * (c.nb + 1) / 2;
        c.grid = c.ntiles + 2 * jj;
        c.lds = 0;
        c.npvy = c.ntiles;
      } else {
        const int nc = (n - c.j - 1) + 2 * jj, rs0 = (c.j + 1) & ~63;
        c.inst = p.tri_b;
        c.nb = c.ntiles = 0;
        c.grid = max_i(1, min_i(512, (nc + 7) / 8));
        c.lds = (int)((size_t)(nr - rs0) * sizeof(double));      // v on rows [rs0, nr)
        c.npvy = c.grid;
      }
      if ((s = v.column(c))) return s;
      prev_slots = eig_inst_is_bs(c.inst);
    }
    const int t0 = p0 + ncols;
    // every column of the NEXT panel takes the lower-triangle products (and there is a next panel): the tiles above the diagonal are
    // not read again until the full-column / unblocked columns begin -- they are skipped and mirrored back once, there
    const bool next_all_lower = uses_bs(t0) && uses_bs(t0 + EB_NB - 1) && n - t0 > p.unb_max;
    eig_tri_end e;
    e.p0 = p0;
    e.t0 = t0;
    e.ncols = ncols;
    e.prev_slots = prev_slots;
    e.lower = (p.lower_updates && (next_all_lower || !upper_valid)) ? 1 + (t0 & 127) : 0;
    if ((s = v.panel_end(e))) return s;
    if (e.lower) upper_valid = false;
    if (!next_all_lower && (s = make_upper_valid(t0))) return s;
  }
  if ((s = make_upper_valid(0))) return s;
  if (j_unb < 0) return v.tail();      // the last 2 x 2 block: k_tri_tail
  // the matrix is fully updated at a panel boundary: nothing is pending at column j_unb.  Steps j_unb .. n - 1: step j applies
  // reflector j - 1 and forms reflector j; the last two steps only collect d and e of the final 2 x 2 block.
  for (int j = j_unb; j < n; ++j) {
    const int rs0 = j & ~63, L = nr - rs0, nA = n - j - 1;
    eig_tri_ucol u;
    u.j = j;
    u.inst = L <= 512 ? EIG_K_TRI_U_4 : L <= 1024 ? EIG_K_TRI_U_8 : L <= 2048 ? EIG_K_TRI_U_16 : EIG_K_TRI_U_20;
    u.grid = max_i(1, min_i(512, (nA + 7) / 8));
    u.lds = (int)((size_t)3 * L * sizeof(double));
    u.has_prev = j > j_unb ? 1 : 0;
    u.ybuf = (j - j_unb) & 1;
    if ((s = v.tail_column(u))) return s;
  }
  return 0;
}

// the predictor's visitor: counts what the driver's visitor would launch
struct eig_walk_summary {
  int64_t launches[EIG_NINST] = {};     // per instance
  int64_t max_npn[EIG_NINST] = {};      // k_tri_b / k_tri_bs: most partial norms an instance is handed
  int64_t max_npvy[EIG_NINST] = {};     // k_tri_a: most partial sums of v . y an instance is handed
  int64_t max_lds[EIG_NINST] = {};      // most dynamic LDS bytes
  int64_t max_ntiles = 0, max_npvy_all = 0, max_nb = 0, max_ga = 0;
  int64_t panel_cols = 0, panel_ends = 0, mirrors = 0, lower_updates = 0, tails = 0, j_unb = -1;
  int npvy = 0;                         // left by the last products
  static void up(int64_t& m, int64_t v) { if (v > m) m = v; }
  void tri_a(bool slots) {
    const int a = slots ? EIG_K_TRI_A_SLOTS : EIG_K_TRI_A;
    ++launches[a];
    up(max_npvy[a], npvy);
  }
  int column(const eig_tri_col& c) {
    tri_a(c.prev_slots);
    ++panel_cols;
    ++launches[c.inst];
    up(max_npn[c.inst], c.ga);
    up(max_lds[c.inst], c.lds);
    up(max_ga, c.ga);
    up(max_ntiles, c.ntiles);
    up(max_nb, c.nb);
    up(max_npvy_all, c.npvy);
    npvy = c.npvy;
    return 0;
  }
  int panel_end(const eig_tri_end& e) {
    tri_a(e.prev_slots);
    ++panel_ends;
    if (e.lower) ++lower_updates;
    return 0;
  }
  int mirror(int) { return ++mirrors, 0; }
  int tail_column(const eig_tri_ucol& u) {
    if (!u.has_prev) j_unb = u.j;
    ++launches[u.inst];
    up(max_lds[u.inst], u.lds);
    return 0;
  }
  int tail() { return ++tails, 0; }
};
