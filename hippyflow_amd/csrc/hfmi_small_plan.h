// Launch plans of the one-compute-unit k x k stage (k <= 256): the column-at-a-time Cholesky (hfmi_chol_col.hip) and the blocked MFMA
// Cholesky (hfmi_chol.hip), the Jacobi eigensolver and SVD (hfmi_jacobi.hip), the divide-and-conquer eigensolver (hfmi_eig_dc.hip) and
// the blocked LU (hfmi_lu.hip).  Host only, plain C++17, nothing from HIP: given k and the knobs a planner fills a plain struct with
// every launch of the call (kernel family, template parameters, threads, grid, dynamic LDS and whether the attribute is raised) and
// the WS_MISC workspace as one list of regions; the launchers check their arguments, plan, allocate and carve by the plan, look the
// kernel pointer up in a switch expanded from the table below, and launch.  hfmi_small_plan_predict (include/hfmi.h) writes the same
// structs out without a device; tests/test_small_plan_cpu.py holds them to the if-chains they replace
// (tests/helpers/small_plan_twin.py) and to what each kernel's indexing needs to stay in bounds.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

constexpr int SMALL_MAXK = 256;            // SM_MAXK of hfmi_internal.h
constexpr int SMALL_THREADS = 1024;        // workgroup of the one-workgroup kernels unless HFMI_SMALL_THREADS says otherwise
constexpr int SMALL_LDS_BYTES = 163840;    // LDS of a workgroup on gfx950
constexpr int CHOL_REG_THREADS = 512;      // k_chol_reg, k_chol_tile<TR, TC>
constexpr int CM_SCR = 4 * 16 * 17;        // k_chol_mfma: padded 16 x 16 blocks of scratch per wave: input / R_KK, Z_KK, two dump blocks
constexpr int JAC_MAX_SWEEPS = 40;
constexpr int DC_THREADS = 1024;
constexpr int DC_WAVES = 16;
constexpr int DC_MAXN = 256;
constexpr int LU_THREADS = 1024;
constexpr int LU_BOOK_BYTES = (64 + 64 + 256 + 128) * 8;   // wave partials (|v|, v, index), 1 / pivot, pivot rows
constexpr int LU_LDS_BYTES = SMALL_LDS_BYTES;

// ------------------------------------------------------------------ knobs
// The ten environment switches and the two tuning keys of the stage, one instance per process, the environment read once when the
// instance is first used.  "chol" and "eig" of hfmi_tuning_set and their environment values HFMI_CHOL / HFMI_EIG resolve here:
// the environment value counts only while the key was never set (small_use_column_chol, small_use_jacobi).
struct small_knobs {
  int small_threads;       // HFMI_SMALL_THREADS: workgroup of k_chol_inv, k_jacobi_*; 64 .. 1024 in multiples of 64, anything else 1024
  int chol_env;            // HFMI_CHOL=tile: 1 = the column-at-a-time kernels, anything else 0 = the blocked MFMA kernel
  int chol_generic;        // HFMI_CHOL_GENERIC (A/B): the generic one-kernel path k_chol_inv
  int chol_tile;           // HFMI_CHOL_TILE=0 (A/B): the cyclic ownership map k_chol_reg instead of k_chol_tile; default 1
  int jacobi_db;           // HFMI_JACOBI_DB (A/B): 0 never k_jacobi_eig_db, 1 where it wins (>= 3 blocks per thread), 2 whenever it fits
  int jacobi_replay_lds;   // HFMI_JACOBI_REPLAY_LDS (A/B): the LDS + barrier replay k_jacobi_vectors at every size
  int eig_env;             // HFMI_EIG=jacobi: 1 = Jacobi for every small eigensolve, anything else 0 = divide and conquer
  int tri_waves;           // HFMI_TRI_WAVES = 4 | 8 (A/B): workgroup shape of k_tridiag; anything but 4 means 8
  int dc_split_top;        // HFMI_DC_SPLIT_TOP=0 (A/B): the last merge's product inside k_dc; default 1
  int dc_timing;           // HFMI_DC_TIMING: section ticks of k_tridiag / k_dc on stderr (a stream synchronisation per call)
  int chol_key;            // tuning key "chol": -1 never set, else 0 | 1
  int eig_key;             // tuning key "eig": -1 never set, else 0 | 1
};
constexpr int SMALL_KNOB_WORDS = 12;       // the fields above, in this order
// on when set to anything but "" or "0" (env_flag of hfmi_internal.h)
inline int small_env_flag(const char* name) {
  const char* e = getenv(name);
  return (e && e[0] && !(e[0] == '0' && e[1] == 0)) ? 1 : 0;
}
inline small_knobs& small_knobs_ref() {
  static small_knobs kn = [] {
    auto is = [](const char* name, const char* word) {
      const char* e = getenv(name);
      return (e && !strcmp(e, word)) ? 1 : 0;
    };
    auto num = [](const char* name, int unset) {
      const char* e = getenv(name);
      return e ? atoi(e) : unset;
    };
    small_knobs k;
    const int t = num("HFMI_SMALL_THREADS", SMALL_THREADS);
    k.small_threads = (t < 64 || t > 1024 || (t & 63)) ? SMALL_THREADS : t;
    k.chol_env = is("HFMI_CHOL", "tile");
    k.chol_generic = small_env_flag("HFMI_CHOL_GENERIC");
    k.chol_tile = num("HFMI_CHOL_TILE", 1) == 0 ? 0 : 1;
    k.jacobi_db = num("HFMI_JACOBI_DB", 1);
    k.jacobi_replay_lds = small_env_flag("HFMI_JACOBI_REPLAY_LDS");
    k.eig_env = is("HFMI_EIG", "jacobi");
    k.tri_waves = num("HFMI_TRI_WAVES", 8) == 4 ? 4 : 8;
    k.dc_split_top = num("HFMI_DC_SPLIT_TOP", 1);
    k.dc_timing = small_env_flag("HFMI_DC_TIMING");
    k.chol_key = k.eig_key = -1;
    return k;
  }();
  return kn;
}
// the stage's keys of hfmi_tuning_set: true = key known and value accepted
inline bool small_knob_set(const char* key, int v) {
  if (v != 0 && v != 1) return false;
  small_knobs& kn = small_knobs_ref();
  if (!strcmp(key, "chol")) return kn.chol_key = v, true;     // 0 = blocked MFMA kernel (default), 1 = column-at-a-time kernels
  if (!strcmp(key, "eig")) return kn.eig_key = v, true;       // 0 = divide and conquer (default), 1 = Jacobi
  return false;
}
inline bool small_use_column_chol(const small_knobs& kn) { return (kn.chol_key >= 0 ? kn.chol_key : kn.chol_env) == 1; }
inline bool small_use_jacobi(const small_knobs& kn) { return (kn.eig_key >= 0 ? kn.eig_key : kn.eig_env) == 1; }
// Rayleigh-Ritz eigensolver selection: 1 = Jacobi, 0 = divide and conquer.  method 1 is the caller's wish for the high RELATIVE
// accuracy of small eigenvalues of graded positive definite matrices (hfmi_sym_eig_small flag bit 1, hfmi_double_pass flag bit 3)
inline int sym_eig_route(int method, const small_knobs& kn) { return (method == 1 || small_use_jacobi(kn)) ? 1 : 0; }

// ------------------------------------------------------------------ instance tables
// Stated once: the dispatch switch of the unit that owns the kernel expands a list into kernel pointers, the planner into the
// ladder.  Every ladder takes the FIRST entry whose bound holds; the last entry of a list also takes whatever is left (the Jacobi blocks
// per thread excepted: there nothing left over is launched).
// k_chol_reg<E>: triangle entries per thread (512 threads), bound: ceil(k (k + 1) / 2 / 512) <= E
#define HFMI_CHOL_REG_CASES(X) X(1) X(2) X(4) X(6) X(8) X(12) X(16) X(20)
// k_chol_tile<TR, TC> at 512 threads: the smallest rectangle whose tiles fit the threads, bound: chol_tiles(k, TR, TC) <= 512
#define HFMI_CHOL_TILE_CASES(X) X(1, 2) X(2, 2) X(2, 3) X(3, 3) X(3, 4) X(4, 4) X(4, 5) X(5, 5)
// k_chol_tile<TR, TC, 1024, true> (140 <= k <= 256, the factor's copy in a global slot), bound: chol_tiles(k, TR, TC) <= 1024
#define HFMI_CHOL_BIG_CASES(X) X(4, 4) X(4, 5) X(5, 5) X(5, 6) X(6, 6)
// k_chol_mfma<NW, SLOTS>: X(NW, SLOTS, largest nb = ceil(k / 16)); nb (nb + 1) / 2 block slots over the waves: 15, 28, 45, 78, 136
// (sixteen waves would have 128 registers each: not enough)
#define HFMI_CHOL_MFMA_CASES(X) X(8, 2, 5) X(8, 4, 7) X(8, 6, 9) X(8, 10, 12) X(8, 17, 16)
// k_jacobi_eig<NB, LDS>, both LDS values of every NB: 2 x 2 blocks per thread of the update phase, bound: ceil(cells / threads) <= NB
#define HFMI_JACOBI_NB_CASES(X) X(1) X(2) X(3) X(9)
// k_jacobi_eig_db<NB>, bound: ceil(cells / (threads - 128)) <= NB
#define HFMI_JACOBI_DB_CASES(X) X(1) X(2) X(3)
// k_tridiag<RI, CJ, NW>: X(largest k, RI, CJ), four waves (HFMI_TRI_WAVES=4) and eight (default; k <= 160)
#define HFMI_TRI_W4_CASES(X) X(32, 8, 1) X(64, 16, 1) X(80, 20, 2) X(96, 24, 2) X(128, 32, 2) X(144, 36, 3) X(160, 40, 3) X(192, 48, 3) X(256, 64, 4)
#define HFMI_TRI_W8_CASES(X) X(32, 4, 1) X(64, 8, 1) X(96, 12, 2) X(128, 16, 2) X(160, 20, 3)
// k_tridiag<RI, CJ, 8, LR>: X(largest k, RI, CJ, LR).  160 < k <= 256 with eight waves: 64 k^2 doubles leave no registers for
// anything else (the compiler spills 84..99 values per thread and the reduction runs 3x slower), so the last LR rows live in LDS;
// these shapes do not spill (k <= 192) or spill 5 values (k <= 224); above that 64 rows are all the LDS holds beside the work arrays
#define HFMI_TRI_LDS_CASES(X) X(192, 20, 3, 32) X(224, 20, 4, 64) X(256, 24, 4, 64)
// k_dc<G> and k_dc_batch<G>: X(largest n, G)
#define HFMI_DC_CASES(X) X(128, 8) X(256, 4)
// k_dc_back<EL>: X(largest k, EL)
#define HFMI_DC_BACK_CASES(X) X(80, 5) X(96, 6) X(128, 8) X(144, 9) X(192, 12) X(256, 16)

// G of k_dc<G> / k_dc_batch<G> for problems (leaves) of at most n rows
inline int dc_group(int n) {
#define X(KMAX, G) \
  if (n <= KMAX) return G;
  HFMI_DC_CASES(X)
#undef X
  return 0;
}
// tiles of TR x TC that touch the upper triangle of a k x k matrix: one thread of k_chol_tile each
inline int chol_tiles(int k, int trr, int tcc) {
  const int ntr = (k + trr - 1) / trr, ntc = (k + tcc - 1) / tcc;
  int n = 0;
  for (int I = 0; I < ntr; ++I)
    for (int J = 0; J < ntc; ++J)
      if (J * tcc + tcc - 1 >= I * trr) ++n;
  return n;
}
// panel width of k_lu_solve's blocked form: the whole matrix (one panel, no trailing update) while m x (m|1) doubles fit the LDS
// next to the bookkeeping (m <= 141), otherwise the widest multiple of 16 that fits (m = 256: 64)
inline int lu_panel_width(int m) {
  const int avail = (LU_LDS_BYTES - LU_BOOK_BYTES - 64) / 8;   // 64 bytes for the kernel's static flag
  if (m * (m | 1) <= avail) return m;
  return ((avail / m) - 1) & ~15;
}

// ------------------------------------------------------------------ workspace
// The regions of WS_MISC, in the order they are laid out, back to back (every element size divides the offset it lands on):
// X(name, element bytes, count).  The counts are written in the locals of the planners.  The plan's region table, the total size
// and the launchers' struct of pointers all expand these lists.
// launch_dc_eig: d, e, tau, reflectors (256 x ldq), Q, Qt, S, the output permutation, the scale exponent, section ticks and what
// k_dc leaves for k_dc_top
#define HFMI_DC_REGIONS(X)                                                                                              \
  X(dvec, 8, DC_MAXN) X(evec, 8, DC_MAXN) X(tauv, 8, DC_MAXN) X(Vh, 8, (size_t)DC_MAXN * ldq) X(Qm, 8, mat) X(Qt, 8, mat) \
  X(Sm, 8, mat) X(perm, 4, DC_MAXN) X(sexp, 4, 16) X(ticks, 8, 16) X(top_meta, 4, 3 * DC_MAXN + 16)
// launch_jacobi_eig / launch_jacobi_svd: one (c, s) pair per pivot of every round, then the output permutation
#define HFMI_JACOBI_REGIONS(X) X(rotlog, 16, (size_t)rounds*(n / 2)) X(perm, 4, 1024)
constexpr int SMALL_MAX_REGIONS = 12;
struct small_region {
  int64_t offset, bytes;
};
#define HFMI_REGION_MEMBER(name, eb, cnt) char* name;
struct dc_ws { HFMI_DC_REGIONS(HFMI_REGION_MEMBER) };
struct jacobi_ws { HFMI_JACOBI_REGIONS(HFMI_REGION_MEMBER) };
#undef HFMI_REGION_MEMBER

// ------------------------------------------------------------------ plan
enum small_kind { SMALL_KIND_CHOL = 0, SMALL_KIND_EIGH = 1, SMALL_KIND_SVD = 2, SMALL_KIND_LU = 3 };
enum small_family {
  SF_NONE = 0,
  SF_CHOL_MFMA,             // k_chol_mfma<t0 = NW, t1 = SLOTS>
  SF_CHOL_REG,              // k_chol_reg<t0 = E>
  SF_CHOL_TILE,             // k_chol_tile<t0 = TR, t1 = TC>
  SF_CHOL_BIG,              // k_chol_tile<t0 = TR, t1 = TC, 1024, true>
  SF_CHOL_INV,              // k_chol_inv
  SF_JACOBI_EIG,            // k_jacobi_eig<t0 = NB, t1 = LDS>
  SF_JACOBI_EIG_DB,         // k_jacobi_eig_db<t0 = NB>
  SF_JACOBI_SVD,            // k_jacobi_svd<t0 = LDS>
  SF_JACOBI_VECTORS,        // k_jacobi_vectors: one workgroup per row, LDS + barriers
  SF_JACOBI_VECTORS_WAVE,   // k_jacobi_vectors_wave: one wave per row, four rows per workgroup
  SF_TRIDIAG,               // k_tridiag<t0 = RI, t1 = CJ, t2 = NW, t3 = LR>
  SF_DC,                    // k_dc<t0 = G>
  SF_DC_TOP,                // k_dc_top
  SF_DC_BACK,               // k_dc_back<t0 = EL>
  SF_LU                     // k_lu_solve
};
enum small_refusal {
  SMALL_OK = 0,
  SMALL_REFUSE_RANGE,       // k outside 1 .. 256
  SMALL_REFUSE_INSTANCE     // Jacobi: more 2 x 2 blocks per thread (nb) than any instance holds (a small HFMI_SMALL_THREADS)
};
struct small_launch {
  int family;               // small_family
  int t[4];                 // template parameters, by family
  int threads, grid;
  int64_t lds;              // dynamic LDS bytes
  int raise;                // hipFuncAttributeMaxDynamicSharedMemorySize is set to lds before the launch
};
constexpr int SMALL_MAX_LAUNCHES = 4;
struct small_plan {
  int refuse;               // small_refusal; nothing is launched unless SMALL_OK
  int nlaunch;
  small_launch launch[SMALL_MAX_LAUNCHES];     // in launch order
  int64_t ws_bytes;         // of WS_MISC (0: none)
  int nregions;
  small_region region[SMALL_MAX_REGIONS];
  int route;                // Cholesky: 1 = column-at-a-time, 0 = blocked MFMA; eigh: 1 = Jacobi, 0 = divide and conquer
  int use_lds;              // the working matrix is in LDS (column Cholesky, Jacobi, SVD)
  int n;                    // Jacobi, SVD: k rounded up to even
  int nb;                   // Jacobi: 2 x 2 blocks per thread; LU: panel width; blocked Cholesky: 16-row blocks
  int ldq, levels;          // divide and conquer: leading dimension of Q, Qt, S, Vh; tree levels
  int split_top;            // ... the last merge's product is k_dc_top's
  int top_from_qt;          // ... k_dc_top reads Qt and writes Qm (else the other way round)
  int fin_in_qt;            // ... the eigenvectors of the tridiagonal matrix end in Qt (else Qm)
  int timing;               // ... section ticks on stderr
};
inline small_plan small_plan_empty() {
  small_plan p;
  memset(&p, 0, sizeof(p));
  return p;
}
inline small_plan small_plan_refused(int why) {
  small_plan p = small_plan_empty();
  p.refuse = why;
  return p;
}
inline small_launch& small_add_launch(small_plan& p, int family, int threads, int grid, int64_t lds, bool raise) {
  small_launch& L = p.launch[p.nlaunch++];
  L.family = family;
  L.threads = threads;
  L.grid = grid;
  L.lds = lds;
  L.raise = raise ? 1 : 0;
  return L;
}
#define HFMI_REGION_PLAN(name, eb, cnt)                     \
  p.region[p.nregions].offset = p.ws_bytes;                 \
  p.region[p.nregions].bytes = (int64_t)(eb) * (int64_t)(cnt); \
  p.ws_bytes += p.region[p.nregions++].bytes;
// the launchers' half: a struct of pointers into the allocation, one per region
#define HFMI_REGION_CARVE(name, eb, cnt) w.name = base + p.region[r++].offset;
inline dc_ws dc_ws_carve(const small_plan& p, void* ws) {
  dc_ws w;
  char* base = (char*)ws;
  int r = 0;
  HFMI_DC_REGIONS(HFMI_REGION_CARVE)
  return w;
}
inline jacobi_ws jacobi_ws_carve(const small_plan& p, void* ws) {
  jacobi_ws w;
  char* base = (char*)ws;
  int r = 0;
  HFMI_JACOBI_REGIONS(HFMI_REGION_CARVE)
  return w;
}
#undef HFMI_REGION_CARVE

// ------------------------------------------------------------------ planners
// the blocked MFMA kernel (hfmi_chol.hip): one workgroup of 64 NW threads
inline small_plan chol_mfma_plan(int k) {
  if (k < 1 || k > SMALL_MAXK) return small_plan_refused(SMALL_REFUSE_RANGE);
  small_plan p = small_plan_empty();
  const int nb = p.nb = (k + 15) / 16;
  int nw = 0, slots = 0;
  bool hit = false;
#define X(NW, SLOTS, NBMAX) \
  if (!hit) nw = NW, slots = SLOTS, hit = nb <= NBMAX;
  HFMI_CHOL_MFMA_CASES(X)
#undef X
  small_launch& L = small_add_launch(p, SF_CHOL_MFMA, 64 * nw, 1, (int64_t)(32 + 5 * 256 + nw * CM_SCR + 2 * nb * 256) * 8, true);
  L.t[0] = nw;
  L.t[1] = slots;
  return p;
}
// launch_chol_inv.  Default: the blocked MFMA kernel; the column-at-a-time kernels stay for A/B runs (HFMI_CHOL=tile, tuning
// "chol" = 1) and as the reference the tests compare the blocked kernel with
inline small_plan chol_plan(int k, const small_knobs& kn) {
  if (k < 1 || k > SMALL_MAXK) return small_plan_refused(SMALL_REFUSE_RANGE);
  if (!small_use_column_chol(kn)) return chol_mfma_plan(k);
  small_plan p = small_plan_empty();
  p.route = 1;
  p.use_lds = (k <= 139) ? 1 : 0;   // (32 + 4 * 256) * 8 + 139 * 139 * 8 = 163,016 bytes <= 160 KB (163,840)
  const int64_t matrix = (int64_t)k * (k | 1) * 8;
  if (kn.chol_generic) {
    // the generic path: any k, the matrix in LDS when it fits, else in the global slot SM_TMP
    small_add_launch(p, SF_CHOL_INV, kn.small_threads, 1, (32 + 3 * 256) * 8 + (p.use_lds ? matrix : 0), true);
  } else if (p.use_lds) {
    const int64_t lds = (32 + 4 * 256) * 8 + matrix;
    int a = 0, b = 0;
    bool hit = false;
    if (kn.chol_tile && k >= 8) {
#define X(TR, TC) \
  if (!hit) a = TR, b = TC, hit = chol_tiles(k, TR, TC) <= CHOL_REG_THREADS;
      HFMI_CHOL_TILE_CASES(X)
#undef X
      small_launch& L = small_add_launch(p, SF_CHOL_TILE, CHOL_REG_THREADS, 1, lds, true);
      L.t[0] = a;
      L.t[1] = b;
    } else {
      const int ept = (k * (k + 1) / 2 + CHOL_REG_THREADS - 1) / CHOL_REG_THREADS;   // <= 19 for k <= 139
#define X(E) \
  if (!hit) a = E, hit = ept <= E;
      HFMI_CHOL_REG_CASES(X)
#undef X
      small_add_launch(p, SF_CHOL_REG, CHOL_REG_THREADS, 1, lds, true).t[0] = a;
    }
  } else {
    // 140 <= k <= 256: tiles in the registers of 1024 threads, the factor's copy in the global slot SM_TMP
    int a = 0, b = 0;
    bool hit = false;
#define X(TR, TC) \
  if (!hit) a = TR, b = TC, hit = chol_tiles(k, TR, TC) <= 1024;
    HFMI_CHOL_BIG_CASES(X)
#undef X
    small_launch& L = small_add_launch(p, SF_CHOL_BIG, 1024, 1, (32 + 4 * 256) * 8, false);
    L.t[0] = a;
    L.t[1] = b;
  }
  return p;
}

// the rotation log and the permutation of the Jacobi kernels: `rounds` rounds of n / 2 pivots
inline void jacobi_regions(small_plan& p, int n, size_t rounds) {
  HFMI_JACOBI_REGIONS(HFMI_REGION_PLAN)
}
inline small_plan jacobi_eig_plan(int k, const small_knobs& kn) {
  if (k < 1 || k > SMALL_MAXK) return small_plan_refused(SMALL_REFUSE_RANGE);
  small_plan p = small_plan_empty();
  p.route = 1;
  const int n = p.n = (k + 1) & ~1, np = n / 2;
  p.use_lds = (n <= 138) ? 1 : 0;   // 138*138*8 + 6.4 KB of tables = 158.8 KB <= 160 KB
  const int threads = kn.small_threads;
  const int cells = ((np + 1) >> 1) * (np + 1);
  const int nb = p.nb = (cells + threads - 1) / threads;
  const int nblk = np * (np + 1) / 2;
  const int64_t lds_db = (32 + 512 + 256) * 8 + (int64_t)8 * nblk * 8;
  const int nb_db = threads > 128 ? (cells + (threads - 128) - 1) / (threads - 128) : 99;
  // measured (scripts/jacobi_ab.py, kernel traces): k = 138 1.21 vs 1.38 ms, but k = 74 0.41 vs 0.35 and k = 84 0.46 vs
  // 0.44 ms -- with one block per thread the look-ahead chain is longer than the three short phases it replaces
  const int db_min_blocks = (kn.jacobi_db == 2) ? 1 : 3;
  int inst = 0;
  bool hit = false;
  if (kn.jacobi_db && nb >= db_min_blocks && n <= 138 && np <= 128 && threads >= 256 && nb_db <= 3 && lds_db <= 160 * 1024) {
#define X(NB) \
  if (!hit) inst = NB, hit = nb_db <= NB;
    HFMI_JACOBI_DB_CASES(X)
#undef X
    small_add_launch(p, SF_JACOBI_EIG_DB, threads, 1, lds_db, true).t[0] = inst;
  } else {
#define X(NB) \
  if (!hit) inst = NB, hit = nb <= NB;
    HFMI_JACOBI_NB_CASES(X)
#undef X
    if (!hit) {   // the one ladder whose last entry does not take what is left
      p.refuse = SMALL_REFUSE_INSTANCE;
      return p;
    }
    small_launch& L = small_add_launch(p, SF_JACOBI_EIG, threads, 1, (32 + 256 + 256) * 8 + (p.use_lds ? (int64_t)n * n * 8 : 0), true);
    L.t[0] = inst;
    L.t[1] = p.use_lds;
  }
  // the rotations are replayed on the identity: one wave per row while a row's registers hold it (n <= 128)
  if (n <= 128 && !kn.jacobi_replay_lds) small_add_launch(p, SF_JACOBI_VECTORS_WAVE, 256, (k + 3) / 4, 0, false);
  else small_add_launch(p, SF_JACOBI_VECTORS, 128, k, 0, false);
  jacobi_regions(p, n, (size_t)JAC_MAX_SWEEPS * (n - 1));
  return p;
}
inline small_plan jacobi_svd_plan(int k, const small_knobs& kn) {
  if (k < 1 || k > SMALL_MAXK) return small_plan_refused(SMALL_REFUSE_RANGE);
  small_plan p = small_plan_empty();
  const int n = p.n = (k + 1) & ~1;
  p.use_lds = (k <= 139) ? 1 : 0;   // 139*139*8 + 3.4 KB of tables <= 160 KB
  small_add_launch(p, SF_JACOBI_SVD, kn.small_threads, 1, (32 + 256 + 132) * 8 + (p.use_lds ? (int64_t)k * (k | 1) * 8 : 0), true).t[0] = p.use_lds;
  small_add_launch(p, SF_JACOBI_VECTORS, 128, k, 0, false);
  jacobi_regions(p, n, (size_t)(JAC_MAX_SWEEPS + 1) * (n - 1));
  return p;
}

// launch_dc_eig: k_tridiag, k_dc, k_dc_top unless the last merge stays inside k_dc, k_dc_back
inline small_plan dc_eig_plan(int k, const small_knobs& kn) {
  if (k < 1 || k > SMALL_MAXK) return small_plan_refused(SMALL_REFUSE_RANGE);
  small_plan p = small_plan_empty();
  const int ldq = p.ldq = (k + 15) / 16 * 16;
  const size_t mat = (size_t)ldq * ldq;
  HFMI_DC_REGIONS(HFMI_REGION_PLAN)
  int ri = 0, cj = 0, lr = 0;
  bool hit = false;
  if (kn.tri_waves == 4) {
#define X(KMAX, RI, CJ) \
  if (!hit) ri = RI, cj = CJ, hit = k <= KMAX;
    HFMI_TRI_W4_CASES(X)
  } else {
    HFMI_TRI_W8_CASES(X)
#undef X
#define X(KMAX, RI, CJ, LR) \
  if (!hit) ri = RI, cj = CJ, lr = LR, hit = k <= KMAX;
    HFMI_TRI_LDS_CASES(X)
#undef X
  }
  small_launch& tri = small_add_launch(p, SF_TRIDIAG, 64 * kn.tri_waves, 1, (int64_t)lr * 64 * cj * 8, lr > 0);
  tri.t[0] = ri;
  tri.t[1] = cj;
  tri.t[2] = kn.tri_waves;
  tri.t[3] = lr;
  while ((1 << p.levels) < k) ++p.levels;
  small_add_launch(p, SF_DC, DC_THREADS, 1, 0, false).t[0] = dc_group(k);
  p.split_top = (kn.dc_split_top && k >= 32) ? 1 : 0;
  if (p.split_top) {
    // level 0 is the last of the ping-pong merges (levels - 1 of them: the deepest level works in place): its input is the
    // buffer after levels - 2 swaps
    const int before = p.levels >= 2 ? p.levels - 2 : 0, T = (k + 15) / 16;
    p.top_from_qt = before & 1;
    small_add_launch(p, SF_DC_TOP, 64, T * T + 16, 0, false);
  }
  const int swaps = p.levels >= 1 ? p.levels - 1 : 0;   // the deepest level is solved in place (2 x 2 blocks in closed form)
  p.fin_in_qt = swaps & 1;                              // the other merges ping-pong between the two buffers
  int el = 0;
  hit = false;
#define X(KMAX, EL) \
  if (!hit) el = EL, hit = k <= KMAX;
  HFMI_DC_BACK_CASES(X)
#undef X
  small_add_launch(p, SF_DC_BACK, 64, (k + 3) / 4, 0, false).t[0] = el;
  p.timing = kn.dc_timing;
  return p;
}

inline small_plan lu_plan(int m) {
  if (m < 1 || m > SMALL_MAXK) return small_plan_refused(SMALL_REFUSE_RANGE);
  small_plan p = small_plan_empty();
  p.nb = lu_panel_width(m);
  small_add_launch(p, SF_LU, LU_THREADS, 1, LU_BOOK_BYTES + (int64_t)m * (p.nb | 1) * 8, true);
  return p;
}
#undef HFMI_REGION_PLAN

// ------------------------------------------------------------------ hfmi_small_plan_predict's record
constexpr int SMALL_PLAN_WORDS = 12 + 9 * SMALL_MAX_LAUNCHES + 2 * SMALL_MAX_REGIONS + SMALL_KNOB_WORDS;
inline void small_knob_words(const small_knobs& kn, int* w) {
  const int v[SMALL_KNOB_WORDS] = {kn.small_threads, kn.chol_env, kn.chol_generic, kn.chol_tile, kn.jacobi_db, kn.jacobi_replay_lds,
                                   kn.eig_env,       kn.tri_waves, kn.dc_split_top, kn.dc_timing, kn.chol_key,  kn.eig_key};
  memcpy(w, v, sizeof(v));
}
inline small_knobs small_knobs_from_words(const int* w) {
  return small_knobs{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11]};
}
inline void small_plan_words(const small_plan& p, const small_knobs& kn, int64_t* w) {
  memset(w, 0, sizeof(int64_t) * SMALL_PLAN_WORDS);
  const int64_t head[12] = {p.refuse, p.nlaunch, p.ws_bytes, p.nregions, p.route, p.use_lds, p.n, p.nb, p.ldq, p.levels, p.split_top,
                            p.top_from_qt | (p.fin_in_qt << 1) | (p.timing << 2)};
  memcpy(w, head, sizeof(head));
  w += 12;
  for (int i = 0; i < p.nlaunch; ++i) {
    const small_launch& L = p.launch[i];
    const int64_t v[9] = {L.family, L.t[0], L.t[1], L.t[2], L.t[3], L.threads, L.grid, L.lds, L.raise};
    memcpy(w + 9 * i, v, sizeof(v));
  }
  w += 9 * SMALL_MAX_LAUNCHES;
  for (int i = 0; i < p.nregions; ++i) w[2 * i] = p.region[i].offset, w[2 * i + 1] = p.region[i].bytes;
  w += 2 * SMALL_MAX_REGIONS;
  int kw[SMALL_KNOB_WORDS];
  small_knob_words(kn, kw);
  for (int i = 0; i < SMALL_KNOB_WORDS; ++i) w[i] = kw[i];
}
