// Launch plans of the tall-skinny fp64 contractions: k_tsgemm_tn (hfmi_gemm.hip), k_tsgemm_nn[_res] (hfmi_gemm_nn.hip),
// k_tsgemm_ss[b] (hfmi_skinny.hip) and the partial-sum reduction behind them.  Host only, plain C++17, nothing from HIP: given a
// shape, the knobs and the CU count a planner fills a plain struct with the instance, the grid, the split and the workspace of the
// launch; the launchers allocate, look the kernel pointer up, launch and record what the struct says, and hfmi_plan_predict
// (include/hfmi.h) writes the same records from the same structs without a device.
//
// The instance tables are stated once, as X-macro lists: the dispatch switches of the three units expand them into kernel
// instances, the planners into look-ups.  tests/helpers/contraction_plan_twin.py restates tables and planners in Python;
// tests/test_contraction_plan_cpu.py compares the two record for record.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "hfmi.h"

// ------------------------------------------------------------------ knobs
// Every tuning knob of the three dispatchers (hfmi_tuning_set, include/hfmi.h), one instance per process.  The three environment
// switches are read once, when the instance is first used.
struct tsgemm_knobs {
  int waves = 8;           // tn workgroup shape: 8 = two waves per SIMD, <= 16 accumulator tiles each; 4 = one wave, <= 32 tiles;
                           // 44 = two 4-wave workgroups with the small tiles per CU.  Measured: 8 is best or equal on every shape
  int rem4 = 1;            // last column tile of <= 12 columns in 4-column groups (4x4x4 MFMA), tn and nn
  int probe = 0;           // timing-only diagnostic of k_tsgemm_tn (-DHFMI_TN_PROBE builds)
  int tn_mt = 0;           // A/B: cap on the wave tile height of tn (0 = automatic)
  int tn_hybrid = 1;       // tn: whole rounds of row blocks coarsely split + a finely split tail
  int ss = 1;              // route skinny x skinny contractions to tsgemm_ss
  int ss_percu = 2;        // cap on resident tsgemm_ss workgroups per CU used to size the grid
  int ss_blocked = 1;      // 0 = round-robin kernel, 1 = blocked, 2 = blocked without the stage pipelining
  int nn_waves = 0;        // 0 = automatic (4 for <= 6 column tiles, else 8)
  int nn_tt = 0;           // A/B: force the nn wave-tile height (1 = tallest, 2, 3 = next smaller)
  int nn_hybrid = 1;       // split only the row tiles beyond the last full round of CUs
  int nn_res = 1;          // small matrix resident in LDS + persistent workgroups when it fits
  int nn_res_tt = 0;       // 0: tile height of nn_res by the round count; 1: always the table's; 2: always one less
  int nn_upper = 1;        // Q R^-1: skip the structurally zero column tiles of the upper-triangular small matrix
  int nn_halve_last = 0;   // overlapped rank reduction: last round of a 2-3 round product as two launches of half-height tiles (off: on
                           // one GPU the shorter tiles cost more than the smaller exposed panel saves, profiles/r04i_halve_last_ab.txt)
  int env_halve_last = -1; // HFMI_NN_HALVE_LAST: 1 / 0 overrides nn_halve_last, unset = -1
  bool env_upper_off = false;   // HFMI_NN_UPPER=0 overrides nn_upper
};
inline tsgemm_knobs& tsgemm_knobs_ref() {
  static tsgemm_knobs kn = [] {
    tsgemm_knobs k;
    const char* w = getenv("HFMI_GEMM_WAVES");
    k.waves = (w && atoi(w) == 4) ? 4 : (w && atoi(w) == 44) ? 44 : 8;
    const char* h = getenv("HFMI_NN_HALVE_LAST");
    k.env_halve_last = h ? atoi(h) : -1;
    const char* u = getenv("HFMI_NN_UPPER");
    k.env_upper_off = u && atoi(u) == 0;
    return k;
  }();
  return kn;
}
// the contraction keys of hfmi_tuning_set: true = key known and value accepted
inline bool tsgemm_knob_set(const char* key, int v) {
  tsgemm_knobs& kn = tsgemm_knobs_ref();
  auto put = [&](const char* name, int& field, bool ok) {
    if (strcmp(key, name) != 0 || !ok) return false;
    field = v;
    return true;
  };
  const bool flag = v == 0 || v == 1;
  return put("waves", kn.waves, v == 4 || v == 8 || v == 44) || put("rem4", kn.rem4, flag) || put("probe", kn.probe, true) ||
         put("tn_mt", kn.tn_mt, v >= 0 && v <= 8) || put("tn_hybrid", kn.tn_hybrid, flag) || put("ss", kn.ss, flag) ||
         put("ss_percu", kn.ss_percu, v >= 1 && v <= 4) || put("ss_blocked", kn.ss_blocked, v >= 0 && v <= 2) ||
         put("nn_waves", kn.nn_waves, v == 0 || v == 4 || v == 8) || put("nn_tt", kn.nn_tt, v >= 0 && v <= 3) ||
         put("nn_hybrid", kn.nn_hybrid, flag) || put("nn_res", kn.nn_res, flag) || put("nn_res_tt", kn.nn_res_tt, v >= 0 && v <= 2) ||
         put("nn_upper", kn.nn_upper, flag) || put("nn_halve_last", kn.nn_halve_last, flag);
}

// ------------------------------------------------------------------ instance tables
// tn: tallest wave tile (16-row MFMA tiles) by column tiles 0..16, one and two waves per SIMD.  A/B (r01e): <3,6> and <2,9> beat
// <2,6> / <1,9>; <4,5> does not beat <3,5>
#define HFMI_TN_MT_MAX_W4 0, 8, 8, 8, 8, 6, 5, 4, 4, 3, 3, 2, 2, 2, 2, 2, 2
#define HFMI_TN_MT_MAX_W8 0, 5, 5, 5, 4, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1
// tn: the tile heights and widths compiled; an (MT, NT) pair exists where MT * NT is within tn_mt_limit(WAVES)
#define HFMI_TN_MT_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8)
#define HFMI_TN_NT_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
constexpr int tn_mt_limit(int waves) { return waves == 8 ? 20 : 32; }
// nn, streaming kernel: X(NT, tallest TT of 4 waves, TT of 8 waves); 4 waves also compile the next two heights below (nn_tt_lower)
#define HFMI_NN_CASES(X)                                                                                                  \
  X(1, 8, 8) X(2, 8, 8) X(3, 8, 5) X(4, 8, 4) X(5, 6, 3) X(6, 5, 2) X(7, 4, 2) X(8, 4, 2) X(9, 3, 2) X(10, 3, 1) X(11, 2, 1) \
  X(12, 2, 1) X(13, 2, 1) X(14, 2, 1) X(15, 2, 1) X(16, 2, 1)
// nn, resident kernel: X(NT, TT); the height one below (nn_tt_lower(TT, 1)) is compiled too
#define HFMI_NN_RES_CASES(X) X(1, 4) X(2, 4) X(3, 4) X(4, 4) X(5, 3) X(6, 2) X(7, 2) X(8, 2) X(9, 2) X(10, 1)
constexpr int nn_tt_lower(int tt, int by) { return tt > by ? tt - by : 1; }
constexpr int64_t NN_RES_MIN_N = 4096;
constexpr size_t NN_RES_LDS_BYTES = 160 * 1024;
// ss, round-robin kernel: X(tiles per wave, 16-byte chunks per thread) -- every pair reachable with rt, ct <= 10 and at most 288
// staged columns, and no other; the last five are the one-operand (Gram) tile lists: rt (rt + 1) / 2 tiles, rt * 16 staged columns
#define HFMI_SS_CASES(X)                                                                                                   \
  X(1, 1) X(1, 2) X(1, 3) X(1, 4) X(1, 5) X(2, 2) X(2, 3) X(2, 4) X(2, 5) X(2, 6) X(3, 5) X(3, 6) X(4, 5) X(4, 6) X(4, 7) X(5, 6) \
  X(5, 7) X(6, 7) X(7, 7) X(7, 8) X(8, 8) X(9, 9) X(10, 9) X(11, 9)                                                        \
  X(3, 3) X(4, 4) X(5, 4) X(6, 5) X(7, 5)
// ss, blocked kernel: X(row tiles, column tiles), rt <= ct after the role swap
#define HFMI_SSB_CASES(X)                                                                                                  \
  X(2, 5) X(3, 5) X(4, 5) X(5, 5) X(2, 6) X(3, 6) X(4, 6) X(5, 6) X(6, 6) X(2, 9) X(3, 9) X(4, 9) X(5, 9) X(6, 9) X(7, 9) X(8, 9) \
  X(9, 9)

constexpr int TN_BK = 32;   // tn: reduction indices per LDS stage
constexpr int NN_KC = 32;   // nn: reduction indices per LDS stage (8 MFMA k-steps)
constexpr int SS_BK = 32;   // ss: reduction indices per stage (16 chunks of 16 bytes per column)

inline int tn_mt_max(int nt, int waves) {
  static const int t4[17] = {HFMI_TN_MT_MAX_W4}, t8[17] = {HFMI_TN_MT_MAX_W8};
  return waves == 4 ? t4[nt] : t8[nt];
}
inline bool tn_has_instance(int mt, int nt, int waves) {
  if (nt < 1 || nt > 16 || mt * nt > tn_mt_limit(waves)) return false;
#define X(M) if (mt == M) return true;
  HFMI_TN_MT_CASES(X)
#undef X
  return false;
}
inline bool nn_case(int nt, int* tt4, int* tt8) {
#define X(NTV, TT4, TT8) if (nt == NTV) { *tt4 = TT4; *tt8 = TT8; return true; }
  HFMI_NN_CASES(X)
#undef X
  return false;
}
inline int nn_res_case(int nt) {   // 0: none
#define X(NTV, TTV) if (nt == NTV) return TTV;
  HFMI_NN_RES_CASES(X)
#undef X
  return 0;
}
inline bool ss_has_instance(int tpw, int nq) {
#define X(T, Q) if (tpw == T && nq == Q) return true;
  HFMI_SS_CASES(X)
#undef X
  return false;
}
inline bool ssb_has_instance(int rt, int ct) {
#define X(R, Cc) if (rt == R && ct == Cc) return true;
  HFMI_SSB_CASES(X)
#undef X
  return false;
}
constexpr int ss_pf(int tpw, int nq) { return (tpw <= 4 && nq <= 6) ? 2 : 1; }

// ------------------------------------------------------------------ helpers
inline int64_t plan_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int plan_cus(int num_cus) { return num_cus > 0 ? num_cus : 256; }
// number of 4-column groups the last of nt column tiles is computed in (0 = as a full 16-column tile)
inline int plan_r4(int cols, int nt, int rem4) {
  const int rem = cols - (nt - 1) * 16;
  return (rem4 && rem <= 12) ? (rem + 3) / 4 : 0;
}
// one record: word 0 = kind (HFMI_PLAN_*), then the fields in the order include/hfmi.h lists them, zero filled
inline void plan_words(int* w, int kind, std::initializer_list<int> fields) {
  int i = 0;
  w[i++] = kind;
  for (int v : fields)
    if (i < HFMI_PLAN_WORDS) w[i++] = v;
  while (i < HFMI_PLAN_WORDS) w[i++] = 0;
}

// ------------------------------------------------------------------ partial-sum reduction
// C[i rs + j cs] = scale * sum_sp part[sp] + beta * C over nsplit slices `pstride` apart, slice rows `inner_ld` apart (tr: the
// slices hold the transpose).  part_off / c_off: where the slices and the m x k result start, relative to the launch's workspace and C.
struct reduce_call {
  int nsplit;
  int64_t pstride;
  int inner_ld;
  bool tr;
  int m, k;
  int64_t part_off, c_off;
};
struct reduce_plan {
  int route, ry;                     // HFMI_REDUCE_*, split lanes (0: the vector kernel)
  int nsplit, tr, m, k;
  unsigned gx, gy;
  int64_t rowlen, kpad, crow;        // vector kernel: row length, padded / real columns of a long row, row stride of C
  int nrows, kreal;
};
inline reduce_plan reduce_plan_make(const reduce_call& c, int64_t rs, int64_t cs, bool ptrs_aligned) {
  reduce_plan p = {};
  const int m = c.m, k = c.k, inner_ld = c.inner_ld;
  const bool tr = c.tr;
  p.nsplit = c.nsplit;
  p.m = m;
  p.k = k;
  const int fastn = tr ? m : k, slown = tr ? k : m;
  // vector path: fast axis contiguous and even-strided on both sides, pointers 16-byte aligned, enough work to matter
  const int64_t cfast = tr ? rs : cs, crow = tr ? cs : rs;
  const bool aligned = ptrs_aligned && c.pstride % 2 == 0 && inner_ld % 2 == 0 && crow % 2 == 0;
  if (cfast == 1 && aligned && (int64_t)fastn * slown >= 65536) {
    const bool long_row = !tr && rs == inner_ld;
    if (long_row) {                       // rows are back to back on both sides: one long row, pad columns zeroed
      p.rowlen = (int64_t)m * inner_ld;
      p.nrows = 1;
      p.kpad = inner_ld;
      p.kreal = k;
    } else {
      p.rowlen = fastn & ~1;              // an odd fast extent: not this kernel, the scalar kernels below take the whole reduction
      p.nrows = slown;
    }
    if (p.rowlen == fastn || long_row) {  // (a single row of odd length is no long row: its last element needs the scalar kernel)
      p.route = long_row ? HFMI_REDUCE_VEC_LONG : HFMI_REDUCE_VEC_ROWS;
      p.tr = tr ? 1 : 0;
      p.crow = crow;
      p.gx = (unsigned)((p.rowlen / 2 + 255) / 256);
      p.gy = (unsigned)(p.nrows < 32768 ? p.nrows : 32768);
      return p;
    }
  }
  p.ry = c.nsplit <= 32 ? 4 : 16;
  if (!tr && cs == 1 && rs == inner_ld && (int64_t)m * inner_ld >= 65536) {
    p.route = HFMI_REDUCE_FLAT;
    p.rowlen = (int64_t)m * inner_ld;     // all entries of a slice
    p.gx = (unsigned)((p.rowlen + 63) / 64);
    p.gy = 1;
    return p;
  }
  p.route = HFMI_REDUCE_PARTIALS;
  p.tr = tr ? 1 : 0;
  p.gx = (unsigned)((fastn + 63) / 64);
  p.gy = (unsigned)(slown < 32768 ? slown : 32768);
  return p;
}
inline void reduce_plan_words(const reduce_plan& p, int* w) {
  plan_words(w, HFMI_PLAN_REDUCE, {p.route, p.ry, p.nsplit, p.tr, p.m, p.k});
}

// ------------------------------------------------------------------ tsgemm_tn, one panel of at most 256 columns
// Row blocks [0, nrb) are split nsplit ways over the reduction axis; with the hybrid plan they are the whole rounds of the CUs and
// the tail_nrb blocks behind them are split tail_nsplit ways into their own, compact partial buffer behind the first one.
struct tn_plan {
  bool has_instance;
  int mt, nt, waves, tr, r4;         // instance <MT, NT, TR, WAVES, R4>
  int kpad;
  int64_t Npad;
  size_t shmem;
  int nrb, nsplit, mpad;
  int64_t chunk;
  bool direct;                       // one split, nothing to scale or accumulate: the kernel writes C itself
  int tail_nrb, tail_nsplit, tail_mpad;
  int64_t tail_chunk, tail_off;      // tail_off: doubles in front of the tail's partial buffer
  int grid;
  size_t ws_bytes;
  int nred;
  reduce_call red[2];
};
// C is addressed as C[i rs + j cs]; aliased: C is one of the operands (no direct write)
inline tn_plan tn_plan_make(int m, int k, int64_t N, double scale, double beta, int64_t rs, int64_t cs, bool aliased, int nsplit_req,
                            const tsgemm_knobs& kn, int num_cus) {
  tn_plan p = {};
  const int nt = (k + 15) / 16;
  const int kpad = nt * 16;
  const int64_t Npad = plan_round_up(N, TN_BK);
  const bool tr = (rs == 1 && cs != 1);  // column-major output: coalesce along i
  // wave tile height: as tall as the accumulator budget allows, but no taller than the problem needs
  // waves: 8 = one 8-wave workgroup per CU (two waves per SIMD); 4 = one 4-wave workgroup with big tiles;
  // 44 = 4-wave workgroups with the small (two-per-SIMD) tiles, TWO workgroups per CU: their stage barriers are not
  // synchronised with each other, so one workgroup's MFMAs cover the other's barrier / staging bubbles
  const int wcfg = (nt > 11) ? 4 : kn.waves;   // very wide panels: the 2-waves/SIMD register budget is too tight
  const bool small4 = wcfg == 44;
  const int waves = small4 ? 4 : wcfg;
  const int row_tiles = (m + 15) / 16;
  int mt = nt <= 16 ? tn_mt_max(nt, small4 ? 8 : waves) : 1;
  const int need = (row_tiles + waves - 1) / waves;
  if (need < mt) mt = need;
  if (kn.tn_mt > 0 && kn.tn_mt < mt) mt = kn.tn_mt;
  if (mt == 7) mt = 6;
  if (mt < 1) mt = 1;
  const int rows_per_block = 16 * waves * mt;
  const int nrb = (m + rows_per_block - 1) / rows_per_block;
  const int mpad = nrb * rows_per_block;
  // split the long axis so that the grid fills the chip in (nearly) whole rounds of CUs
  const int cus = plan_cus(num_cus) * (small4 ? 2 : 1);   // resident workgroup slots
  const int64_t stages = Npad / TN_BK;
  int nsplit = nsplit_req;
  if (nsplit <= 0) {
    int best = 1;
    double best_cost = 1e300;
    for (int ns = 1; ns <= 128; ++ns) {
      if (ns > 1 && stages / ns < 16) break;
      const int64_t blocks = (int64_t)nrb * ns;
      const int64_t rounds = (blocks + cus - 1) / cus;
      const double eff = (double)blocks / (double)(rounds * cus);
      const double part_ratio = 2.0 * ns * (double)mpad * kpad / ((double)N * (m + k));
      const double cost = 1.0 / eff + part_ratio;
      if (cost < best_cost - 1e-12) {
        best_cost = cost;
        best = ns;
      }
    }
    nsplit = best;
  }
  // Hybrid plan: when the row blocks make at least one whole round of the CUs, the rounds that ARE whole need no fine split at
  // all (ns_full = 1 or 2: their partial traffic is a single slice or none) and only the blocks beyond them are split finely
  // enough to fill one more round for 1 / ns_tail of a block's time.  m = 1e5 (config 2): 261 blocks = 256 whole + 5 x 51 instead
  // of 261 x 19 (the uniform plan's best: 3 % quantisation loss, 1.5 GB of partials written and read back, a 0.3 ms reduction);
  // m = 51200 (config 4): 128 x 2 + 6 x 42 instead of 134 x 21 (0.7 GB of partials, 0.12 ms).
  const bool can_direct = (scale == 1.0 && beta == 0.0 && !aliased);
  int ns_full = 0, nrb_full = 0, ns_tail = 0;
  if (nsplit_req <= 0 && kn.tn_hybrid) {
    const double ideal = (double)nrb / cus;
    const double part_unit = 2.0 * (double)rows_per_block * kpad / ((double)N * (m + k));   // one slice of one row block
    double uniform_cost;
    {
      const int64_t blocks = (int64_t)nrb * nsplit;
      const int64_t rounds = (blocks + cus - 1) / cus;
      uniform_cost = (double)(rounds * cus) / (double)blocks + part_unit * nsplit * nrb;
    }
    double best_cost = uniform_cost;
    static const int cand[] = {1, 2, 3, 4, 6, 8};
    for (int ci = 0; ci < 6; ++ci) {
      const int nsf = cand[ci];
      if (nsf > 1 && stages / nsf < 16) break;
      const int64_t R = ((int64_t)nrb * nsf) / cus;            // whole rounds of full-region workgroups
      if (R < 1 || (R * cus) % nsf != 0) continue;
      const int nf = (int)(R * cus / nsf);
      const int nt_blocks = nrb - nf;
      if (nt_blocks <= 0) continue;                             // the uniform plan already is this one
      int nst = cus / nt_blocks;
      if (nst > stages / 16) nst = (int)(stages / 16);
      if (nst > 128) nst = 128;
      if (nst < 1) nst = 1;
      const int64_t tail_rounds = ((int64_t)nt_blocks * nst + cus - 1) / cus;
      const double time = (double)R / nsf + (double)tail_rounds / nst;
      const double parts = part_unit * ((nsf == 1 && can_direct ? 0.0 : (double)nsf * nf) + (double)nst * nt_blocks);
      const double cost = time / ideal + parts;
      if (cost < best_cost - 1e-9) {
        best_cost = cost;
        ns_full = nsf;
        nrb_full = nf;
        ns_tail = nst;
      }
    }
  }
  p.has_instance = tn_has_instance(mt, nt, waves);
  p.mt = mt;
  p.nt = nt;
  p.waves = waves;
  p.tr = tr ? 1 : 0;
  // columns of the last tile: up to 12 are done as 1..3 groups of 4 with the 4x4x4 MFMA (16 instead of 64 cycles each)
  p.r4 = waves == 8 ? plan_r4(k, nt, kn.rem4) : 0;
  p.kpad = kpad;
  p.Npad = Npad;
  p.shmem = (size_t)2 * nt * 16 * (TN_BK + 2) * sizeof(double);
  if (ns_full > 0) {
    const int nrb_t = nrb - nrb_full;
    p.nrb = nrb_full;
    p.mpad = nrb_full * rows_per_block;   // every row of the whole rounds is a real row (only the last block is ragged)
    p.chunk = plan_round_up((Npad + ns_full - 1) / ns_full, TN_BK);
    p.nsplit = (int)((Npad + p.chunk - 1) / p.chunk);
    p.tail_nrb = nrb_t;
    p.tail_mpad = nrb_t * rows_per_block;
    p.tail_chunk = plan_round_up((Npad + ns_tail - 1) / ns_tail, TN_BK);
    p.tail_nsplit = (int)((Npad + p.tail_chunk - 1) / p.tail_chunk);
    p.direct = p.nsplit == 1 && can_direct;
    p.tail_off = p.direct ? 0 : (int64_t)p.nsplit * p.mpad * kpad;
    p.ws_bytes = ((size_t)p.tail_off + (size_t)p.tail_nsplit * p.tail_mpad * kpad) * sizeof(double);
    if (!p.direct) p.red[p.nred++] = {p.nsplit, (int64_t)p.mpad * kpad, tr ? p.mpad : kpad, tr, p.mpad, k, 0, 0};
    p.red[p.nred++] = {p.tail_nsplit, (int64_t)p.tail_mpad * kpad, tr ? p.tail_mpad : kpad, tr, m - p.mpad, k, p.tail_off, (int64_t)p.mpad * rs};
  } else {
    p.nrb = nrb;
    p.mpad = mpad;
    p.chunk = plan_round_up((Npad + nsplit - 1) / nsplit, TN_BK);
    if (p.chunk < TN_BK) p.chunk = TN_BK;
    p.nsplit = (int)((Npad + p.chunk - 1) / p.chunk);
    if (p.nsplit < 1) p.nsplit = 1;
    p.direct = p.nsplit == 1 && can_direct;   // blocks never overlap partially
    p.ws_bytes = (size_t)p.nsplit * mpad * kpad * sizeof(double);
    if (!p.direct) p.red[p.nred++] = {p.nsplit, (int64_t)mpad * kpad, tr ? mpad : kpad, tr, m, k, 0, 0};
  }
  p.grid = p.nrb * p.nsplit + p.tail_nrb * p.tail_nsplit;
  return p;
}
inline void tn_plan_words(const tn_plan& p, int* w) {
  plan_words(w, HFMI_PLAN_TN, {p.mt, p.nt, p.waves, p.tr, p.r4, p.grid, p.nrb, p.nsplit, p.direct ? 1 : 0, p.tail_nrb, p.tail_nsplit});
}

// ------------------------------------------------------------------ tsgemm_nn, one panel of at most 256 columns
// One kernel launch of a plan.  The arguments are the kernel's: row tiles [full_base, full_base + full_tiles) are computed whole,
// tail_tiles tiles from tail_base on are split msplit ways into the partial buffer.  k_reduce_nn and the row-panel hook (rows
// [hook_row0, hook_row0 + hook_rows) are final; hook_rows = 0: no call) follow the launch in that order.
struct nn_launch {
  bool half;                         // the kernel of half the plan's tile height
  int grid, tail_tiles, msplit, full_tiles, full_base, tail_base;
  bool reduce;
  int64_t hook_row0, hook_rows;
  int rec_tt, rec_tail;              // plan record: tile height, split tiles (the kernel wants tail_tiles >= 1)
};
constexpr int NN_MAX_PANELS = 8;     // row panels of an overlapped rank reduction (the context has as many events)
struct nn_plan {
  bool has_instance;
  bool res;                          // the LDS-resident kernel with persistent workgroups: <TT, NT, R4, UPPER>, one launch
  int tt, nt, waves, r4, upper;
  size_t shmem;
  int tile_rows, ntiles, grid;
  // streaming kernel <TT, NT, WAVES, R4>
  int msplit, mchunk, full_tiles, tail_tiles;
  int64_t ldo, pstride;              // leading dimension and slice stride of the partial buffer (msplit > 1)
  size_t ws_bytes;
  int64_t reduce_row0;
  unsigned reduce_gx;
  bool hooked, halved;               // issued as row panels: the hook is called; the last round by the half-height kernel
  int nlaunch;
  nn_launch launch[NN_MAX_PANELS + 2];
};
// Time model of a tile of `tile_rows` rows: how many ways to split the reduction axis m so that the grid fills the CUs in (nearly)
// whole rounds.  The kernel is MFMA bound, the split partials only cost their own HBM round trip in k_reduce_nn:
// t = flops / (eff * rate) + (msplit + 1) * N * r * 8 / hbm.
inline double nn_cost(int num_cus, int tile_rows, int m, int r, int64_t N, double rate_factor, int* msplit_out) {
  const int cus = plan_cus(num_cus);
  const int64_t ntiles = (N + tile_rows - 1) / tile_rows;
  const int stages = (m + NN_KC - 1) / NN_KC;
  const double flops = 2.0 * (double)ntiles * tile_rows * (double)m * (double)(((r + 15) / 16) * 16);
  const double rate = 60e12 * rate_factor, hbm = 4.0e12;
  int best = 1;
  double best_t = 1e300;
  for (int ns = 1; ns <= 64; ++ns) {
    if (ns > 1 && stages / ns < 8) break;
    const int64_t blocks = ntiles * ns;
    const int64_t rounds = (blocks + cus - 1) / cus;
    const double eff = (double)blocks / (double)(rounds * cus);
    const double t = flops / (eff * rate) + (ns > 1 ? (ns + 1.0) * (double)N * r * 8.0 / hbm + 3e-6 : 0.0);
    if (t < best_t - 1e-12) {
      best_t = t;
      best = ns;
    }
  }
  *msplit_out = best;
  return best_t;
}
// the streaming kernel at tile height p.tt: split, partial buffer and the list of launches
inline void nn_plan_stream(nn_plan& p, int m, int r, int64_t N, int msplit, bool tail_split, int hook_panels, const tsgemm_knobs& kn,
                           int num_cus) {
  const int cus = plan_cus(num_cus);
  const int tile_rows = 16 * p.tt * p.waves;
  const int ntiles = (int)((N + tile_rows - 1) / tile_rows);
  const int sld = p.nt * 16 + ((p.nt % 2 == 0) ? 16 : 0);
  p.shmem = (size_t)2 * NN_KC * sld * sizeof(double);
  p.r4 = plan_r4(r, p.nt, kn.rem4);
  // msplit > 1 means the time model found the row tiles badly quantised over the CUs.  With at least one full round of
  // tiles, only the tiles beyond the last full round are split (see the kernel); otherwise every tile is.
  int full_tiles = 0;
  if ((msplit > 1 || tail_split) && ntiles >= cus && kn.nn_hybrid) {
    full_tiles = ntiles / cus * cus;
    const int tail = ntiles - full_tiles;
    if (tail == 0) {
      msplit = 1;
    } else {
      const int stages = (m + NN_KC - 1) / NN_KC;
      // split the tail tiles ms ways so that their pieces fill whole rounds of CUs: the tail then costs
      // ceil(tail ms / cus) / ms of a round instead of a whole one (config 3: 162 tail tiles, ms = 3 -> 486 pieces = 2 rounds
      // of a third each = 0.67 of a round; unsplit it was the 8th round of 7.63).  A few tail tiles: one round of short pieces.
      int ms = cus / tail;
      if (ms < 2) {
        double best = 1.0;
        ms = 1;
        for (int c = 2; c <= 8; ++c) {
          const double cost = (double)((tail * c + cus - 1) / cus) / c + 0.01 * c;     // + the partials' round trip
          if (cost < best - 1e-9) {
            best = cost;
            ms = c;
          }
        }
      }
      if (ms > stages / 4) ms = stages / 4;                 // at least four LDS stages per workgroup
      if (ms < 1) ms = 1;
      msplit = ms;
      if (msplit == 1) full_tiles = 0;                      // nothing to split: plain launch
    }
  }
  const int mchunk = (int)plan_round_up((m + msplit - 1) / msplit, NN_KC);
  msplit = (m + mchunk - 1) / mchunk;
  if (msplit > 1) {
    p.ldo = plan_round_up(N, 32);
    p.pstride = p.ldo * r;
    p.ws_bytes = (size_t)msplit * p.pstride * sizeof(double);
  } else {
    full_tiles = 0;
  }
  const int tail_tiles = ntiles - full_tiles;
  p.tile_rows = tile_rows, p.ntiles = ntiles, p.msplit = msplit, p.mchunk = mchunk;
  p.full_tiles = full_tiles, p.tail_tiles = tail_tiles, p.grid = full_tiles + tail_tiles * msplit;
  p.reduce_row0 = (int64_t)full_tiles * tile_rows;          // multiple of 64
  int64_t gx = ((N - p.reduce_row0 + 1) / 2 + 255) / 256;
  if (gx > 2048) gx = 2048;
  if (gx < 1) gx = 1;
  p.reduce_gx = (unsigned)gx;
  // a launch of `cnt` whole tiles from tile `first` on, both in tiles of the launched height
  auto whole = [&](bool half, int cnt, int first, int64_t row0, int64_t rows) {
    p.launch[p.nlaunch++] = {half, cnt, 1, 1, cnt, first, 0, false, row0, rows, half ? p.tt / 2 : p.tt, 0};
  };
  // a launch of `cnt` whole tiles from `first` on and `tl` tail tiles split msplit ways, with the reduction behind it if `reduce`
  auto split = [&](int cnt, int first, int tl, bool reduce, int64_t row0, int64_t rows) {
    p.launch[p.nlaunch++] = {false, cnt + tl * msplit, tl > 0 ? tl : 1, msplit, cnt, first, full_tiles, reduce, row0, rows, p.tt, tl};
  };
  const int whole_cnt = msplit > 1 ? full_tiles : ntiles;   // tiles computed in one piece
  const int rounds = whole_cnt / cus;
  if (hook_panels <= 0 || rounds < 2) {
    split(full_tiles, 0, tail_tiles, msplit > 1, 0, 0);
    return;
  }
  // Row panels for an overlapped rank reduction (hook_panels > 0): whole rounds of tiles per launch, the hook is told which rows
  // are final after each.  Tiles keep the plan of the single launch, so the results are the same bits.  A round's tiles finish
  // together, so with R rounds the last panel is 1/R of the block and its reduction is exposed.  When every round already is its
  // own panel and one more panel is allowed, the LAST round is issued as two launches of tiles of HALF the height (same
  // reduction order per row: still the same bits): its first half is final -- and on its way through the fabric -- while the
  // second half is computed, and only a quarter of a two-round product is left exposed.
  if (hook_panels > NN_MAX_PANELS) hook_panels = NN_MAX_PANELS;
  const int panels = rounds < hook_panels ? rounds : hook_panels;
  const bool on = kn.env_halve_last >= 0 ? kn.env_halve_last != 0 : kn.nn_halve_last != 0;
  p.hooked = true;
  p.halved = on && p.tt % 2 == 0 && panels == rounds && panels + 1 <= hook_panels;
  int base = 0;
  for (int q = 0; q < panels; ++q) {
    const bool last = q == panels - 1;
    const int cnt = last ? whole_cnt - base : (rounds / panels + (q < rounds % panels ? 1 : 0)) * cus;
    const int tl = (last && msplit > 1) ? tail_tiles : 0;
    const int64_t row0 = (int64_t)base * tile_rows, row1 = last ? N : (int64_t)(base + cnt) * tile_rows;
    if (last && p.halved) {
      // the two halves of the round (the last half-height tile may be ragged: rows >= N are never stored), then the split tail
      // tiles; the rows behind the first half are final when the last of these launches is
      const int cnt_a = cnt / 2, cnt_b = cnt - cnt_a;       // in tiles of the full height
      const int64_t mid = (int64_t)(base + cnt_a) * tile_rows;
      whole(true, 2 * cnt_a, 2 * base, row0, mid - row0);
      whole(true, 2 * cnt_b, 2 * (base + cnt_a), tl > 0 ? 0 : mid, tl > 0 ? 0 : N - mid);
      if (tl > 0) split(0, base, tl, true, mid, N - mid);
    } else if (msplit > 1) {
      split(cnt, base, tl, last, row0, row1 - row0);
    } else {
      whole(false, cnt, base, row0, row1 - row0);
    }
    base += cnt;
  }
}
// upper_hint: the caller knows the small matrix is upper triangular; hook_panels: most row panels of an overlapped rank reduction
// (0: no hook)
inline nn_plan nn_plan_make(int m, int r, int64_t N, bool upper_hint, int hook_panels, const tsgemm_knobs& kn, int num_cus) {
  nn_plan p = {};
  const int cus = plan_cus(num_cus);
  const int nt = (r + 15) / 16;
  p.nt = nt;
  p.has_instance = true;
  // S whole in LDS (one workgroup per CU): [round_up(m, 4)][SLD] doubles.  In-place products (Y == A: Q <- Q R^-1) are
  // fine: a workgroup reads the rows of a tile completely before it stores them, and tiles do not overlap.
  const int ttv = (kn.nn_res && N >= NN_RES_MIN_N) ? nn_res_case(nt) : 0;
  if (ttv > 0) {
    const int sld = nt * 16 + ((nt % 2 == 0) ? 16 : 0);
    const size_t shmem = (size_t)((m + 3) & ~3) * sld * sizeof(double);
    if (shmem <= NN_RES_LDS_BYTES) {
      // Tile height: the persistent workgroups take whole tiles of 128 TT rows in turn, so the product costs
      // ceil(tiles / CUs) rounds of TT units each.  N = 2e5 with TT = 3 is 521 tiles = 2.03 rounds -> 3 rounds (9 units) where
      // TT = 2 needs 4 rounds of 2 (8 units): the shorter tile is taken when it saves more than the ~5 % its worse
      // MFMA-to-LDS ratio costs.
      auto units = [&](int tt) {
        const int64_t tiles = (N + 128 * tt - 1) / (128 * tt);
        return (double)((tiles + cus - 1) / cus) * tt;
      };
      const int tl = nn_tt_lower(ttv, 1);
      const bool lower = kn.nn_res_tt == 2 || (kn.nn_res_tt == 0 && tl != ttv && units(tl) * 1.05 < units(ttv));
      p.res = true;
      p.tt = lower ? tl : ttv;
      p.waves = 8;
      p.r4 = plan_r4(r, nt, kn.rem4);
      p.upper = (upper_hint && kn.nn_upper && !kn.env_upper_off) ? 1 : 0;
      p.shmem = shmem;
      p.tile_rows = 16 * p.tt * 8;
      p.ntiles = (int)((N + p.tile_rows - 1) / p.tile_rows);
      p.grid = p.ntiles < cus ? p.ntiles : cus;
      p.msplit = 1;
      p.full_tiles = p.ntiles;
      return p;
    }
  }
  int tt4 = 0, tt8 = 0;
  if (!nn_case(nt, &tt4, &tt8)) {
    p.has_instance = false;
    return p;
  }
  p.waves = kn.nn_waves ? kn.nn_waves : (nt >= 7 ? 8 : 4);   // A/B (scripts/nn_waves_ab.py, r01g): one wave per SIMD wins up to 6 column tiles
  int ms = 1;
  bool tail_split = false;
  if (p.waves == 8) {
    p.tt = tt8;
    nn_cost(num_cus, 128 * tt8, m, r, N, 1.0, &ms);
  } else {
    // one wave per SIMD: the tile height is chosen among the table's and the two below it together with the reduction split, by
    // the time model -- a slightly shorter tile often fills the last round of CUs
    const int t1 = nn_tt_lower(tt4, 1), t2 = nn_tt_lower(tt4, 2);
    int ms0 = 1, ms1 = 1, ms2 = 1;
    const double c0 = nn_cost(num_cus, 64 * tt4, m, r, N, 1.0, &ms0);
    const double c1 = (t1 != tt4) ? nn_cost(num_cus, 64 * t1, m, r, N, 0.98, &ms1) : 1e300;
    const double c2 = (t2 != t1) ? nn_cost(num_cus, 64 * t2, m, r, N, 0.96, &ms2) : 1e300;
    // With at least one full round of the tallest tiles the quantisation is handled by splitting only the tail tiles
    // (nn_plan_stream), so the tallest tile -- the best MFMA-to-LDS ratio -- is taken (A/B r01e: config 4 nn 56.5 -> 59.7 TF)
    if (kn.nn_hybrid && kn.nn_tt == 0 && (N + 64 * tt4 - 1) / (64 * tt4) >= cus && m >= 16 * NN_KC) p.tt = tt4, ms = 1, tail_split = true;
    else if (kn.nn_tt == 1) p.tt = tt4, ms = ms0;
    else if (kn.nn_tt == 2) p.tt = t1, ms = ms1;
    else if (kn.nn_tt == 3) p.tt = t2, ms = ms2;
    else if (c0 <= c1 && c0 <= c2) p.tt = tt4, ms = ms0;
    else if (c1 <= c2) p.tt = t1, ms = ms1;
    else p.tt = t2, ms = ms2;
  }
  nn_plan_stream(p, m, r, N, ms, tail_split, hook_panels, kn, num_cus);
  return p;
}
inline void nn_res_plan_words(const nn_plan& p, int* w) {
  plan_words(w, HFMI_PLAN_NN_RES, {p.tt, p.nt, 8, p.r4, p.upper, 1, p.ntiles, 0, p.grid});
}
// tile height, the split, whole and split tiles one launch covers, grid
inline void nn_launch_words(const nn_plan& p, const nn_launch& l, int* w) {
  plan_words(w, HFMI_PLAN_NN, {l.rec_tt, p.nt, p.waves, p.r4, 0, l.msplit, l.full_tiles, l.rec_tail, l.grid});
}

// ------------------------------------------------------------------ tsgemm_ss
inline bool ss_applicable(int m, int k, bool same) {
  const int rt = (m + 15) / 16, ct = (k + 15) / 16;
  if (rt < 1 || ct < 1 || rt > 10 || ct > 10) return false;
  const int ctot = same ? rt * 16 : (rt + ct) * 16;
  return ctot <= 288;
}
struct ss_plan {
  bool has_instance;
  bool same, swap, blocked, pipe;    // swap: the blocked kernel runs with the operand roles exchanged
  int rt, ct;                        // row / column tiles as launched (after the swap)
  int tpw, nq, pf;                   // round-robin instance <TPW, NQ, PF>; the blocked one is <RT, CTL, NQ, PIPE>
  size_t shmem;
  int per_cu, nsplit;
  int64_t Npad, chunk;
  size_t ws_bytes;
  reduce_call red;
};
// same: one operand against itself (A == B, equal strides, m == k)
inline ss_plan ss_plan_make(int m, int k, int64_t N, bool same, int nsplit_req, const tsgemm_knobs& kn, int num_cus) {
  ss_plan p = {};
  const int rt = (m + 15) / 16, ct = (k + 15) / 16;
  const int ctot = same ? rt * 16 : (rt + ct) * 16;
  p.Npad = plan_round_up(N, SS_BK);
  p.same = same;
  p.swap = !same && rt > ct;                      // the blocked variant wants rt <= ct: exchange the operand roles
  p.rt = p.swap ? ct : rt;
  p.ct = p.swap ? rt : ct;
  p.blocked = !same && kn.ss_blocked && ssb_has_instance(p.rt, p.ct);
  p.tpw = ((same ? rt * (rt + 1) / 2 : rt * ct) + 7) / 8;
  p.nq = (ctot + 31) / 32;  // staged columns are padded to 32 (one 16-byte chunk per thread per 32 columns)
  p.pf = ss_pf(p.tpw, p.nq);
  p.has_instance = p.blocked || ss_has_instance(p.tpw, p.nq);
  // pipelined stages where the fragments fit next to two register stages (measured, scripts/ss_shapes.py: n = 32 / 48 / 64 at
  // k = 138 +4 / +2.5 / +2 %; the 9 x 9 tile shape loses 10 % to the registers the carried fragments cost)
  p.pipe = p.blocked && kn.ss_blocked != 2 && p.rt * p.ct <= 56;
  // unpadded stage buffers: one for the HBM-bound variants (PF = 2), two plus the column pointer table otherwise
  const size_t stage_bytes = (size_t)p.nq * 32 * SS_BK * sizeof(double);
  p.shmem = (p.pf == 2 && !p.blocked) ? stage_bytes : 2 * stage_bytes + (size_t)p.nq * 32 * sizeof(double*);
  // workgroups resident per CU: LDS (160 KB) and registers (TPW <= 4 compiles for 4 waves per SIMD = 2 workgroups)
  int per_cu = (int)((160 * 1024) / p.shmem);
  const int reg_cap = (p.tpw <= 4 && !p.blocked) ? kn.ss_percu : 1;
  if (per_cu > reg_cap) per_cu = reg_cap;
  if (per_cu < 1) per_cu = 1;
  p.per_cu = per_cu;
  const int64_t stages = p.Npad / SS_BK;
  int nsplit = nsplit_req > 0 ? nsplit_req : plan_cus(num_cus) * per_cu;
  if (nsplit > stages / 2) nsplit = (int)(stages / 2);
  if (nsplit < 1) nsplit = 1;
  p.chunk = plan_round_up((p.Npad + nsplit - 1) / nsplit, SS_BK);
  p.nsplit = (int)((p.Npad + p.chunk - 1) / p.chunk);
  const int mpad = rt * 16, kpad = ct * 16;
  p.ws_bytes = (size_t)p.nsplit * mpad * kpad * sizeof(double);
  // swapped roles: the partial tiles hold (A^T B)^T = B^T A, k x m with row stride mpad
  const bool sw = p.blocked && p.swap;
  p.red = {p.nsplit, (int64_t)mpad * kpad, sw ? mpad : kpad, sw, m, k, 0, 0};
  return p;
}
inline void ss_plan_words(const ss_plan& p, int* w) {
  if (p.blocked) plan_words(w, HFMI_PLAN_SSB, {p.rt, p.ct, p.nq, p.pipe ? 1 : 0, p.swap ? 1 : 0, 0, p.nsplit});
  else plan_words(w, HFMI_PLAN_SS, {p.tpw, p.nq, p.pf, 0, p.same ? 1 : 0, p.nsplit});
}
