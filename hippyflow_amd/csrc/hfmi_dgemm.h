// The general fp64 MFMA product of hfmi_dgemm.hip.
#pragma once
#include <stdint.h>

#include "hfmi_internal.h"

// C (M x N) = alpha (op(A) op(B) + op(A2) op(B2)) + beta C, everything column-major.  op(A) = A (M x K, lda) or A^T (A is K x M);
// op(B) = B (K x N) or B^T (B is N x K); the second product (K2 columns, same shapes and leading dimensions) is optional.
// batch > 1: `batch` independent products, element strides sA, sB, sC; not together with a second product.
struct gemm_desc {
  bool ta, tb;
  int M, N, K;
  double alpha, beta;
  const double *A, *B;
  int64_t lda, ldb;
  double* C;
  int64_t ldc;
  int K2 = 0;
  const double *A2 = nullptr, *B2 = nullptr;
  int batch = 1;
  int64_t sA = 0, sB = 0, sC = 0;
  int lower = 0;            // symmetric update: > 0 = 1 + (first row of C mod 128): tiles above the diagonal 128-blocks are skipped (pipelined kernel only)
  // triangular operands, in 64 x 64 tiles (block row bx, block column by of C); no K2, and only (ta, tb) = (false, true) and (false, false):
  //   bit 0: tiles with by > bx are skipped (the lower triangle of C is kept);
  //   bit 1: the reduction stops at (bx + 1) * 64 (op(A) lower triangular);  bit 2: it starts at by * 64 (op(B) lower triangular)
  int cut = 0;
  const int* skip = nullptr;   // device flag: the launch is a no-op when skip[0] != 0
};
int launch_dgemm(hfmi_ctx* ctx, const gemm_desc& g);

// ------------------------------------------------------------------------------------------------ route (host only, no HIP)
// What launch_dgemm does with a descriptor: which kernel, which load path, which grid, or which refusal.  launch_dgemm launches what
// this says; hfmi_dgemm_route_predict (include/hfmi.h) evaluates it without a context or a device, hfmi_test_dgemm returns it for the
// launch that ran, and tests/helpers/dgemm_twin.py restates it.  The values are HFMI_DGEMM_* of include/hfmi.h.
struct gemm_route {
  int kernel = HFMI_DGEMM_NONE;   // HFMI_DGEMM_K64 (k_dgemm<.., false>), _K64_CUT (k_dgemm<.., true>), _P128 / _P64 (k_dgemm_p<.., 128 | 64>)
  int vec = 0;                    // pipelined kernels: 1 = 16-byte loads for interior tiles (every operand even in offset, ld and stride)
  int gx = 0, gy = 0, gz = 0;     // grid; all zero: nothing is launched (M <= 0 or N <= 0, or a refusal)
  int error = HFMI_DGEMM_ERR_NONE;
};
// `pipelined`: the value of HFMI_EIG_GEMM (dgemm_pipelined_switch(): read once per process, 1 when unset).
// One rule: a descriptor with a cut or a skip flag always runs the 64 x 64 kernel, never the pipelined one (its clients rely on the
// tile size of the cuts and on the bits of that kernel).
inline gemm_route dgemm_route_make(const gemm_desc& g, int pipelined) {
  gemm_route r;
  if (g.M <= 0 || g.N <= 0) return r;
  // k_dgemm does not move A2 / B2 by the batch index (k_dgemm_p does): a second product takes no batch, whichever kernel would run.
  // (The eleven scalar instructions of that offset in k_dgemm's prologue move its main loop by 44 bytes and cost the small TN products
  // of the eigensolver 2 %: docs/measurements.md, dgemm-rate section.  No caller combines the two.)
  if (g.K2 > 0 && g.batch > 1) {
    r.error = HFMI_DGEMM_ERR_K2_BATCH;
    return r;
  }
  const bool cut = g.cut != 0 || g.skip != nullptr;
  if (cut && (g.K2 > 0 || g.ta)) {
    r.error = HFMI_DGEMM_ERR_CUT;
    return r;
  }
  // the pipelined kernel where its tiles fill the chip: 128 x 128 from 192 tiles on, 64 x 128 from 192 of those; the 64 x 64 kernel
  // for the small products (panel factors, merges of small nodes)
  const int64_t t128 = (int64_t)((g.M + 127) / 128) * ((g.N + 127) / 128) * g.batch;
  const int64_t t64 = (int64_t)((g.M + 63) / 64) * ((g.N + 127) / 128) * g.batch;
  r.gz = g.batch;
  if (!cut && pipelined && (t128 >= 192 || t64 >= 192) && g.K + g.K2 >= 32) {
    auto even = [](int64_t v) { return (v & 1) == 0; };
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    r.vec = even(g.lda) && even(g.ldb) && even(g.sA) && even(g.sB) && al16(g.A) && al16(g.B) && (g.K2 == 0 || (al16(g.A2) && al16(g.B2)));
    const int bm = t128 >= 192 ? 128 : 64;
    r.kernel = bm == 128 ? HFMI_DGEMM_P128 : HFMI_DGEMM_P64;
    r.gx = (g.M + bm - 1) / bm;
    r.gy = (g.N + 127) / 128;
    return r;
  }
  r.kernel = cut ? HFMI_DGEMM_K64_CUT : HFMI_DGEMM_K64;
  r.gx = (g.M + 63) / 64;
  r.gy = (g.N + 63) / 64;
  return r;
}
int dgemm_pipelined_switch();      // HFMI_EIG_GEMM, read once per process
