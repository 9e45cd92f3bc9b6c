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
