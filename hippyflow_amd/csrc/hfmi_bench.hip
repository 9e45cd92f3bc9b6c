// Micro-benchmark entry points of libhfmi.so (include/hfmi.h) behind bench.py and the parity tests.  Host side only.
#include <string.h>

#include "hfmi_internal.h"

extern "C" int hfmi_bench_tsgemm_tn(const hfmi_block* A, const hfmi_block* B, int nsplit, int reps, double* host_C, double* avg_ms) {
  if (!A || !B) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->N != B->N) HFMI_FAIL(HFMI_ERR_INVALID, "bench_tsgemm_tn: vector lengths differ");
  hfmi_ctx* ctx = A->ctx;
  void* out = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)A->nvec * round_up(B->nvec, 16) * sizeof(double), &out));
  const int ldc = (int)round_up(B->nvec, 16);
  HFMI_TRY(launch_tsgemm_tn(ctx, A->p, A->ld, A->nvec, B->p, B->ld, B->nvec, A->N, 1.0, 0.0, (double*)out, ldc, 1, nsplit));
  if (reps > 0) {
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < reps; ++i)
      HFMI_TRY(launch_tsgemm_tn(ctx, A->p, A->ld, A->nvec, B->p, B->ld, B->nvec, A->N, 1.0, 0.0, (double*)out, ldc, 1, nsplit));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (avg_ms) *avg_ms = ms / reps;
  }
  if (host_C) {
    std::vector<double> tmp((size_t)A->nvec * ldc);
    HFMI_TRY(read_back(ctx, (const double*)out, tmp.size(), tmp.data()));
    for (int i = 0; i < A->nvec; ++i) memcpy(host_C + (size_t)i * B->nvec, tmp.data() + (size_t)i * ldc, (size_t)B->nvec * sizeof(double));
  }
  return HFMI_OK;
}
// launch_tsgemm_tn with its whole argument list on a device copy of the caller's array (the instance sweep of the tests)
extern "C" int hfmi_test_tsgemm_tn(const hfmi_block* A, const hfmi_block* B, double scale, double beta, int colmajor, int ldc, int nsplit,
                                   double* host_C) {
  if (!A || !B || !host_C) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->N != B->N) HFMI_FAIL(HFMI_ERR_INVALID, "test_tsgemm_tn: vector lengths differ");
  if (A->ctx != B->ctx) HFMI_FAIL(HFMI_ERR_INVALID, "test_tsgemm_tn: blocks of different contexts");
  const int m = A->nvec, k = B->nvec;
  const int fast = colmajor ? m : k, slow = colmajor ? k : m;
  if (ldc < fast || (colmajor && ldc == 1)) HFMI_FAIL(HFMI_ERR_INVALID, "test_tsgemm_tn: ldc %d too small for %d x %d", ldc, m, k);
  if (nsplit < 0) HFMI_FAIL(HFMI_ERR_INVALID, "test_tsgemm_tn: negative split count");
  hfmi_ctx* ctx = A->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t count = (size_t)slow * ldc;
  void* dev = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, count * sizeof(double), &dev));
  HIP_TRY(hipMemcpyAsync(dev, host_C, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HFMI_TRY(launch_tsgemm_tn(ctx, A->p, A->ld, m, B->p, B->ld, k, A->N, scale, beta, (double*)dev, colmajor ? 1 : ldc, colmajor ? ldc : 1,
                            nsplit));
  return read_back(ctx, (const double*)dev, count, host_C);
}
extern "C" int hfmi_bench_tsgemm_nn(const hfmi_block* A, const double* host_S, hfmi_block* Y, int reps, double* avg_ms) {
  if (!A || !host_S || !Y) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = A->ctx;
  const int m = A->nvec, r = Y->nvec;
  const int ld = (int)round_up(r, 16);
  void* S = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)m * ld * sizeof(double), &S));
  HFMI_TRY(upload_small(ctx, host_S, m, r, (double*)S, ld));
  HFMI_TRY(launch_tsgemm_nn(ctx, A->p, A->ld, m, (const double*)S, ld, r, 1.0, 0.0, Y->p, Y->ld, A->N));
  if (reps > 0) {
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < reps; ++i)
      HFMI_TRY(launch_tsgemm_nn(ctx, A->p, A->ld, m, (const double*)S, ld, r, 1.0, 0.0, Y->p, Y->ld, A->N));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (avg_ms) *avg_ms = ms / reps;
  }
  return HFMI_OK;
}
extern "C" int hfmi_bench_peaks(hfmi_ctx* ctx, double* mfma_f64_tflops, double* fma_f64_tflops, double* hbm_copy_gbs) {
  if (!ctx || !mfma_f64_tflops || !fma_f64_tflops || !hbm_copy_gbs) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_bench_peaks(ctx, mfma_f64_tflops, fma_f64_tflops, hbm_copy_gbs);
}
extern "C" int hfmi_bench_loaded_peak(hfmi_ctx* ctx, double* mfma_f64_tflops, double* hbm_copy_gbs) {
  if (!ctx || !mfma_f64_tflops || !hbm_copy_gbs) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_bench_loaded_peak(ctx, mfma_f64_tflops, hbm_copy_gbs);
}
// C (M x N) = op(A) op(B) on the device's general fp64 MFMA product (hfmi_dgemm.hip), host column-major operands in and out: the two
// N x N x N congruence products of the deterministic POD's N-dimensional route (PODProjector.py:812-833 when there are more snapshots
// than the n x n eigensolver takes and the state dimension is the small one: S = B^T (X^T X) B with M = B B^T)
extern "C" int hfmi_dense_matmul(hfmi_ctx* ctx, int M, int N, int K, int ta, int tb, const double* host_A, const double* host_B, double* host_C) {
  if (!ctx || !host_A || !host_B || !host_C) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (M < 1 || N < 1 || K < 1) HFMI_FAIL(HFMI_ERR_INVALID, "dense_matmul: bad shape %d x %d x %d", M, N, K);
  HIP_TRY(hipSetDevice(ctx->device));
  return eig_dgemm_bench(ctx, M, N, K, ta, tb, 0, host_A, host_B, host_C, nullptr);
}
extern "C" int hfmi_bench_dgemm(hfmi_ctx* ctx, int M, int N, int K, int ta, int tb, int reps, const double* host_A, const double* host_B,
                                double* host_C, double* avg_ms) {
  if (!ctx || !host_A || !host_B) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (M < 1 || N < 1 || K < 1 || reps < 0) HFMI_FAIL(HFMI_ERR_INVALID, "bench_dgemm: bad shape %d x %d x %d", M, N, K);
  HIP_TRY(hipSetDevice(ctx->device));
  return eig_dgemm_bench(ctx, M, N, K, ta, tb, reps, host_A, host_B, host_C, avg_ms);
}
extern "C" int hfmi_bench_hbm_read(hfmi_ctx* ctx, double* hbm_read_gbs) {
  if (!ctx || !hbm_read_gbs) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_bench_read(ctx, hbm_read_gbs);
}
extern "C" int hfmi_bench_random_peaks(hfmi_ctx* ctx, double* mfma_f64_tflops, double* mfma_f64_tflops_while_streaming, double* hbm_copy_gbs) {
  if (!ctx || !mfma_f64_tflops || !mfma_f64_tflops_while_streaming || !hbm_copy_gbs) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_bench_random_peaks(ctx, mfma_f64_tflops, mfma_f64_tflops_while_streaming, hbm_copy_gbs);
}
