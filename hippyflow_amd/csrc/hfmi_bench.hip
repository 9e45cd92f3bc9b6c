// Micro-benchmarks of libhfmi.so (include/hfmi.h) behind bench.py and the parity tests: the peak kernels that measure the roofline
// denominators in the same job, and the entry points that time or replay single contractions.
#include <string.h>

#include "hfmi_dgemm.h"
#include "hfmi_internal.h"

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ micro-benchmarks (roofline denominators)
__global__ __launch_bounds__(256, 2) void k_bench_mfma(double* out, int iters) {
  d4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (s == 123.456) out[0] = s;
}
__global__ __launch_bounds__(256, 2) void k_bench_fma(double* out, int iters) {
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = threadIdx.x * 1e-9 + i;
  const double a = 1.0000001, b = 1e-9;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = fma(acc[i], a, b);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += acc[i];
  if (s == 123.456) out[0] = s;
}
__global__ void k_bench_copy(const d2* __restrict__ src, d2* __restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
int launch_bench_peaks(hfmi_ctx* ctx, double* mfma_tflops, double* fma_tflops, double* copy_gbs) {
  void* buf = nullptr;
  const size_t bytes = (size_t)2 << 30;  // 1 GiB read + 1 GiB write per copy
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, bytes, &buf));
  double* out = (double*)buf;
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  float ms = 0.f;
  // fp64 MFMA: 4 waves/CU (one per SIMD) x 8 independent accumulators
  const int it1 = 2000, g1 = cus * 16;
  hipLaunchKernelGGL(k_bench_mfma, dim3(g1), dim3(256), 0, ctx->stream, out, 100);
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(k_bench_mfma, dim3(g1), dim3(256), 0, ctx->stream, out, it1);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *mfma_tflops = (double)g1 * 4 * it1 * 8 * (2.0 * 16 * 16 * 4) / (ms * 1e-3) / 1e12;
  // fp64 vector FMA: 8 waves/CU x 16 independent chains
  const int it2 = 2000, g2 = cus * 32;
  hipLaunchKernelGGL(k_bench_fma, dim3(g2), dim3(256), 0, ctx->stream, out, 100);
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  hipLaunchKernelGGL(k_bench_fma, dim3(g2), dim3(256), 0, ctx->stream, out, it2);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *fma_tflops = (double)g2 * 256 * it2 * 16 * 2.0 / (ms * 1e-3) / 1e12;
  // HBM copy
  const int64_t n = (int64_t)(bytes / 2 / sizeof(d2));
  d2* src = (d2*)buf;
  d2* dst = src + n;
  hipLaunchKernelGGL(k_bench_copy, dim3(cus * 8), dim3(256), 0, ctx->stream, src, dst, n);
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int rep = 0; rep < 5; ++rep) hipLaunchKernelGGL(k_bench_copy, dim3(cus * 8), dim3(256), 0, ctx->stream, src, dst, n);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *copy_gbs = 5.0 * (double)bytes / (ms * 1e-3) / 1e9;
  return HFMI_OK;
}

// The same loop on FULL-MANTISSA operands: every lane holds eight Gaussian values per operand, and each MFMA of an iteration takes
// another pair of them (the register pairs rotate through the eight accumulators), so operand and accumulator bits toggle like
// those of the solve's contractions on Gaussian data.  The constant-operand loop above multiplies 1 +- tid 1e-9: almost no
// toggling, a clock (2.35-2.40 GHz) that random data does not see under the power limit (MI355X_MICROARCH.md, "DVFS give-back").
__global__ __launch_bounds__(256, 2) void k_bench_mfma_rand(const double* __restrict__ vals, double* out, int iters) {
  d4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  double a[8], b[8];
  const double* src = vals + ((size_t)blockIdx.x % 64) * 4096 + threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = src[256 * i];
    b[i] = src[256 * (8 + i)];
  }
  for (int it = 0; it < iters; it += 8) {
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(i + r) & 7], b[(i + 3 * r) & 7], acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (s == 123.456) out[0] = s;
}
__global__ void k_bench_copy_loop(const d2* __restrict__ src, d2* __restrict__ dst, int64_t n, int reps) {
  for (int rep = 0; rep < reps; ++rep)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
      __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}
// The fp64 MFMA rate this box sustains WHILE HBM is being streamed: the constant-operand MFMA loop on the context's stream with
// the copy kernel running beside it on the auxiliary stream (two workgroups per CU, ~3 TB/s).  The big contractions of the
// solve run in exactly that regime (their clock is set by the power limit), so this, not the cold
// micro-benchmark, is the in-job ceiling their fraction should be read against.
int launch_bench_loaded_peak(hfmi_ctx* ctx, double* mfma_tflops, double* copy_gbs) {
  void* buf = nullptr;
  const size_t bytes = (size_t)2 << 30;
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, bytes + 4096, &buf));
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const int64_t n = (int64_t)(bytes / 2 / sizeof(d2));
  d2* src = (d2*)buf;
  d2* dst = src + n;
  double* out = (double*)(dst + n);
  hip_event c0, c1;
  OWN_TRY(c0.create());
  OWN_TRY(c1.create());
  const int it1 = 2000, g1 = cus * 16, copies = 24, reps = 3;
  hipLaunchKernelGGL(k_bench_mfma, dim3(g1), dim3(256), 0, ctx->stream, out, 100);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipEventRecord(c0, ctx->aux_stream));
  // ONE resident launch (its workgroups keep their slots beside the MFMA waves), four workgroups per CU
  hipLaunchKernelGGL(k_bench_copy_loop, dim3(cus * 4), dim3(256), 0, ctx->aux_stream, src, dst, n, copies);
  HIP_TRY(hipEventRecord(c1, ctx->aux_stream));
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int rep = 0; rep < reps; ++rep) hipLaunchKernelGGL(k_bench_mfma, dim3(g1), dim3(256), 0, ctx->stream, out, it1);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventSynchronize(c1));
  float ms = 0.f, msc = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&msc, c0, c1));
  *mfma_tflops = (double)reps * g1 * 4 * it1 * 8 * (2.0 * 16 * 16 * 4) / (ms * 1e-3) / 1e12;
  *copy_gbs = (double)copies * (double)bytes / (msc * 1e-3) / 1e9;   // over the whole copy window (part of it runs alone)
  return HFMI_OK;
}

// read-only stream: what a contraction that only READS its big operand can get from HBM (the copy above also writes)
__global__ __launch_bounds__(256) void k_bench_read(const d2* __restrict__ src, double* out, int64_t n) {
  double s = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256 * 8;
  for (int64_t i = (int64_t)blockIdx.x * 256 * 8 + threadIdx.x; i + 7 * 256 < n; i += stride) {
    d2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[i + 256 * u];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u].x + v[u].y;
  }
  if (s == 123.456) out[0] = s;
}
int launch_bench_read(hfmi_ctx* ctx, double* read_gbs) {
  void* buf = nullptr;
  const size_t bytes = (size_t)2 << 30;
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, bytes + 4096, &buf));
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const int64_t n = (int64_t)(bytes / sizeof(d2));
  double* out = (double*)((char*)buf + bytes);
  float ms = 0.f;
  hipLaunchKernelGGL(k_bench_read, dim3(cus * 8), dim3(256), 0, ctx->stream, (const d2*)buf, out, n);
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int rep = 0; rep < 5; ++rep) hipLaunchKernelGGL(k_bench_read, dim3(cus * 8), dim3(256), 0, ctx->stream, (const d2*)buf, out, n);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *read_gbs = 5.0 * (double)bytes / (ms * 1e-3) / 1e9;
  return HFMI_OK;
}

// fp64 MFMA rate on Gaussian operands: alone, and with the copy kernel streaming HBM beside it (the regime of the solve's big
// contractions) -- the denominators bench.py reports as roofline.frac_of_in_job_random_operand_peak[_while_streaming]
int launch_bench_random_peaks(hfmi_ctx* ctx, double* mfma_tflops, double* mfma_tflops_streaming, double* copy_gbs) {
  void* buf = nullptr;
  const size_t bytes = (size_t)2 << 30;
  const size_t nvals = (size_t)64 * 4096;
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, bytes + 4096 + nvals * sizeof(double), &buf));
  const int cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
  const int64_t n = (int64_t)(bytes / 2 / sizeof(d2));
  d2* src = (d2*)buf;
  d2* dst = src + n;
  double* out = (double*)(dst + n);
  double* vals = out + 512;
  HFMI_TRY(launch_randn(ctx, vals, (int64_t)nvals, 1, (int64_t)nvals, 0x5eedULL, 7u, 1.0));
  const int it1 = 2000, g1 = cus * 16, copies = 24, reps = 3;
  float ms = 0.f, msc = 0.f;
  hipLaunchKernelGGL(k_bench_mfma_rand, dim3(g1), dim3(256), 0, ctx->stream, vals, out, 104);
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int rep = 0; rep < reps; ++rep) hipLaunchKernelGGL(k_bench_mfma_rand, dim3(g1), dim3(256), 0, ctx->stream, vals, out, it1);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *mfma_tflops = (double)reps * g1 * 4 * it1 * 8 * (2.0 * 16 * 16 * 4) / (ms * 1e-3) / 1e12;
  hip_event c0, c1;
  OWN_TRY(c0.create());
  OWN_TRY(c1.create());
  HIP_TRY(hipEventRecord(c0, ctx->aux_stream));
  hipLaunchKernelGGL(k_bench_copy_loop, dim3(cus * 4), dim3(256), 0, ctx->aux_stream, src, dst, n, copies);
  HIP_TRY(hipEventRecord(c1, ctx->aux_stream));
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int rep = 0; rep < reps; ++rep) hipLaunchKernelGGL(k_bench_mfma_rand, dim3(g1), dim3(256), 0, ctx->stream, vals, out, it1);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventSynchronize(c1));
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  HIP_TRY(hipEventElapsedTime(&msc, c0, c1));
  *mfma_tflops_streaming = (double)reps * g1 * 4 * it1 * 8 * (2.0 * 16 * 16 * 4) / (ms * 1e-3) / 1e12;
  *copy_gbs = (double)copies * (double)bytes / (msc * 1e-3) / 1e9;
  return HFMI_OK;
}

// ------------------------------------------------------------------ entry points

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
static void dgemm_route_words(const gemm_route& r, int* route) {
  const int w[HFMI_DGEMM_ROUTE_WORDS] = {r.kernel, r.vec, r.gx, r.gy, r.gz, r.error, 0, 0};
  memcpy(route, w, sizeof(w));
}
// the route launch_dgemm would take, from the function it calls (hfmi_dgemm.h); no device involved.  The pointers of the descriptor
// carry the alignments only and are never dereferenced.
extern "C" int hfmi_dgemm_route_predict(int M, int N, int K, int K2, int batch, int ta, int tb, int64_t lda, int64_t ldb, int64_t sA, int64_t sB,
                                        int align_A, int align_B, int align_A2, int align_B2, int cut, int has_skip, int pipelined, int* route) {
  if (!route) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  static const int flag = 0;
  auto at = [](int align) { return (const double*)(uintptr_t)(4096 + (align & 15)); };
  gemm_desc g;
  g.ta = ta != 0;
  g.tb = tb != 0;
  g.M = M;
  g.N = N;
  g.K = K;
  g.alpha = 1.0;
  g.beta = 0.0;
  g.A = at(align_A);
  g.B = at(align_B);
  g.lda = lda;
  g.ldb = ldb;
  g.C = nullptr;
  g.ldc = M;
  g.K2 = K2;
  g.A2 = at(align_A2);
  g.B2 = at(align_B2);
  g.batch = batch;
  g.sA = sA;
  g.sB = sB;
  g.cut = cut;
  g.skip = has_skip ? &flag : nullptr;
  dgemm_route_words(dgemm_route_make(g, pipelined), route);
  return HFMI_OK;
}
// launch_dgemm with its whole descriptor on device copies of the caller's arrays (the descriptor sweep of the tests)
extern "C" int hfmi_test_dgemm(hfmi_ctx* ctx, const int64_t* dims, double alpha, double beta, const double* host_A, const double* host_B,
                               const double* host_A2, const double* host_B2, double* host_C, int* route, int* launch_status) {
  if (!ctx || !dims || !host_A || !host_B || !host_C || !route || !launch_status) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  const int64_t* d = dims;
  const bool ta = d[0] != 0, tb = d[1] != 0;
  const int64_t M = d[2], N = d[3], K = d[4], K2 = d[5], batch = d[6], lda = d[7], ldb = d[8], ldc = d[9], sA = d[10], sB = d[11], sC = d[12];
  const int64_t skip_mode = d[15];
  const int64_t n[5] = {d[16], d[18], d[20], d[22], d[24]}, off[5] = {d[17], d[19], d[21], d[23], d[25]};
  const double* host[5] = {host_A, host_B, host_A2, host_B2, host_C};
  for (int i = 0; i < HFMI_TEST_DGEMM_DIMS; ++i)
    if (d[i] < 0 || d[i] > ((int64_t)1 << 40)) HFMI_FAIL(HFMI_ERR_INVALID, "test_dgemm: dims[%d] = %lld out of range", i, (long long)d[i]);
  if (M > 0x7fffffff || N > 0x7fffffff || K > 0x7fffffff || K2 > 0x7fffffff || batch < 1 || batch > 65535 || skip_mode > 2 || n[4] < 1)
    HFMI_FAIL(HFMI_ERR_INVALID, "test_dgemm: bad shape");
  if ((n[2] > 0 && !host_A2) || (n[3] > 0 && !host_B2)) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  // buffer sizes: the last element a kernel may touch of an operand of `rows` x `cols` (every batch member) lies inside its array
  auto fits = [&](int64_t rows, int64_t cols, int64_t ld, int64_t stride, int which) {
    if (rows <= 0 || cols <= 0) return off[which] <= n[which];
    const double last = (double)off[which] + (double)(batch - 1) * (double)stride + (double)(cols - 1) * (double)ld + (double)rows;
    return last <= (double)n[which];
  };
  const bool okA = fits(ta ? K : M, ta ? M : K, lda, sA, 0), okB = fits(tb ? N : K, tb ? K : N, ldb, sB, 1);
  const bool okA2 = K2 == 0 || fits(ta ? K2 : M, ta ? M : K2, lda, sA, 2), okB2 = K2 == 0 || fits(tb ? N : K2, tb ? K2 : N, ldb, sB, 3);
  if (!okA || !okB || !okA2 || !okB2 || !fits(M, N, ldc, sC, 4)) HFMI_FAIL(HFMI_ERR_INVALID, "test_dgemm: an operand does not fit its array");
  HIP_TRY(hipSetDevice(ctx->device));
  // one allocation: the five arrays on 16-byte boundaries, the flag behind them
  int64_t base[6], total = 0;
  for (int i = 0; i < 5; ++i) {
    base[i] = total;
    total += round_up(n[i], 2);
  }
  base[5] = total;
  void* wv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)(total + 2) * sizeof(double), &wv));
  double* dev = (double*)wv;
  hipStream_t st = ctx->stream;
  for (int i = 0; i < 5; ++i)
    if (n[i] > 0) HIP_TRY(hipMemcpyAsync(dev + base[i], host[i], (size_t)n[i] * sizeof(double), hipMemcpyHostToDevice, st));
  int* flag = (int*)(dev + base[5]);
  const int up = skip_mode == 2 ? 1 : 0;
  HIP_TRY(hipMemcpyAsync(flag, &up, sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));       // (`up` is a local)
  gemm_desc g;
  g.ta = ta;
  g.tb = tb;
  g.M = (int)M;
  g.N = (int)N;
  g.K = (int)K;
  g.alpha = alpha;
  g.beta = beta;
  g.A = dev + base[0] + off[0];
  g.B = dev + base[1] + off[1];
  g.lda = lda;
  g.ldb = ldb;
  g.C = dev + base[4] + off[4];
  g.ldc = ldc;
  g.K2 = (int)K2;
  g.A2 = n[2] > 0 ? dev + base[2] + off[2] : nullptr;
  g.B2 = n[3] > 0 ? dev + base[3] + off[3] : nullptr;
  g.batch = (int)batch;
  g.sA = sA;
  g.sB = sB;
  g.sC = sC;
  g.lower = (int)d[13];
  g.cut = (int)d[14];
  g.skip = skip_mode ? flag : nullptr;
  dgemm_route_words(dgemm_route_make(g, dgemm_pipelined_switch()), route);
  *launch_status = launch_dgemm(ctx, g);
  return read_back(ctx, dev + base[4], (size_t)n[4], host_C);
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
