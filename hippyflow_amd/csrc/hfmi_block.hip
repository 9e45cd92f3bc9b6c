// Blocks (hippylib's MultiVector) and CSR matrices of libhfmi.so (include/hfmi.h): creation, views, host <-> device
// transfers, the streaming ingest ring and the elementwise / small-product entry points.  Host side only; kernels live in
// hfmi_misc.hip / hfmi_gemm.hip / hfmi_gemm_nn.hip.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "hfmi_internal.h"

// ------------------------------------------------------------------ blocks
extern "C" int hfmi_block_create(hfmi_ctx* ctx, int64_t N, int nvec, hfmi_block** out) {
  if (!ctx || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  hfmi_block* b = nullptr;
  HFMI_TRY(block_alloc(ctx, N, nvec, &b));
  hipError_t e = hipMemsetAsync(b->p, 0, (size_t)b->ld * nvec * sizeof(double), ctx->stream);
  if (e != hipSuccess) {
    (void)hfmi_block_destroy(b);
    HFMI_FAIL(HFMI_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
  }
  *out = b;
  return HFMI_OK;
}
extern "C" int hfmi_block_wrap(hfmi_ctx* ctx, double* dptr, int64_t N, int nvec, int64_t ld, hfmi_block** out) {
  if (!ctx || !out || !dptr) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (N <= 0 || nvec <= 0) HFMI_FAIL(HFMI_ERR_INVALID, "block_wrap: N and nvec must be positive");
  if (ld % 32 != 0 || ld < N) HFMI_FAIL(HFMI_ERR_INVALID, "block_wrap: ld=%lld must be a multiple of 32 and >= N", (long long)ld);
  if (((uintptr_t)dptr) % 128 != 0) HFMI_FAIL(HFMI_ERR_INVALID, "block_wrap: pointer must be 128-byte aligned");
  hfmi_block* b = new (std::nothrow) hfmi_block();
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  b->ctx = ctx;
  b->p = dptr;
  b->N = N;
  b->nvec = nvec;
  b->ld = ld;
  b->owner = false;
  int s = launch_zero_pad(ctx, dptr, N, nvec, ld);
  if (s != HFMI_OK) {
    delete b;
    return s;
  }
  *out = b;
  return HFMI_OK;
}
extern "C" int hfmi_block_view(hfmi_block* parent, int first, int count, hfmi_block** out) {
  if (!parent || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (first < 0 || count <= 0 || first + count > parent->nvec)
    HFMI_FAIL(HFMI_ERR_INVALID, "block_view: [%d,%d) outside [0,%d)", first, first + count, parent->nvec);
  hfmi_block* b = new (std::nothrow) hfmi_block(*parent);
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  b->p = parent->p + (int64_t)first * parent->ld;
  b->nvec = count;
  b->owner = false;
  *out = b;
  return HFMI_OK;
}
extern "C" int hfmi_block_destroy(hfmi_block* b) {
  if (!b) return HFMI_OK;
  if (b->owner && b->p) {
    (void)hipSetDevice(b->ctx->device);
    pool_release(b->ctx, b->p, (size_t)b->ld * b->nvec * sizeof(double));
  }
  delete b;
  return HFMI_OK;
}
extern "C" int hfmi_block_info(const hfmi_block* b, int64_t* N, int* nvec, int64_t* ld, double** dptr) {
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  if (N) *N = b->N;
  if (nvec) *nvec = b->nvec;
  if (ld) *ld = b->ld;
  if (dptr) *dptr = b->p;
  return HFMI_OK;
}

int check_same_shape(const hfmi_block* a, const hfmi_block* b, const char* what) {
  if (!a || !b) HFMI_FAIL(HFMI_ERR_INVALID, "%s: null block", what);
  if (a->N != b->N || a->nvec != b->nvec)
    HFMI_FAIL(HFMI_ERR_INVALID, "%s: x and y have non-matching shapes (%lld x %d vs %lld x %d)", what, (long long)a->N,
              a->nvec, (long long)b->N, b->nvec);
  return HFMI_OK;
}

extern "C" int hfmi_block_upload(hfmi_block* b, const double* host, int layout) {
  if (!b || !host) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = b->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  if (layout == HFMI_LAYOUT_VECTORS) {
    HIP_TRY(hipMemcpy2DAsync(b->p, (size_t)b->ld * sizeof(double), host, (size_t)b->N * sizeof(double),
                             (size_t)b->N * sizeof(double), (size_t)b->nvec, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  } else if (layout == HFMI_LAYOUT_DENSE) {
    // stage in slabs of rows so that the staging buffer stays bounded
    const int64_t rows_per = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)b->nvec * 8));
    void* stage = nullptr;
    HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)std::min<int64_t>(rows_per, b->N) * b->nvec * sizeof(double), &stage));
    for (int64_t t0 = 0; t0 < b->N; t0 += rows_per) {
      const int64_t rows = std::min<int64_t>(rows_per, b->N - t0);
      HIP_TRY(hipMemcpyAsync(stage, host + t0 * b->nvec, (size_t)rows * b->nvec * sizeof(double), hipMemcpyHostToDevice,
                             ctx->stream));
      HFMI_TRY(launch_dense_to_block(ctx, (const double*)stage, b->p + t0, b->ld, rows, b->nvec));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  } else {
    HFMI_FAIL(HFMI_ERR_INVALID, "block_upload: unknown layout %d", layout);
  }
  return HFMI_OK;
}
// ------------------------------------------------------------------ streaming ingest (PODProjector.py:343-357,
// activeSubspaceProjector.py:178-221: the reference fills its blocks sample by sample from host PDE solves)
// A host producer appends sample i + 1 while sample i's contraction runs: the copy is enqueued on the context's INGEST stream
// from pinned memory (hfmi_host_alloc_pinned) and returns at once with a ticket; hfmi_ingest_wait(ticket) tells the producer
// when that pinned buffer may be overwritten; hfmi_ingest_fence makes the compute stream wait (on the device, the host is
// not blocked) for everything uploaded so far.
extern "C" int hfmi_host_alloc_pinned(size_t bytes, void** out) {
  if (!out || bytes == 0) HFMI_FAIL(HFMI_ERR_INVALID, "host_alloc_pinned: bad argument");
  void* p = nullptr;
  OWN_TRY(own_acquire(OWN_PINNED, bytes, &p));
  *out = p;      // the caller's from here: counted, but no owner object
  return HFMI_OK;
}
extern "C" int hfmi_host_free_pinned(void* p) {
  own_release(OWN_PINNED, p);
  return HFMI_OK;
}
extern "C" int hfmi_block_upload_async(hfmi_block* b, const double* host_pinned, int layout, int64_t* ticket) {
  if (!b || !host_pinned) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = b->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->ingest_stream) {      // the ring first: the stream is what says that both exist
    for (hip_event& e : ctx->ev_ingest) OWN_TRY(e.create(hipEventDisableTiming));
    OWN_TRY(ctx->ingest_stream.create(hipStreamNonBlocking));
  }
  // the block may still be read by work queued on the compute stream (a view that is being refilled): order behind it
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->ingest_stream, ctx->ev_status, 0));
  const int slot = (int)(ctx->ingest_seq % HFMI_INGEST_RING);
  if (ctx->ingest_seq >= HFMI_INGEST_RING) HIP_TRY(hipEventSynchronize(ctx->ev_ingest[slot]));   // ring of tickets: the oldest must be done
  if (layout == HFMI_LAYOUT_VECTORS) {
    // one vector per host row: straight into the block's columns, no staging, no conversion kernel
    HIP_TRY(hipMemcpy2DAsync(b->p, (size_t)b->ld * sizeof(double), host_pinned, (size_t)b->N * sizeof(double),
                             (size_t)b->N * sizeof(double), (size_t)b->nvec, hipMemcpyHostToDevice, ctx->ingest_stream));
    HIP_TRY(hipEventRecord(ctx->ev_ingest[slot], ctx->ingest_stream));
  } else if (layout == HFMI_LAYOUT_DENSE) {
    void* stage = nullptr;
    HFMI_TRY(ctx_ws(ctx, WS_INGEST, (size_t)b->N * b->nvec * sizeof(double), &stage));
    HIP_TRY(hipMemcpyAsync(stage, host_pinned, (size_t)b->N * b->nvec * sizeof(double), hipMemcpyHostToDevice, ctx->ingest_stream));
    HIP_TRY(hipEventRecord(ctx->ev_ingest[slot], ctx->ingest_stream));     // the pinned buffer is free from here
    auto saved = std::move(ctx->stream);                                    // the launchers enqueue on ctx->stream
    ctx->stream.borrow(ctx->ingest_stream);
    const int s = launch_dense_to_block(ctx, (const double*)stage, b->p, b->ld, b->N, b->nvec);
    ctx->stream = std::move(saved);
    if (s != HFMI_OK) return s;
  } else {
    HFMI_FAIL(HFMI_ERR_INVALID, "block_upload_async: unknown layout %d", layout);
  }
  if (ticket) *ticket = ctx->ingest_seq;
  ++ctx->ingest_seq;
  return HFMI_OK;
}
extern "C" int hfmi_ingest_wait(hfmi_ctx* ctx, int64_t ticket) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  if (ticket < 0 || ticket >= ctx->ingest_seq) HFMI_FAIL(HFMI_ERR_INVALID, "ingest_wait: no upload with ticket %lld", (long long)ticket);
  if (ctx->ingest_seq - ticket > HFMI_INGEST_RING) return HFMI_OK;          // waited for when its ring slot was reused
  HIP_TRY(hipEventSynchronize(ctx->ev_ingest[ticket % HFMI_INGEST_RING]));
  return HFMI_OK;
}
extern "C" int hfmi_ingest_fence(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  if (!ctx->ingest_stream) return HFMI_OK;
  HIP_TRY(hipEventRecord(ctx->ev_join, ctx->ingest_stream));
  HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  return HFMI_OK;
}

extern "C" int hfmi_block_download(const hfmi_block* b, double* host, int layout) {
  if (!b || !host) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = b->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  if (layout == HFMI_LAYOUT_VECTORS) {
    HIP_TRY(hipMemcpy2DAsync(host, (size_t)b->N * sizeof(double), b->p, (size_t)b->ld * sizeof(double),
                             (size_t)b->N * sizeof(double), (size_t)b->nvec, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  } else if (layout == HFMI_LAYOUT_DENSE) {
    const int64_t rows_per = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)b->nvec * 8));
    void* stage = nullptr;
    HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)std::min<int64_t>(rows_per, b->N) * b->nvec * sizeof(double), &stage));
    for (int64_t t0 = 0; t0 < b->N; t0 += rows_per) {
      const int64_t rows = std::min<int64_t>(rows_per, b->N - t0);
      HFMI_TRY(launch_block_to_dense(ctx, b->p + t0, b->ld, (double*)stage, rows, b->nvec));
      HIP_TRY(hipMemcpyAsync(host + t0 * b->nvec, stage, (size_t)rows * b->nvec * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  } else {
    HFMI_FAIL(HFMI_ERR_INVALID, "block_download: unknown layout %d", layout);
  }
  return ctx_check_comm(ctx);                 // the block may have come through a collective that gave up
}
extern "C" int hfmi_block_zero(hfmi_block* b) {
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  return launch_fill(b->ctx, b->p, b->N, b->nvec, b->ld, 0.0, true);
}
extern "C" int hfmi_block_copy(hfmi_block* dst, const hfmi_block* src) {
  HFMI_TRY(check_same_shape(dst, src, "block_copy"));
  return launch_copy(dst->ctx, dst->p, dst->ld, src->p, src->ld, src->N, src->nvec);
}
extern "C" int hfmi_block_scale(hfmi_block* b, double alpha) {
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  return launch_scale(b->ctx, b->p, b->ld, b->N, b->nvec, alpha);
}
extern "C" int hfmi_block_axpy(hfmi_block* y, double alpha, const hfmi_block* x) {
  HFMI_TRY(check_same_shape(y, x, "block_axpy"));
  return launch_axpy(y->ctx, y->p, y->ld, alpha, x->p, x->ld, x->N, x->nvec);
}

extern "C" int hfmi_block_norms(const hfmi_block* b, double* host_norms) {
  if (!b || !host_norms) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = b->ctx;
  void* out = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)b->nvec * sizeof(double), &out));
  HFMI_TRY(launch_col_dots(ctx, b->p, b->ld, b->p, b->ld, b->N, b->nvec, (double*)out));
  HFMI_TRY(read_back(ctx, (const double*)out, b->nvec, host_norms));
  for (int j = 0; j < b->nvec; ++j) host_norms[j] = sqrt(host_norms[j]);
  return HFMI_OK;
}

extern "C" int hfmi_randn_fill(hfmi_block* b, uint64_t seed, uint32_t stream, double sigma) {
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  return launch_randn(b->ctx, b->p, b->N, b->nvec, b->ld, seed, stream, sigma);
}
extern "C" int hfmi_block_fill_matern32(hfmi_block* C, int nx, int ny, double sigma, double ell) {
  if (!C) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  if (C->N != C->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "fill_matern32: the block must be square (%lld x %d)", (long long)C->N, C->nvec);
  if (nx < 2 || ny < 2 || (int64_t)nx * ny < C->N) HFMI_FAIL(HFMI_ERR_INVALID, "fill_matern32: a %d x %d grid has fewer than %lld nodes", nx, ny, (long long)C->N);
  if (!(ell > 0.0)) HFMI_FAIL(HFMI_ERR_INVALID, "fill_matern32: correlation length must be positive");
  return launch_matern32(C->ctx, C->p, C->N, C->nvec, C->ld, nx, ny, sigma, ell);
}
extern "C" int hfmi_philox_raw(hfmi_block* shape_of, uint64_t seed, uint32_t stream, uint32_t* host_out) {
  if (!shape_of || !host_out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = shape_of->ctx;
  const size_t words = (size_t)shape_of->nvec * ((shape_of->N + 3) / 4) * 4;
  void* dev = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_STAGE, words * sizeof(uint32_t), &dev));
  HFMI_TRY(launch_philox_raw(ctx, (uint32_t*)dev, shape_of->N, shape_of->nvec, seed, stream));
  HIP_TRY(hipMemcpyAsync(host_out, dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return HFMI_OK;
}

extern "C" int hfmi_block_dot(const hfmi_block* A, const hfmi_block* B, double* host_out) {
  if (!A || !B || !host_out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->N != B->N) HFMI_FAIL(HFMI_ERR_INVALID, "block_dot: vector lengths differ (%lld vs %lld)", (long long)A->N, (long long)B->N);
  hfmi_ctx* ctx = A->ctx;
  void* out = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)A->nvec * B->nvec * sizeof(double), &out));
  HFMI_TRY(launch_tsgemm_tn(ctx, A->p, A->ld, A->nvec, B->p, B->ld, B->nvec, A->N, 1.0, 0.0, (double*)out, B->nvec, 1, 0));
  return read_back(ctx, (const double*)out, (size_t)A->nvec * B->nvec, host_out);
}

// upload a host row-major (rows x cols) matrix into a device buffer with leading dimension ld (zero padded)
int upload_small(hfmi_ctx* ctx, const double* host, int rows, int cols, double* dev, int ld) {
  void* pin = nullptr;
  HFMI_TRY(ctx_pinned(ctx, (size_t)rows * ld * sizeof(double), &pin));
  double* p = (double*)pin;
  for (int i = 0; i < rows; ++i) {
    memcpy(p + (size_t)i * ld, host + (size_t)i * cols, (size_t)cols * sizeof(double));
    for (int j = cols; j < ld; ++j) p[(size_t)i * ld + j] = 0.0;
  }
  HIP_TRY(hipMemcpyAsync(dev, pin, (size_t)rows * ld * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the pinned buffer is reused
  return HFMI_OK;
}

extern "C" int hfmi_block_gemm_small(const hfmi_block* A, const double* host_S, double alpha, double beta, hfmi_block* Y) {
  if (!A || !host_S || !Y) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->N != Y->N) HFMI_FAIL(HFMI_ERR_INVALID, "block_gemm_small: vector lengths differ");
  hfmi_ctx* ctx = A->ctx;
  const int m = A->nvec, r = Y->nvec;
  const int ld = (int)round_up(r, 16);
  void* S = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)m * ld * sizeof(double), &S));
  HFMI_TRY(upload_small(ctx, host_S, m, r, (double*)S, ld));
  return launch_tsgemm_nn(ctx, A->p, A->ld, m, (const double*)S, ld, r, alpha, beta, Y->p, Y->ld, A->N);
}

// ------------------------------------------------------------------ CSR
extern "C" int hfmi_csr_create(hfmi_ctx* ctx, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* indptr,
                               const int32_t* indices, const double* data, hfmi_csr** out) {
  if (!ctx || !indptr || !indices || !data || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (nrows <= 0 || ncols <= 0 || nnz < 0 || indptr[0] != 0 || indptr[nrows] != nnz)
    HFMI_FAIL(HFMI_ERR_INVALID, "csr_create: inconsistent CSR arrays");
  for (int64_t z = 0; z < nnz; ++z)
    if (indices[z] < 0 || indices[z] >= ncols) HFMI_FAIL(HFMI_ERR_INVALID, "csr_create: column index out of range");
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<hfmi_csr> m(new (std::nothrow) hfmi_csr());      // nothing prepared, nothing estimated
  if (!m) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  m->ctx = ctx;
  m->nrows = nrows;
  m->ncols = ncols;
  m->nnz = nnz;
  if (nrows == ncols) {
    // Gershgorin bound on the spectrum of D^-1 A: max_i sum_j |a_ij| / a_ii (used by the Chebyshev solve; 0 = no bound: a
    // row without a positive diagonal entry)
    double g = 0.0;
    bool ok = true;
    for (int64_t i = 0; i < nrows && ok; ++i) {
      double dii = 0.0, sum = 0.0;
      for (int64_t z = indptr[i]; z < indptr[i + 1]; ++z) {
        if (indices[z] == i) dii += data[z];
        sum += fabs(data[z]);
      }
      if (!(dii > 0.0)) ok = false;
      else g = std::max(g, sum / dii);
    }
    m->solve.gersh_lmax = ok ? g : 0.0;
  }
  {
    // ELL image when the longest row is short and the padding stays below 1.5x (FEM mass / stiffness matrices)
    int64_t wmax = 0;
    for (int64_t i = 0; i < nrows; ++i) wmax = std::max(wmax, indptr[i + 1] - indptr[i]);
    if (wmax > 0 && wmax <= 64 && wmax * nrows <= nnz + nnz / 2 + 1024 && nrows < (int64_t)1 << 31) {
      std::vector<int32_t> ei((size_t)wmax * nrows);
      std::vector<double> ev((size_t)wmax * nrows);
      for (int64_t i = 0; i < nrows; ++i) {
        const int64_t b = indptr[i], e = indptr[i + 1];
        for (int64_t s = 0; s < wmax; ++s) {
          const bool in = b + s < e;
          ei[(size_t)s * nrows + i] = in ? indices[b + s] : (e > b ? indices[b] : 0);   // padding: a valid column, value 0
          ev[(size_t)s * nrows + i] = in ? data[b + s] : 0.0;
        }
      }
      OWN_TRY(m->ell_idx.alloc(ei.size()));
      OWN_TRY(m->ell_val.alloc(ev.size()));
      HIP_TRY(hipMemcpy(m->ell_idx, ei.data(), ei.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(m->ell_val, ev.data(), ev.size() * sizeof(double), hipMemcpyHostToDevice));
      m->ell_w = (int)wmax;
    }
  }
  OWN_TRY(m->indptr.alloc((size_t)(nrows + 1)));
  OWN_TRY(m->indices.alloc((size_t)std::max<int64_t>(nnz, 1)));
  OWN_TRY(m->data.alloc((size_t)std::max<int64_t>(nnz, 1)));
  HIP_TRY(hipMemcpy(m->indptr, indptr, (size_t)(nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->indices, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->data, data, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  *out = m.release();
  return HFMI_OK;
}
extern "C" int hfmi_csr_destroy(hfmi_csr* m) {
  if (m) (void)hipStreamSynchronize(m->ctx->stream);     // before the arrays go: a kernel may still read them
  delete m;
  return HFMI_OK;
}
