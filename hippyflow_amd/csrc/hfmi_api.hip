// C ABI of libhfmi.so (include/hfmi.h): object management, operator application, B-orthogonal QR,
// Rayleigh-Ritz and the fused double-pass solves.  Host-side orchestration only; kernels live in
// hfmi_gemm.hip / hfmi_misc.hip / hfmi_small.hip.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "hfmi_internal.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
void hfmi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* hfmi_last_error(void) { return g_err; }
extern "C" int hfmi_version(void) { return HFMI_VERSION; }
#ifndef HFMI_BUILD_TAG
#define HFMI_BUILD_TAG "untagged"
#endif
extern "C" const char* hfmi_build_tag(void) { return HFMI_BUILD_TAG; }

extern "C" int hfmi_device_count(int* count) {
  if (!count) HFMI_FAIL(HFMI_ERR_INVALID, "device_count: null argument");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return HFMI_OK;
}

// ------------------------------------------------------------------ context
// ------------------------------------------------------------------ device memory: pool of released block storage
static void pool_flush(hfmi_ctx* ctx) {
  if (ctx->pool.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& e : ctx->pool) (void)hipFree(e.p);
  ctx->pool.clear();
  ctx->pool_bytes = 0;
}
static hipError_t ctx_malloc(hfmi_ctx* ctx, void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess && !ctx->pool.empty()) {      // give the pooled storage back and try once more
    (void)hipGetLastError();
    pool_flush(ctx);
    e = hipMalloc(p, bytes);
  }
  return e;
}
// storage of a destroyed block: kept for reuse (same stream order as every other use of it) or freed
static void pool_release(hfmi_ctx* ctx, void* p, size_t bytes) {
  constexpr size_t MAX_ENTRY = (size_t)2 << 30, MAX_TOTAL = (size_t)8 << 30;
  if (bytes <= MAX_ENTRY && ctx->pool.size() < 16 && ctx->pool_bytes + bytes <= MAX_TOTAL) {
    ctx->pool.push_back({p, bytes});
    ctx->pool_bytes += bytes;
    return;
  }
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(p);
}
static void* pool_take(hfmi_ctx* ctx, size_t bytes) {
  for (size_t i = ctx->pool.size(); i-- > 0;)
    if (ctx->pool[i].bytes == bytes) {
      void* p = ctx->pool[i].p;
      ctx->pool_bytes -= bytes;
      ctx->pool.erase(ctx->pool.begin() + i);
      return p;
    }
  return nullptr;
}

void ctx_watch_comm(hfmi_ctx* ctx, hfmi_comm* c) {
  if (ctx && c) ctx->watched_comms.push_back(c);
}
void ctx_unwatch_comm(hfmi_ctx* ctx, hfmi_comm* c) {
  if (!ctx) return;
  for (size_t i = 0; i < ctx->watched_comms.size(); ++i)
    if (ctx->watched_comms[i] == c) {
      ctx->watched_comms.erase(ctx->watched_comms.begin() + i);
      return;
    }
}
// after a host synchronisation: did a stream-ordered collective behind it give up?  (one read of pinned host memory per
// communicator; no device call)
int ctx_check_comm(hfmi_ctx* ctx) {
  for (hfmi_comm* c : ctx->watched_comms) HFMI_TRY(comm_check_error(c));
  return HFMI_OK;
}

int ctx_ws(hfmi_ctx* ctx, int slot, size_t bytes, void** out) {
  if (bytes > ctx->ws_bytes[slot]) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // buffers other streams work in: the panel reductions' staging area (auxiliary stream), the ingest buffer
    if (slot == WS_COMM) HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
    if (slot == WS_INGEST) HIP_TRY(hipStreamSynchronize(ctx->ingest_stream));
    if (ctx->ws[slot]) HIP_TRY(hipFree(ctx->ws[slot]));
    ctx->ws[slot] = nullptr;
    ctx->ws_bytes[slot] = 0;
    size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(ctx_malloc(ctx, &ctx->ws[slot], want));
    ctx->ws_bytes[slot] = want;
  }
  *out = ctx->ws[slot];
  return HFMI_OK;
}
int ctx_pinned(hfmi_ctx* ctx, size_t bytes, void** out) {
  if (bytes > ctx->pinned_bytes) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->pinned) HIP_TRY(hipHostFree(ctx->pinned));
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
    HIP_TRY(hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault));
    ctx->pinned_bytes = bytes;
  }
  *out = ctx->pinned;
  return HFMI_OK;
}

extern "C" int hfmi_ctx_create(int device, hfmi_ctx** out) {
  if (!out) HFMI_FAIL(HFMI_ERR_INVALID, "ctx_create: null out");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    HFMI_FAIL(HFMI_ERR_NO_DEVICE, "no HIP device visible (libhfmi has no CPU path)");
  }
  if (device < 0 || device >= n) HFMI_FAIL(HFMI_ERR_INVALID, "ctx_create: device %d out of range [0,%d)", device, n);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  hfmi_ctx* c = new (std::nothrow) hfmi_ctx();
  if (!c) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  c->device = device;
  c->num_cus = prop.multiProcessorCount;
  c->lds_per_block = prop.sharedMemPerBlock;
  c->defl1_static_lds = 0;
  c->defl1_static_known = false;
  c->own_stream = true;
  c->compose_depth = 0;
  for (int i = 0; i < WS_NSLOTS; ++i) {
    c->ws[i] = nullptr;
    c->ws_bytes[i] = 0;
  }
  c->pinned = nullptr;
  c->pinned_bytes = 0;
  c->pinned_cb = nullptr;
  c->pinned_cb_bytes = 0;
  c->xfer = nullptr;
  c->pool_bytes = 0;
  for (int i = 0; i < HFMI_PHASE_COUNT; ++i) c->phase_ms[i] = 0.0;
  c->profiling = false;
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_status, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming));
  for (int i = 0; i < 4; ++i) HIP_TRY(hipEventCreateWithFlags(&c->ev_cb[i], hipEventDisableTiming));
  for (int i = 0; i < 8; ++i) HIP_TRY(hipEventCreateWithFlags(&c->ev_panel[i], hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  c->ingest_stream = nullptr;
  c->ingest_seq = 0;
  c->late_pinned = nullptr;
  c->nn_hook = nullptr;
  c->nn_hook_user = nullptr;
  c->nn_hook_panels = 0;
  c->nn_hook_called = false;
  c->nn_upper_hint = false;
  HIP_TRY(hipMalloc((void**)&c->small, (size_t)SM_NSLOTS * SM_MAXK * SM_LD * sizeof(double)));
  HIP_TRY(hipMemsetAsync(c->small, 0, (size_t)SM_NSLOTS * SM_MAXK * SM_LD * sizeof(double), c->stream));
  HIP_TRY(hipMalloc((void**)&c->status_dev, 2 * sizeof(hfmi_status_words)));      // [1]: a factorisation taken on trust (qr_chol)
  HIP_TRY(hipMemsetAsync(c->status_dev, 0, 2 * sizeof(hfmi_status_words), c->stream));
  HIP_TRY(hipHostMalloc((void**)&c->status_host, sizeof(hfmi_status_words), hipHostMallocDefault));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = c;
  return HFMI_OK;
}

extern "C" int hfmi_ctx_destroy(hfmi_ctx* ctx) {
  if (!ctx) return HFMI_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (hfmi_comm* c : ctx->watched_comms) comm_forget_ctx(c);    // a communicator destroyed after its context must not look for it
  ctx->watched_comms.clear();
  for (hfmi_block* b : ctx->tmp_blocks)
    if (b) {
      if (b->owner && b->p) (void)hipFree(b->p);
      delete b;
    }
  pool_flush(ctx);
  for (int i = 0; i < WS_NSLOTS; ++i)
    if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pinned_cb) (void)hipHostFree(ctx->pinned_cb);
  if (ctx->late_pinned) (void)hipHostFree(ctx->late_pinned);
  xfer_destroy(ctx);
  for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ctx->ev_cb[i]);
  for (int i = 0; i < 8; ++i) (void)hipEventDestroy(ctx->ev_panel[i]);
  (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ingest_stream) {
    (void)hipStreamSynchronize(ctx->ingest_stream);
    for (int i = 0; i < HFMI_INGEST_RING; ++i) (void)hipEventDestroy(ctx->ev_ingest[i]);
    (void)hipStreamDestroy(ctx->ingest_stream);
  }
  (void)hipFree(ctx->small);
  (void)hipFree(ctx->status_dev);
  (void)hipHostFree(ctx->status_host);
  (void)hipEventDestroy(ctx->ev0);
  (void)hipEventDestroy(ctx->ev1);
  (void)hipEventDestroy(ctx->ev_status);
  (void)hipEventDestroy(ctx->ev_side);
  (void)hipStreamDestroy(ctx->aux_stream);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return HFMI_OK;
}

extern "C" int hfmi_ctx_set_stream(hfmi_ctx* ctx, void* hip_stream) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  if (hip_stream != nullptr && ctx->stream == (hipStream_t)hip_stream) return HFMI_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (hip_stream == nullptr) {
    if (!ctx->own_stream) {
      HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
      ctx->own_stream = true;
    }
  } else {
    if (ctx->own_stream) HIP_TRY(hipStreamDestroy(ctx->stream));
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
  }
  return HFMI_OK;
}
extern "C" int hfmi_ctx_get_stream(hfmi_ctx* ctx, void** hip_stream) {
  if (!ctx || !hip_stream) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  *hip_stream = (void*)ctx->stream;
  return HFMI_OK;
}
extern "C" int hfmi_ctx_synchronize(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ctx_check_comm(ctx);
}
extern "C" int hfmi_ctx_device_info(hfmi_ctx* ctx, char* name, int name_len, int* compute_units, int64_t* hbm_bytes) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
  if (name && name_len > 0) {
    snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  return HFMI_OK;
}
extern "C" int hfmi_timer_start(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  return HFMI_OK;
}
extern "C" int hfmi_timer_stop(hfmi_ctx* ctx, double* milliseconds) {
  if (!ctx || !milliseconds) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *milliseconds = ms;
  return HFMI_OK;
}

// ------------------------------------------------------------------ blocks
static int block_alloc(hfmi_ctx* ctx, int64_t N, int nvec, hfmi_block** out) {
  if (N <= 0 || nvec <= 0) HFMI_FAIL(HFMI_ERR_INVALID, "block: N=%lld nvec=%d must be positive", (long long)N, nvec);
  hfmi_block* b = new (std::nothrow) hfmi_block();
  if (!b) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  b->ctx = ctx;
  b->N = N;
  b->nvec = nvec;
  b->ld = round_up(N, 32);
  b->owner = true;
  b->p = (double*)pool_take(ctx, (size_t)b->ld * nvec * sizeof(double));
  hipError_t e = b->p ? hipSuccess : ctx_malloc(ctx, (void**)&b->p, (size_t)b->ld * nvec * sizeof(double));
  if (e != hipSuccess) {
    const double gb = (double)b->ld * nvec * 8 / 1e9;
    delete b;
    HFMI_FAIL(HFMI_ERR_HIP, "hipMalloc of a %lld x %d block (%.2f GB) failed: %s", (long long)N, nvec, gb, hipGetErrorString(e));
  }
  *out = b;
  return HFMI_OK;
}
extern "C" int hfmi_block_create(hfmi_ctx* ctx, int64_t N, int nvec, hfmi_block** out) {
  if (!ctx || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  hfmi_block* b = nullptr;
  HFMI_TRY(block_alloc(ctx, N, nvec, &b));
  hipError_t e = hipMemsetAsync(b->p, 0, (size_t)b->ld * nvec * sizeof(double), ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(b->p);
    delete b;
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

int ctx_tmp_block(hfmi_ctx* ctx, int idx, int64_t N, int nvec, hfmi_block** out) {
  if ((int)ctx->tmp_blocks.size() <= idx) ctx->tmp_blocks.resize(idx + 1, nullptr);
  hfmi_block* b = ctx->tmp_blocks[idx];
  if (b && (b->N != N || b->nvec < nvec)) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (void)hipFree(b->p);
    delete b;
    b = nullptr;
    ctx->tmp_blocks[idx] = nullptr;
  }
  if (!b) {
    HFMI_TRY(block_alloc(ctx, N, nvec, &b));
    HIP_TRY(hipMemsetAsync(b->p, 0, (size_t)b->ld * nvec * sizeof(double), ctx->stream));
    ctx->tmp_blocks[idx] = b;
  }
  *out = b;
  return HFMI_OK;
}

static int ctx_late_pinned(hfmi_ctx* ctx, void** out) {
  if (!ctx->late_pinned) HIP_TRY(hipHostMalloc(&ctx->late_pinned, 256 + (SM_LD + SM_MAXK) * sizeof(double), hipHostMallocDefault));
  *out = ctx->late_pinned;
  return HFMI_OK;
}

static int check_same_shape(const hfmi_block* a, const hfmi_block* b, const char* what) {
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
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return HFMI_OK;
}
extern "C" int hfmi_host_free_pinned(void* p) {
  if (p) HIP_TRY(hipHostFree(p));
  return HFMI_OK;
}
extern "C" int hfmi_block_upload_async(hfmi_block* b, const double* host_pinned, int layout, int64_t* ticket) {
  if (!b || !host_pinned) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = b->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->ingest_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&ctx->ingest_stream, hipStreamNonBlocking));
    for (int i = 0; i < HFMI_INGEST_RING; ++i) HIP_TRY(hipEventCreateWithFlags(&ctx->ev_ingest[i], hipEventDisableTiming));
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
    hipStream_t saved = ctx->stream;                                        // the launchers enqueue on ctx->stream
    ctx->stream = ctx->ingest_stream;
    const int s = launch_dense_to_block(ctx, (const double*)stage, b->p, b->ld, b->N, b->nvec);
    ctx->stream = saved;
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

// read `count` doubles of device memory back to the host (synchronises the stream)
static int read_back(hfmi_ctx* ctx, const double* dev, size_t count, double* host) {
  void* pin = nullptr;
  HFMI_TRY(ctx_pinned(ctx, count * sizeof(double), &pin));
  HIP_TRY(hipMemcpyAsync(pin, dev, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HFMI_TRY(ctx_check_comm(ctx));            // what was read may have come through a collective that gave up
  memcpy(host, pin, count * sizeof(double));
  return HFMI_OK;
}
// Split read-back: `begin` snapshots the status words at the current point of the main stream (event + copy on the
// auxiliary stream), `finish` waits for that copy only -- kernels queued on the main stream in between keep running
// while the host looks at the words and decides what to launch next.
// Y = A S with S upper triangular (R^-1 of a Cholesky-QR pass: every factorisation kernel writes its strict lower triangle as
// zeros): the hint lets the resident-S kernel skip the structurally zero column tiles; any other route ignores it
static int launch_nn_upper(hfmi_ctx* ctx, const double* A, int64_t lda, int m, const double* S, int ld, int r, double* Y, int64_t ldy,
                           int64_t N) {
  ctx->nn_upper_hint = true;
  const int s = launch_tsgemm_nn(ctx, A, lda, m, S, ld, r, 1.0, 0.0, Y, ldy, N);
  ctx->nn_upper_hint = false;
  return s;
}
static int read_status_begin(hfmi_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_status, 0));
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  return HFMI_OK;
}
// Small device -> host copies that nothing on the main stream waits for: a copy engine / blit between two dependent kernels costs
// the main stream 5 us of copy and 10-15 us of bubbles (timeline of the shard step), on the auxiliary stream it costs nothing.
// side_copies_begin orders the auxiliary stream behind the current point of the main stream; the copies are then enqueued on
// ctx->aux_stream by the caller; side_copies_end leaves an event the main stream can be made to wait for before a kernel
// overwrites the source.
static int side_copies_begin(hfmi_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_status, 0));
  return HFMI_OK;
}
static int side_copies_end(hfmi_ctx* ctx) {
  HIP_TRY(hipEventRecord(ctx->ev_side, ctx->aux_stream));
  return HFMI_OK;
}
static void print_status_dbg(const hfmi_status_words* out);
static int read_status_finish(hfmi_ctx* ctx, hfmi_status_words* out) {
  HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
  *out = *ctx->status_host;
  print_status_dbg(out);
  return HFMI_OK;
}
static int read_status(hfmi_ctx* ctx, hfmi_status_words* out) {
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out = *ctx->status_host;
  print_status_dbg(out);
  return HFMI_OK;
}
static void print_status_dbg(const hfmi_status_words* out) {
  static const bool dbg = env_flag("HFMI_DEBUG_TIMING");
  if (dbg)
    fprintf(stderr, "[hfmi timing] %s cycles: %lld %lld %lld %lld\n",
            out->tick[4] == 3 ? "chol-polish(load,-,-,out)" : out->tick[4] ? "jacobi(total,phase1,phase2,sweeps)" : "chol(load,chol,inv,out)",
            out->tick[0], out->tick[1], out->tick[2], out->tick[3]);
  if (dbg && (!out->tick[4] || out->tick[4] == 3))
    fprintf(stderr, "[hfmi timing]   chol status: min pivot ratio %.3e, input defect %.3e, shifted %d; blocked phases (diag, row, trailing) %lld %lld %lld\n",
            out->min_pivot_ratio, out->gram_dev, out->shifted, out->tick[5], out->tick[6], out->tick[7]);
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
static int upload_small(hfmi_ctx* ctx, const double* host, int rows, int cols, double* dev, int ld) {
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
  hfmi_csr* m = new (std::nothrow) hfmi_csr();
  if (!m) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  m->ctx = ctx;
  m->nrows = nrows;
  m->ncols = ncols;
  m->nnz = nnz;
  m->inv_diag = nullptr;
  m->ell_w = 0;
  m->ell_idx = nullptr;
  m->ell_val = nullptr;
  m->gersh_lmax = m->cheb_lmin = m->cheb_lmax = 0.0;
  m->cheb_state = 0;
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
    m->gersh_lmax = ok ? g : 0.0;
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
      HIP_TRY(hipMalloc((void**)&m->ell_idx, ei.size() * sizeof(int32_t)));
      HIP_TRY(hipMalloc((void**)&m->ell_val, ev.size() * sizeof(double)));
      HIP_TRY(hipMemcpy(m->ell_idx, ei.data(), ei.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(m->ell_val, ev.data(), ev.size() * sizeof(double), hipMemcpyHostToDevice));
      m->ell_w = (int)wmax;
    }
  }
  HIP_TRY(hipMalloc((void**)&m->indptr, (size_t)(nrows + 1) * sizeof(int64_t)));
  HIP_TRY(hipMalloc((void**)&m->indices, (size_t)std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
  HIP_TRY(hipMalloc((void**)&m->data, (size_t)std::max<int64_t>(nnz, 1) * sizeof(double)));
  HIP_TRY(hipMemcpy(m->indptr, indptr, (size_t)(nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->indices, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->data, data, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
  *out = m;
  return HFMI_OK;
}
extern "C" int hfmi_csr_destroy(hfmi_csr* m) {
  if (!m) return HFMI_OK;
  (void)hipStreamSynchronize(m->ctx->stream);
  (void)hipFree(m->indptr);
  (void)hipFree(m->indices);
  (void)hipFree(m->data);
  if (m->inv_diag) (void)hipFree(m->inv_diag);
  if (m->ell_idx) (void)hipFree(m->ell_idx);
  if (m->ell_val) (void)hipFree(m->ell_val);
  delete m;
  return HFMI_OK;
}

// ------------------------------------------------------------------ operators
static hfmi_op* op_new(hfmi_ctx* ctx, hfmi_op_kind kind) {
  hfmi_op* op = new (std::nothrow) hfmi_op();
  if (!op) return nullptr;
  memset((void*)op, 0, sizeof(*op));
  op->ctx = ctx;
  op->kind = kind;
  op->scale = 1.0;
  return op;
}
extern "C" int hfmi_op_snapshot_gram(hfmi_ctx* ctx, const hfmi_block* X, double scale, hfmi_op** out) {
  if (!ctx || !X || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_SNAPSHOT_GRAM);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *X;
  op->X.owner = false;
  op->scale = scale;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_low_rank(hfmi_ctx* ctx, const hfmi_block* U, const double* host_d, hfmi_op** out) {
  if (!ctx || !U || !host_d || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_SNAPSHOT_GRAM);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *U;
  op->X.owner = false;
  op->scale = 1.0;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipMalloc((void**)&op->weights, (size_t)U->nvec * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(op->weights, host_d, (size_t)U->nvec * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (op->weights) (void)hipFree(op->weights);
    delete op;
    HFMI_FAIL(HFMI_ERR_HIP, "op_low_rank: %s", hipGetErrorString(e));
  }
  *out = op;
  return HFMI_OK;
}
static int op_jac(hfmi_ctx* ctx, hfmi_op_kind kind, const hfmi_block* J, int ndata, int q, const double* host_gamma_inv,
                  double scale, hfmi_op** out) {
  if (!ctx || !J || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (ndata <= 0 || q <= 0 || (int64_t)ndata * q != J->nvec)
    HFMI_FAIL(HFMI_ERR_INVALID, "jacobian operator: ndata*q = %lld must equal the number of stored rows %d",
              (long long)ndata * q, J->nvec);
  hfmi_op* op = op_new(ctx, kind);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *J;
  op->X.owner = false;
  op->ndata = ndata;
  op->q = q;
  op->scale = scale;
  if (host_gamma_inv) {
    const int ld = (int)round_up(q, 16);
    HIP_TRY(hipMalloc((void**)&op->gamma_inv, (size_t)q * ld * sizeof(double)));
    int s = upload_small(ctx, host_gamma_inv, q, q, op->gamma_inv, ld);
    if (s != HFMI_OK) return s;
  }
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_jtj(hfmi_ctx* ctx, const hfmi_block* J, int ndata, int q, const double* host_gamma_inv,
                           double scale, hfmi_op** out) {
  return op_jac(ctx, OP_JTJ, J, ndata, q, host_gamma_inv, scale, out);
}
extern "C" int hfmi_op_jjt(hfmi_ctx* ctx, const hfmi_block* J, int ndata, int q, double scale, hfmi_op** out) {
  return op_jac(ctx, OP_JJT, J, ndata, q, nullptr, scale, out);
}
extern "C" int hfmi_op_dense_sym(hfmi_ctx* ctx, const hfmi_block* C, hfmi_op** out) {
  if (!ctx || !C || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (C->N != C->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "dense_sym: matrix must be square (%lld x %d)", (long long)C->N, C->nvec);
  hfmi_op* op = op_new(ctx, OP_DENSE_SYM);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->X = *C;
  op->X.owner = false;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_csr(hfmi_ctx* ctx, const hfmi_csr* M, hfmi_op** out) {
  if (!ctx || !M || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_CSR);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->csr = M;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_csr_pcg(hfmi_ctx* ctx, const hfmi_csr* M, double rel_tol, int max_iter, hfmi_op** out) {
  if (!ctx || !M || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (M->nrows != M->ncols) HFMI_FAIL(HFMI_ERR_INVALID, "csr_pcg: matrix must be square");
  hfmi_op* op = op_new(ctx, OP_CSR_PCG);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->csr = M;
  op->rel_tol = rel_tol > 0 ? rel_tol : 1e-13;
  op->max_iter = max_iter > 0 ? max_iter : 500;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_amg_pcg(hfmi_ctx* ctx, hfmi_amg* amg, double rel_tol, int max_iter, hfmi_op** out) {
  if (!ctx || !amg || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_AMG_PCG);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->amg = amg;
  op->rel_tol = rel_tol > 0 ? rel_tol : 1e-12;
  op->max_iter = max_iter > 0 ? max_iter : 100;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_solver_info(const hfmi_op* op, int* iterations, int* method, double* lmin, double* lmax) {
  if (op && op->kind == OP_AMG_PCG) {
    if (iterations) *iterations = op->last_iters;
    if (method) *method = 2;
    if (lmin) *lmin = 0.0;
    if (lmax) *lmax = 0.0;
    return HFMI_OK;
  }
  if (!op || op->kind != OP_CSR_PCG) HFMI_FAIL(HFMI_ERR_INVALID, "op_solver_info: not a sparse solver operator");
  if (iterations) *iterations = op->last_iters;
  if (method) *method = op->last_method;
  if (lmin) *lmin = op->csr->cheb_state == 1 ? op->csr->cheb_lmin : 0.0;
  if (lmax) *lmax = op->csr->cheb_state == 1 ? op->csr->cheb_lmax : 0.0;
  return HFMI_OK;
}
extern "C" int hfmi_op_compose3(hfmi_ctx* ctx, hfmi_op* a, hfmi_op* b, hfmi_op* c, hfmi_op** out) {
  if (!ctx || !a || !b || !c || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_COMPOSE3);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->a = a;
  op->b = b;
  op->c = c;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_host_callback(hfmi_ctx* ctx, hfmi_host_apply_fn fn, void* user, int64_t N, hfmi_op** out) {
  if (!ctx || !fn || !out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_op* op = op_new(ctx, OP_HOST);
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "out of host memory");
  op->host_fn = fn;
  op->host_user = user;
  op->host_N = N;
  *out = op;
  return HFMI_OK;
}
extern "C" int hfmi_op_host_set_chunk(hfmi_op* op, int vectors) {
  if (!op || op->kind != OP_HOST) HFMI_FAIL(HFMI_ERR_INVALID, "op_host_set_chunk: not a host-callback operator");
  if (vectors < 0) HFMI_FAIL(HFMI_ERR_INVALID, "op_host_set_chunk: negative slab size");
  op->host_chunk = vectors;
  return HFMI_OK;
}
extern "C" int hfmi_op_set_post_apply(hfmi_op* op, hfmi_post_apply_fn fn, void* user) {
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "null op");
  op->post_fn = fn;
  op->post_user = user;
  return HFMI_OK;
}
extern "C" int hfmi_op_set_collective(hfmi_op* op, hfmi_comm* comm, int reduce_op) {
  if (!op) HFMI_FAIL(HFMI_ERR_INVALID, "null op");
  if (comm && reduce_op != HFMI_REDUCE_SUM && reduce_op != HFMI_REDUCE_AVG)
    HFMI_FAIL(HFMI_ERR_INVALID, "op_set_collective: reduce_op must be HFMI_REDUCE_SUM or HFMI_REDUCE_AVG");
  op->comm = comm;
  op->comm_op = reduce_op;
  return HFMI_OK;
}
extern "C" int hfmi_op_destroy(hfmi_op* op) {
  if (!op) return HFMI_OK;
  if (op->gamma_inv || op->weights) {
    (void)hipStreamSynchronize(op->ctx->stream);
    if (op->gamma_inv) (void)hipFree(op->gamma_inv);
    if (op->weights) (void)hipFree(op->weights);
  }
  delete op;
  return HFMI_OK;
}

// Y = M^{-1} W for an SPD CSR matrix: Jacobi-preconditioned CG run on all vectors at once (independent
// recurrences, shared SpMM); per-vector scalars stay on the device, the host only polls convergence.
static int pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y);

// ---- spectrum of D^-1 A for the Chebyshev solve -------------------------------------------------------------------------
// extreme eigenvalues of the symmetric tridiagonal matrix (a, b) by bisection on the Sturm count
static int sturm_count(const std::vector<double>& a, const std::vector<double>& b, double x) {
  int cnt = 0;
  double q = a[0] - x;
  if (q < 0) ++cnt;
  for (size_t i = 1; i < a.size(); ++i) {
    if (q == 0.0) q = 1e-300;
    q = a[i] - x - b[i - 1] * b[i - 1] / q;
    if (q < 0) ++cnt;
  }
  return cnt;
}
static void tridiag_extremes(const std::vector<double>& a, const std::vector<double>& b, double* smallest, double* largest) {
  double lo = a[0], hi = a[0];
  for (size_t i = 0; i < a.size(); ++i) {
    const double rad = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < a.size() ? fabs(b[i]) : 0.0);
    lo = std::min(lo, a[i] - rad);
    hi = std::max(hi, a[i] + rad);
  }
  const int m = (int)a.size();
  double l = lo, h = hi;
  for (int it = 0; it < 200 && h - l > 1e-14 * std::max(fabs(l), fabs(h)); ++it) {   // smallest: first x with count >= 1
    const double mid = 0.5 * (l + h);
    if (sturm_count(a, b, mid) >= 1) h = mid; else l = mid;
  }
  *smallest = 0.5 * (l + h);
  l = lo; h = hi;
  for (int it = 0; it < 200 && h - l > 1e-14 * std::max(fabs(l), fabs(h)); ++it) {   // largest: last x with count < m
    const double mid = 0.5 * (l + h);
    if (sturm_count(a, b, mid) >= m) h = mid; else l = mid;
  }
  *largest = 0.5 * (l + h);
}
// One scalar Jacobi-CG run on a pseudo-random right-hand side, on the device, with its two inner products per iteration read
// back: the CG coefficients are the Lanczos matrix of D^-1 A, whose extreme eigenvalues approach those of D^-1 A from inside.
// Once per matrix (~40 iterations of one-vector kernels).
static int cheb_estimate(hfmi_op* op) {
  hfmi_ctx* ctx = op->ctx;
  hfmi_csr* M = const_cast<hfmi_csr*>(op->csr);
  const int64_t N = M->nrows;
  M->cheb_state = -1;
  if (!(M->gersh_lmax > 0.0)) return HFMI_OK;
  hfmi_block *R, *Z, *P, *AP;
  HFMI_TRY(ctx_tmp_block(ctx, 8, N, 1, &R));
  HFMI_TRY(ctx_tmp_block(ctx, 9, N, 1, &Z));
  HFMI_TRY(ctx_tmp_block(ctx, 10, N, 1, &P));
  HFMI_TRY(ctx_tmp_block(ctx, 11, N, 1, &AP));
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, 4 * sizeof(double), &sc));
  double *rz = (double*)sc, *pap = rz + 1, *rz_new = rz + 2;
  HFMI_TRY(launch_randn(ctx, R->p, N, 1, R->ld, 0x5eedc0deull, 77u, 1.0));
  HFMI_TRY(launch_diag_scale(ctx, Z->p, Z->ld, R->p, R->ld, M->inv_diag, N, 1));
  HFMI_TRY(launch_copy(ctx, P->p, P->ld, Z->p, Z->ld, N, 1));
  HFMI_TRY(launch_col_dots(ctx, R->p, R->ld, Z->p, Z->ld, N, 1, rz));
  double h_rz = 0, h_pap = 0, h_new = 0;
  HFMI_TRY(read_back(ctx, rz, 1, &h_rz));
  const double rz0 = h_rz;
  std::vector<double> alpha, beta;
  for (int it = 0; it < 60 && h_rz > 1e-28 * rz0; ++it) {
    HFMI_TRY(launch_csr_spmm(ctx, M, P->p, P->ld, AP->p, AP->ld, 1, false));
    HFMI_TRY(launch_col_dots(ctx, P->p, P->ld, AP->p, AP->ld, N, 1, pap));
    HFMI_TRY(launch_col_axpy_dev(ctx, R->p, R->ld, AP->p, AP->ld, N, 1, rz, pap, -1.0));
    HFMI_TRY(launch_diag_scale(ctx, Z->p, Z->ld, R->p, R->ld, M->inv_diag, N, 1));
    HFMI_TRY(launch_col_dots(ctx, R->p, R->ld, Z->p, Z->ld, N, 1, rz_new));
    HFMI_TRY(launch_col_xpby_dev(ctx, P->p, P->ld, Z->p, Z->ld, N, 1, rz_new, rz));
    double two[3];
    HFMI_TRY(read_back(ctx, rz, 3, two));
    h_pap = two[1];
    h_new = two[2];
    if (!(h_pap > 0.0) || !std::isfinite(h_new)) return HFMI_OK;     // not SPD: leave the Chebyshev route off
    alpha.push_back(h_rz / h_pap);
    beta.push_back(h_new / h_rz);
    HIP_TRY(hipMemcpyAsync(rz, rz_new, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    h_rz = h_new;
  }
  const size_t m = alpha.size();
  if (m < 3) return HFMI_OK;
  std::vector<double> a(m), b(m > 1 ? m - 1 : 0);
  for (size_t i = 0; i < m; ++i) {
    a[i] = 1.0 / alpha[i] + (i > 0 ? beta[i - 1] / alpha[i - 1] : 0.0);
    if (i + 1 < m) b[i] = sqrt(beta[i]) / alpha[i];
  }
  double tmin, tmax;
  tridiag_extremes(a, b, &tmin, &tmax);
  if (!(tmin > 0.0) || !(tmax >= tmin)) return HFMI_OK;
  // Ritz values lie inside the spectrum: widen them; never above Gershgorin's bound
  M->cheb_lmin = 0.9 * tmin;
  M->cheb_lmax = std::min(M->gersh_lmax, 1.05 * tmax);
  if (M->cheb_lmax < tmax) M->cheb_lmax = tmax * (1.0 + 1e-9);
  M->cheb_state = 1;
  return HFMI_OK;
}

// Y = M^-1 W by Chebyshev iteration on row-major copies (hfmi_cheb.hip); *handled = false: the caller runs the block CG
static int cheb_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, bool* handled) {
  hfmi_ctx* ctx = op->ctx;
  hfmi_csr* M = const_cast<hfmi_csr*>(op->csr);
  const int64_t N = W->N;
  const int k = W->nvec;
  *handled = false;
  static const bool off = env_flag("HFMI_PCG");          // A/B switch: always the block CG
  if (off || M->cheb_state < 0) return HFMI_OK;
  if (M->cheb_state == 0) HFMI_TRY(cheb_estimate(op));
  if (M->cheb_state != 1) return HFMI_OK;
  const double lmin = M->cheb_lmin, lmax = M->cheb_lmax;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
  hfmi_block *Bb, *X0b, *X1b;
  HFMI_TRY(ctx_tmp_block(ctx, 8, N, k, &Bb));
  HFMI_TRY(ctx_tmp_block(ctx, 9, N, k, &X0b));
  HFMI_TRY(ctx_tmp_block(ctx, 10, N, k, &X1b));
  double* B = Bb->p;                                                 // used as row-major N x k arrays (ld >= N: large enough)
  double* X[2] = {X0b->p, X1b->p};
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)2 * k * sizeof(double), &sc));
  double* bb = (double*)sc;
  double* rr = bb + k;
  HFMI_TRY(launch_block_to_dense(ctx, W->p, W->ld, B, N, k));
  HFMI_TRY(launch_rm_colsq(ctx, B, N, k, bb));
  HFMI_TRY(launch_cheb_first(ctx, B, X[1], X[0], M->inv_diag, N, k, 1.0 / theta));     // x_0 = 0 in X[0], x_1 in X[1]
  int steps = 1, cur = 1;                                            // X[cur] = x_steps, X[cur ^ 1] = x_{steps-1}
  const bool spread = delta > 1e-12 * theta;                         // else D^-1 A is a multiple of the identity: x_1 is the answer
  double rho = spread ? delta / theta : 0.0;                         // 1 / sigma
  int planned = 1;
  if (spread) {
    const double sk = sqrt(lmax / lmin), c = (sk - 1.0) / (sk + 1.0);
    planned = (int)ceil(log(2.0 / op->rel_tol) / -log(c)) + 1;
  }
  if (planned > op->max_iter || planned > 200) {
    // a spectrum this wide needs more steps than CG's superlinear convergence would: leave this matrix to the block CG
    M->cheb_state = -1;
    return HFMI_OK;
  }
  std::vector<double> h(2 * (size_t)k);
  int budget = planned - 1;
  for (int round = 0; round < 4; ++round) {
    for (int i = 0; i < budget; ++i, ++steps) {
      const double rho_new = 1.0 / (2.0 * theta / delta - rho);
      HFMI_TRY(launch_cheb_step(ctx, M, B, X[cur], X[cur ^ 1], k, rho_new * rho, 2.0 * rho_new / delta, false));
      rho = rho_new;
      cur ^= 1;
    }
    // the true residual b - A x into the spare array, its column norms against those of b
    void* rs = nullptr;
    HFMI_TRY(ctx_ws(ctx, WS_STAGE, (size_t)N * k * sizeof(double), &rs));
    HFMI_TRY(launch_cheb_step(ctx, M, B, X[cur], (double*)rs, k, 0.0, 0.0, true));
    HFMI_TRY(launch_rm_colsq(ctx, (const double*)rs, N, k, rr));
    HFMI_TRY(read_back(ctx, bb, (size_t)2 * k, h.data()));
    bool done = true, diverged = false;
    for (int j = 0; j < k; ++j) {
      if (!std::isfinite(h[j]))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "csr solve: non-finite right-hand side in vector %d", j);
      // a residual that is not finite, or larger than the right-hand side it started from, means the polynomial grew: an
      // eigenvalue of D^-1 A lies outside the bracket (Ritz values of a short CG run from one random vector can miss the top of
      // the spectrum).  That is a failure of the ESTIMATE, not of the matrix: hand the solve to the block CG, which alone
      // reports a matrix that is not SPD (advisor r4)
      if (!std::isfinite(h[k + j]) || h[k + j] > h[j]) diverged = true;
      if (!(h[k + j] <= op->rel_tol * op->rel_tol * h[j])) done = false;
    }
    if (diverged) break;
    if (done) {
      op->last_iters = steps;
      op->last_method = 1;
      HFMI_TRY(launch_dense_to_block(ctx, X[cur], Y->p, Y->ld, N, k));
      *handled = true;
      return HFMI_OK;
    }
    if (!spread) break;
    budget = std::max(2, planned / 3);
    if (steps + budget > op->max_iter) break;
  }
  M->cheb_state = -1;       // the bracket of the spectrum was not good enough: this matrix goes back to the block CG for good
  return HFMI_OK;
}

static int pcg_solve(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_ctx* ctx = op->ctx;
  hfmi_csr* M = const_cast<hfmi_csr*>(op->csr);
  const int64_t N = W->N;
  const int k = W->nvec;
  if (M->nrows != N) HFMI_FAIL(HFMI_ERR_INVALID, "csr_pcg: matrix has %lld rows, block vectors have %lld", (long long)M->nrows, (long long)N);
  if (!M->inv_diag) {
    HIP_TRY(hipMalloc((void**)&M->inv_diag, (size_t)N * sizeof(double)));
    HFMI_TRY(launch_csr_diag_inv(ctx, M));
  }
  {
    bool handled = false;
    HFMI_TRY(cheb_solve(op, W, Y, &handled));
    if (handled) return HFMI_OK;
  }
  hfmi_block *R, *Z, *P, *AP;
  HFMI_TRY(ctx_tmp_block(ctx, 8, N, k, &R));
  HFMI_TRY(ctx_tmp_block(ctx, 9, N, k, &Z));
  HFMI_TRY(ctx_tmp_block(ctx, 10, N, k, &P));
  HFMI_TRY(ctx_tmp_block(ctx, 11, N, k, &AP));
  void* sc = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)6 * k * sizeof(double), &sc));
  // two (r.z, r.r) pairs: an iteration reads r.z from one and writes the new r.z and r.r into the other (r.r must follow
  // r.z_new: launch_pcg_update fills both with one final pass); the pairs swap roles instead of being copied
  double* rz = (double*)sc;       // r.z
  double* rz_new = rz + 2 * k;
  double* rr = rz_new + k;
  double* pap = rz + 4 * k;
  double* bb = rz + 5 * k;
  std::vector<double> h_rr(k), h_bb(k);
  // x0 = 0, r = b
  HFMI_TRY(launch_fill(ctx, Y->p, N, k, Y->ld, 0.0, false));
  HFMI_TRY(launch_copy(ctx, R->p, R->ld, W->p, W->ld, N, k));
  HFMI_TRY(launch_col_dots(ctx, W->p, W->ld, W->p, W->ld, N, k, bb));
  HFMI_TRY(read_back(ctx, bb, k, h_bb.data()));
  HFMI_TRY(launch_diag_scale(ctx, Z->p, Z->ld, R->p, R->ld, M->inv_diag, N, k));
  HFMI_TRY(launch_copy(ctx, P->p, P->ld, Z->p, Z->ld, N, k));
  HFMI_TRY(launch_col_dots(ctx, R->p, R->ld, Z->p, Z->ld, N, k, rz));
  int it = 0;
  bool done = false;
  for (; it < op->max_iter && !done; ++it) {
    if (M->ell_w > 0) {
      // three passes over the blocks per iteration: A p fused with p . A p; (x, r) update fused with both residual
      // dots; the new direction with z = D^-1 r recomputed on the fly (never stored)
      HFMI_TRY(launch_ell_spmm_dot(ctx, M, P->p, P->ld, AP->p, AP->ld, k, pap));
      HFMI_TRY(launch_pcg_update(ctx, Y->p, Y->ld, R->p, R->ld, P->p, P->ld, AP->p, AP->ld, M->inv_diag, N, k, rz, pap, rz_new, rr));
      HFMI_TRY(launch_pcg_direction(ctx, P->p, P->ld, R->p, R->ld, M->inv_diag, N, k, rz_new, rz));
      double* const rr_done = rr;
      std::swap(rz, rz_new);        // the pair just written becomes "current"
      rr = rz_new + k;
      if ((it & 3) == 3 || it + 1 == op->max_iter) {
        HFMI_TRY(read_back(ctx, rr_done, k, h_rr.data()));
        done = true;
        for (int j = 0; j < k; ++j)
          if (!(h_rr[j] <= op->rel_tol * op->rel_tol * h_bb[j])) done = false;
        for (int j = 0; j < k; ++j)
          if (!std::isfinite(h_rr[j]) || !std::isfinite(h_bb[j]))
            HFMI_FAIL(HFMI_ERR_NUMERIC, "csr_pcg: non-finite residual in vector %d at iteration %d (matrix not SPD, or non-finite input)", j, it + 1);
      }
      continue;
    }
    HFMI_TRY(launch_csr_spmm(ctx, M, P->p, P->ld, AP->p, AP->ld, k, false));
    HFMI_TRY(launch_col_dots(ctx, P->p, P->ld, AP->p, AP->ld, N, k, pap));
    HFMI_TRY(launch_col_axpy_dev(ctx, Y->p, Y->ld, P->p, P->ld, N, k, rz, pap, 1.0));
    HFMI_TRY(launch_col_axpy_dev(ctx, R->p, R->ld, AP->p, AP->ld, N, k, rz, pap, -1.0));
    HFMI_TRY(launch_diag_scale(ctx, Z->p, Z->ld, R->p, R->ld, M->inv_diag, N, k));
    HFMI_TRY(launch_col_dots(ctx, R->p, R->ld, Z->p, Z->ld, N, k, rz_new));
    HFMI_TRY(launch_col_xpby_dev(ctx, P->p, P->ld, Z->p, Z->ld, N, k, rz_new, rz));
    HIP_TRY(hipMemcpyAsync(rz, rz_new, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if ((it & 3) == 3 || it + 1 == op->max_iter) {
      HFMI_TRY(launch_col_dots(ctx, R->p, R->ld, R->p, R->ld, N, k, rr));
      HFMI_TRY(read_back(ctx, rr, k, h_rr.data()));
      done = true;
      for (int j = 0; j < k; ++j)
        if (!(h_rr[j] <= op->rel_tol * op->rel_tol * h_bb[j])) done = false;
      for (int j = 0; j < k; ++j)
        if (!std::isfinite(h_rr[j]) || !std::isfinite(h_bb[j]))
          HFMI_FAIL(HFMI_ERR_NUMERIC, "csr_pcg: non-finite residual in vector %d at iteration %d (matrix not SPD, or non-finite input)", j, it + 1);
    }
  }
  op->last_iters = it;
  op->last_method = 0;
  if (!done) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "csr_pcg: no convergence to %.1e in %d iterations", op->rel_tol, op->max_iter);
  return HFMI_OK;
}

// Host black box on a device block (hfmi_op_host_callback): W goes device -> pinned host, the callback fills Y on the
// host, Y goes pinned host -> device.  With a slab size (hfmi_op_host_set_chunk) the three legs are pipelined over
// slabs of vectors: while the host works on slab i, slab i+1 is already arriving on the auxiliary stream and slab i-1
// is on its way back on the main stream.  The host-side wall clock of the three legs is kept for the phase report.
static double wall_ms() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
static int host_apply_pipelined(hfmi_op* op, const hfmi_block* W, hfmi_block* Y) {
  hfmi_ctx* ctx = op->ctx;
  const int64_t N = W->N, NY = Y->N;
  const int k = W->nvec;
  const int chunk = (op->host_chunk > 0 && op->host_chunk < k) ? op->host_chunk : k;
  const int nchunks = (k + chunk - 1) / chunk;
  const size_t wslab = (size_t)chunk * N, yslab = (size_t)chunk * NY;
  const int nbuf = nchunks > 1 ? 2 : 1;
  const size_t need = (size_t)nbuf * (wslab + yslab) * sizeof(double);
  if (need > ctx->pinned_cb_bytes) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->pinned_cb) HIP_TRY(hipHostFree(ctx->pinned_cb));
    ctx->pinned_cb = nullptr;
    ctx->pinned_cb_bytes = 0;
    HIP_TRY(hipHostMalloc(&ctx->pinned_cb, need, hipHostMallocDefault));
    ctx->pinned_cb_bytes = need;
  }
  double* wbuf[2] = {(double*)ctx->pinned_cb, (double*)ctx->pinned_cb + (nbuf - 1) * wslab};
  double* ybuf[2] = {(double*)ctx->pinned_cb + nbuf * wslab, (double*)ctx->pinned_cb + nbuf * wslab + (nbuf - 1) * yslab};
  auto fetch = [&](int c) -> int {      // slab c of W -> wbuf[c & 1] on the auxiliary stream
    const int c0 = c * chunk, nc = std::min(chunk, k - c0);
    HIP_TRY(hipMemcpy2DAsync(wbuf[c & 1], (size_t)N * sizeof(double), W->p + (int64_t)c0 * W->ld, (size_t)W->ld * sizeof(double),
                             (size_t)N * sizeof(double), (size_t)nc, hipMemcpyDeviceToHost, ctx->aux_stream));
    HIP_TRY(hipEventRecord(ctx->ev_cb[c & 1], ctx->aux_stream));
    return HFMI_OK;
  };
  // W is complete once the main stream reaches this point
  HIP_TRY(hipEventRecord(ctx->ev_status, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_status, 0));
  HFMI_TRY(fetch(0));
  double t_d2h = 0.0, t_fn = 0.0, t_h2d = 0.0;
  for (int c = 0; c < nchunks; ++c) {
    const int c0 = c * chunk, nc = std::min(chunk, k - c0);
    double t0 = wall_ms();
    HIP_TRY(hipEventSynchronize(ctx->ev_cb[c & 1]));                       // slab c has arrived
    if (c + 1 < nchunks) HFMI_TRY(fetch(c + 1));                           // wbuf[(c+1)&1] was consumed by call c-1
    double t1 = wall_ms();
    t_d2h += t1 - t0;
    if (c >= 2) HIP_TRY(hipEventSynchronize(ctx->ev_cb[2 + (c & 1)]));     // ybuf[c&1] has left for the device (slab c-2)
    double t2 = wall_ms();
    t_h2d += t2 - t1;
    memset(ybuf[c & 1], 0, (size_t)nc * NY * sizeof(double));
    const int rc = op->host_fn(op->host_user, wbuf[c & 1], ybuf[c & 1], N, nc);
    double t3 = wall_ms();
    t_fn += t3 - t2;
    if (rc != 0) {
      (void)hipStreamSynchronize(ctx->aux_stream);
      (void)hipStreamSynchronize(ctx->stream);
      HFMI_FAIL(HFMI_ERR_CALLBACK, "host operator callback returned %d", rc);
    }
    HIP_TRY(hipMemcpy2DAsync(Y->p + (int64_t)c0 * Y->ld, (size_t)Y->ld * sizeof(double), ybuf[c & 1], (size_t)NY * sizeof(double),
                             (size_t)NY * sizeof(double), (size_t)nc, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev_cb[2 + (c & 1)], ctx->stream));
    t_h2d += wall_ms() - t3;
  }
  double t0 = wall_ms();
  HIP_TRY(hipStreamSynchronize(ctx->stream));                              // the pinned slabs are free again
  t_h2d += wall_ms() - t0;
  if (ctx->profiling) {
    ctx->phase_ms[HFMI_PHASE_HOST_D2H] += t_d2h;
    ctx->phase_ms[HFMI_PHASE_HOST_FN] += t_fn;
    ctx->phase_ms[HFMI_PHASE_HOST_H2D] += t_h2d;
  }
  return HFMI_OK;
}

static int op_apply_raw(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, double beta);
static int phase_begin_on(hfmi_ctx* ctx, int phase, hipStream_t st);
static void phase_end_on(hfmi_ctx* ctx, int idx, hipStream_t st);

// Overlapped rank reduction of an operator application (collectiveOperator.py:73-80, collective.py:98-111): the
// last contraction of a Gram-form apply (Y = X^T G) is issued in row panels of whole rounds of tiles (hfmi_gemm_nn.hip), and
// as soon as a panel's rows are final they are packed into a contiguous buffer, all-reduced and unpacked on the AUXILIARY
// stream while the next panel is computed on the main one.  Only the last panel's reduction is exposed.  Same arithmetic per
// element as the one-launch product followed by one all-reduce of the block: bit-identical results (tests/test_gpu_comm.py).
struct panel_reduce {
  hfmi_op* op;
  int npanels;
  int64_t stage_off;     // doubles used in WS_COMM so far
  double* stage;
  int status;
};
static int panel_reduce_hook(void* user, double* Y, int64_t ldy, int r, int64_t row0, int64_t rows) {
  panel_reduce* pr = (panel_reduce*)user;
  hfmi_ctx* ctx = pr->op->ctx;
  if (pr->npanels >= 8) HFMI_FAIL(HFMI_ERR_INVALID, "panel_reduce: more than 8 row panels");
  hipEvent_t ev = ctx->ev_panel[pr->npanels++];
  HIP_TRY(hipEventRecord(ev, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ev, 0));
  double* st = pr->stage + pr->stage_off;
  const int64_t rld = round_up(rows, 2);
  pr->stage_off += rld * r;
  const int ph = phase_begin_on(ctx, HFMI_PHASE_ALLREDUCE_AUX, ctx->aux_stream);
  if (rld != rows) HIP_TRY(hipMemsetAsync(st, 0, (size_t)rld * r * sizeof(double), ctx->aux_stream));
  HIP_TRY(hipMemcpy2DAsync(st, (size_t)rld * sizeof(double), Y + row0, (size_t)ldy * sizeof(double), (size_t)rows * sizeof(double),
                           (size_t)r, hipMemcpyDeviceToDevice, ctx->aux_stream));
  HFMI_TRY(comm_allreduce_device_on(pr->op->comm, st, rld * r, pr->op->comm_op, ctx->aux_stream));
  HIP_TRY(hipMemcpy2DAsync(Y + row0, (size_t)ldy * sizeof(double), st, (size_t)rld * sizeof(double), (size_t)rows * sizeof(double),
                           (size_t)r, hipMemcpyDeviceToDevice, ctx->aux_stream));
  phase_end_on(ctx, ph, ctx->aux_stream);
  return HFMI_OK;
}
static int g_comm_panels = -1;    // HFMI_COMM_PANELS: 0 = one all-reduce after the product, n = at most n row panels (default 4)
// What a profiling region (hfmi_profile_begin .. _end) records.  Every record is a pair of events on the stream, and an event
// between two dependent kernels costs 2-4 us of idle GPU: with one pair per contraction and per phase a 64-sample shard step of
// config 4 carried ~32 of them.  Level 2 (default): contractions and phases.  Level 1: only contractions of at least
// HFMI_PROF_MIN_GFLOP (2.0) Gflop -- what a roofline line needs -- and no phases.
static int g_prof_level = 2;
// HFMI_QR_TRUST_FIRST=0 / tuning key "qr_trust_first": the first Cholesky-QR pass of the Gram-form solve waits for its status words
// (the behaviour up to round 4: one host round trip in the middle of every solve); default 1
static int g_qr_trust_first = -1;
int api_tuning_set(const char* key, int value) {
  if (key && !strcmp(key, "comm_panels") && value >= 0 && value <= 8) {
    g_comm_panels = value;
    return 1;
  }
  if (key && !strcmp(key, "prof_level") && (value == 1 || value == 2)) {
    g_prof_level = value;
    return 1;
  }
  if (key && !strcmp(key, "qr_trust_first") && (value == 0 || value == 1)) {
    g_qr_trust_first = value;
    return 1;
  }
  return 0;
}

static int op_apply_raw(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, double beta) {
  hfmi_ctx* ctx = op->ctx;
  const int k = W->nvec;
  switch (op->kind) {
    case OP_SNAPSHOT_GRAM:
    case OP_JTJ: {
      const hfmi_block& X = op->X;
      if (X.N != W->N) HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld", (long long)X.N, (long long)W->N);
      const int m = X.nvec;
      const int ldg = (int)round_up(k, 16);
      void* G = nullptr;
      HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)m * ldg * sizeof(double), &G));
      // G (m x k) = scale * X^T W ; then Y = X G
      HFMI_TRY(launch_tsgemm_tn(ctx, X.p, X.ld, m, W->p, W->ld, k, X.N, op->scale, 0.0, (double*)G, ldg, 1, 0));
      if (op->kind == OP_JTJ && op->gamma_inv)
        HFMI_TRY(launch_gamma_apply(ctx, (double*)G, ldg, op->ndata, op->q, k, op->gamma_inv, (int)round_up(op->q, 16)));
      if (op->weights) HFMI_TRY(launch_row_scale(ctx, (double*)G, ldg, m, k, op->weights));
      if (g_comm_panels < 0) {
        const char* e = getenv("HFMI_COMM_PANELS");
        g_comm_panels = e ? atoi(e) : 4;
        if (g_comm_panels < 0 || g_comm_panels > 8) g_comm_panels = 4;
      }
      if (op->comm && g_comm_panels > 1 && beta == 0.0 && comm_transport(op->comm) != 0 && k <= 256) {
        void* sv = nullptr;
        HFMI_TRY(ctx_ws(ctx, WS_COMM, ((size_t)Y->ld + 16) * k * sizeof(double), &sv));
        // the largest panel is at most the whole block: size the transport's staging area for that before the first panel is
        // in flight on the auxiliary stream (regrowing it later would close peers' mappings under a running reduction)
        HFMI_TRY(comm_reserve_stage(op->comm, ((size_t)Y->ld + 16) * k * sizeof(double)));
        panel_reduce pr = {op, 0, 0, (double*)sv, HFMI_OK};
        ctx->nn_hook = panel_reduce_hook;
        ctx->nn_hook_user = &pr;
        ctx->nn_hook_panels = g_comm_panels;
        ctx->nn_hook_called = false;
        const int s = launch_tsgemm_nn(ctx, X.p, X.ld, m, (const double*)G, ldg, k, 1.0, beta, Y->p, Y->ld, X.N);
        ctx->nn_hook = nullptr;
        if (s != HFMI_OK) return s;
        if (ctx->nn_hook_called) {
          // join: the main stream continues when the last panel is back
          const int ph = phase_begin(ctx, HFMI_PHASE_ALLREDUCE);
          HIP_TRY(hipEventRecord(ctx->ev_join, ctx->aux_stream));
          HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
          phase_end(ctx, ph);
          op->reduced_by_panels = true;
        }
        return HFMI_OK;
      }
      HFMI_TRY(launch_tsgemm_nn(ctx, X.p, X.ld, m, (const double*)G, ldg, k, 1.0, beta, Y->p, Y->ld, X.N));
      return HFMI_OK;
    }
    case OP_JJT: {
      // Y (q x k) = scale * sum_i J_i (J_i^T W): per sample  H_i (N x k) = J_i^T-as-block * W ; Y += J_i^T H_i
      const hfmi_block& J = op->X;
      const int q = op->q;
      if (W->N != q) HFMI_FAIL(HFMI_ERR_INVALID, "JJT acts on vectors of length %d, got %lld", q, (long long)W->N);
      hfmi_block* H = nullptr;
      HFMI_TRY(ctx_tmp_block(ctx, 12, J.N, k, &H));
      // W as a small row-major (q x k) matrix: W block is column-major q x k with ld -> transpose into WS_G
      const int ldw = (int)round_up(k, 16);
      void* Ws = nullptr;
      HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)q * ldw * sizeof(double), &Ws));
      HIP_TRY(hipMemsetAsync(Ws, 0, (size_t)q * ldw * sizeof(double), ctx->stream));
      HFMI_TRY(launch_block_to_dense_ld(ctx, W->p, W->ld, (double*)Ws, ldw, q, k));
      for (int i = 0; i < op->ndata; ++i) {
        const double* Ji = J.p + (int64_t)i * q * J.ld;
        HFMI_TRY(launch_tsgemm_nn(ctx, Ji, J.ld, q, (const double*)Ws, ldw, k, 1.0, 0.0, H->p, H->ld, J.N));
        // Y[o][j] (+)= scale * <J_i row o, H_j>  -> column-major q x k output: rs = 1, cs = ld
        HFMI_TRY(launch_tsgemm_tn(ctx, Ji, J.ld, q, H->p, H->ld, k, J.N, op->scale, (i == 0) ? beta : 1.0, Y->p, 1, Y->ld, 0));
      }
      return HFMI_OK;
    }
    case OP_DENSE_SYM: {
      const hfmi_block& C = op->X;
      if (C.N != W->N) HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld", (long long)C.N, (long long)W->N);
      // Y = C W with C symmetric: Y[t][j] = <C_t, W_j>  (column-major output)
      return launch_tsgemm_tn(ctx, C.p, C.ld, C.nvec, W->p, W->ld, k, C.N, 1.0, beta, Y->p, 1, Y->ld, 0);
    }
    case OP_CSR: {
      if (op->csr->ncols != W->N || op->csr->nrows != Y->N) HFMI_FAIL(HFMI_ERR_INVALID, "csr operator / block shape mismatch");
      if (beta != 0.0 && beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
      return launch_csr_spmm(ctx, op->csr, W->p, W->ld, Y->p, Y->ld, k, beta != 0.0);
    }
    case OP_CSR_PCG: {
      if (beta != 0.0) {
        hfmi_block* T = nullptr;
        HFMI_TRY(ctx_tmp_block(ctx, 13, W->N, k, &T));
        HFMI_TRY(pcg_solve(op, W, T));
        if (beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
        return launch_axpy(ctx, Y->p, Y->ld, 1.0, T->p, T->ld, Y->N, k);
      }
      return pcg_solve(op, W, Y);
    }
    case OP_AMG_PCG: {
      if (beta != 0.0) {
        hfmi_block* T = nullptr;
        HFMI_TRY(ctx_tmp_block(ctx, 13, W->N, k, &T));
        hfmi_block tv = *T;
        tv.nvec = k;
        HFMI_TRY(amg_pcg_solve(op, W, &tv));
        if (beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
        return launch_axpy(ctx, Y->p, Y->ld, 1.0, T->p, T->ld, Y->N, k);
      }
      return amg_pcg_solve(op, W, Y);
    }
    case OP_COMPOSE3: {
      // a composition inside a composition (M C M with C = A^-1 M A^-1 itself composed) takes its own pair of temporaries
      const int depth = ctx->compose_depth;
      if (depth >= 4) HFMI_FAIL(HFMI_ERR_INVALID, "compose3: operators nested more than 4 deep");
      struct depth_guard {
        hfmi_ctx* c;
        ~depth_guard() { --c->compose_depth; }
      } guard{ctx};
      ++ctx->compose_depth;
      const int slot = depth == 0 ? 14 : 14 + 2 * depth + 2;
      hfmi_block *T1, *T2;
      HFMI_TRY(ctx_tmp_block(ctx, slot, W->N, k, &T1));
      HFMI_TRY(ctx_tmp_block(ctx, slot + 1, W->N, k, &T2));
      hfmi_block v1 = *T1, v2 = *T2;
      v1.nvec = k;
      v2.nvec = k;
      HFMI_TRY(hfmi_op_apply(op->a, W, &v1, 0));
      HFMI_TRY(hfmi_op_apply(op->b, &v1, &v2, 0));
      if (beta == 0.0) return hfmi_op_apply(op->c, &v2, Y, 0);
      HFMI_TRY(hfmi_op_apply(op->c, &v2, &v1, 0));
      if (beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
      return launch_axpy(ctx, Y->p, Y->ld, 1.0, v1.p, v1.ld, Y->N, k);
    }
    case OP_HOST: {
      const int64_t N = W->N;
      if (op->host_N > 0 && op->host_N != N) HFMI_FAIL(HFMI_ERR_INVALID, "host operator acts on vectors of length %lld, got %lld", (long long)op->host_N, (long long)N);
      hfmi_block* dst = Y;
      hfmi_block tmpv;
      if (beta != 0.0) {
        hfmi_block* T = nullptr;
        HFMI_TRY(ctx_tmp_block(ctx, 13, Y->N, k, &T));
        tmpv = *T;
        tmpv.nvec = k;
        dst = &tmpv;
      }
      HFMI_TRY(host_apply_pipelined(op, W, dst));
      if (beta == 0.0) return HFMI_OK;
      if (beta != 1.0) HFMI_TRY(launch_scale(ctx, Y->p, Y->ld, Y->N, k, beta));
      return launch_axpy(ctx, Y->p, Y->ld, 1.0, dst->p, dst->ld, Y->N, k);
    }
  }
  HFMI_FAIL(HFMI_ERR_INVALID, "unknown operator kind");
}

extern "C" int hfmi_op_apply(hfmi_op* op, const hfmi_block* W, hfmi_block* Y, int accumulate) {
  if (!op || !W || !Y) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (W->nvec != Y->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "x and y have non-matching number of vectors (%d vs %d)", W->nvec, Y->nvec);
  if (W->p == Y->p) HFMI_FAIL(HFMI_ERR_INVALID, "op_apply: input and output blocks must not alias");
  HIP_TRY(hipSetDevice(op->ctx->device));
  if (accumulate && (op->post_fn || op->comm)) HFMI_FAIL(HFMI_ERR_INVALID, "op_apply: accumulate with a rank reduction attached is ambiguous");
  op->reduced_by_panels = false;
  HFMI_TRY(op_apply_raw(op, W, Y, accumulate ? 1.0 : 0.0));
  if (op->comm && !op->reduced_by_panels) {
    const int ph = phase_begin(op->ctx, HFMI_PHASE_ALLREDUCE);
    HFMI_TRY(comm_allreduce_device(op->comm, Y->p, Y->ld * (int64_t)Y->nvec, op->comm_op));
    phase_end(op->ctx, ph);
  }
  if (op->post_fn) {
    const int rc = op->post_fn(op->post_user, Y);
    if (rc != 0) HFMI_FAIL(HFMI_ERR_CALLBACK, "post-apply hook returned %d", rc);
  }
  return HFMI_OK;
}

// ------------------------------------------------------------------ QR
// deferred (optional): if non-null and B == null, the LAST pass (the one whose input is already orthonormal to 1e-2 and
// needs no shift) does not apply its R^-1: *deferred = true and R^-1 stays in SM_RINV for the caller to fold into
// the small matrices downstream (Q = Q_in R^-1 is never formed: one N x k x k contraction less).
// opt (optional, fused solves only): do not stop the stream for the decisions of the SECOND pass.  When the first pass needed no
// shift, the second one is assumed to be the last (deferred R^-1, as above); its status words and the R_jj / ||z_j|| table are
// copied to pinned memory in stream order and verified by the caller after the synchronisation it needs anyway for the
// eigenvalues.  If the assumption was wrong the caller repeats the solve on the checked path.  (Two host round trips of ~60 us
// each per solve: 1.4 % of the 64-sample shard step.)
static_assert(sizeof(hfmi_status_words) <= 128, "two sets of status words share the first 256 bytes of the late-check buffer");
struct qr_late_checks {
  bool used;
  hfmi_status_words* st2;   // pinned
  double* aux;              // pinned, SM_LD + k doubles
  int k;
  hfmi_status_words* st1;   // pinned: status words of the FIRST pass when that one was taken on trust as well
  bool first_trusted;
};
static int qr_chol(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, bool want_r, int* passes_out, bool* deferred = nullptr,
                   qr_late_checks* opt = nullptr) {
  hfmi_ctx* ctx = Q->ctx;
  const int64_t N = Q->N;
  const int k = Q->nvec;
  if (k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: at most %d vectors (got %d)", SM_MAXK, k);
  hfmi_block* BZ = nullptr;
  hfmi_block bz_view;
  if (B) {
    if (BQ) {
      BZ = BQ;
    } else {
      HFMI_TRY(ctx_tmp_block(ctx, 4, N, k, &BZ));
      bz_view = *BZ;
      bz_view.nvec = k;
      BZ = &bz_view;
    }
  }
  const double u = 1.1102230246251565e-16;
  const double shift_rel = 11.0 * ((double)N * k + (double)k * (k + 1)) * u;
  // Breakdown threshold on pivot / (original diagonal): only pivots that are round-off noise (64 k eps) trigger the
  // shifted factorisation.  A pass with small but genuine pivots leaves a defect ~ eps / min pivot ratio, which the
  // next pass measures (st.gram_dev) and removes -- a more cautious threshold (100 k sqrt(N) u) cost config 3 a whole
  // extra pass (shifted first pass, cond(Q1) ~ 260) without making the result more accurate.
  const double pivot_tol = 0.0;   // launch_chol_inv default: 64 k eps
  int passes = 0;
  const int max_passes = 6;
  bool first_pass_clean = false;
  if (g_qr_trust_first < 0) {
    const char* e = getenv("HFMI_QR_TRUST_FIRST");
    g_qr_trust_first = (e && e[0] == '0') ? 0 : 1;
  }
  const bool trust_first = g_qr_trust_first != 0;
  for (;;) {
    const hfmi_block* right = Q;
    if (B) {
      HFMI_TRY(hfmi_op_apply(B, Q, BZ, 0));
      right = BZ;
    }
    HFMI_TRY(launch_tsgemm_tn(ctx, Q->p, Q->ld, k, right->p, right->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_GRAM), SM_LD, 1, 0));
    const int rtot_mode = (passes == 0) ? 1 : 2;   // always track R = R_p ... R_1: its diagonal exposes dependent columns
    if (deferred && !B && passes == 0 && opt && trust_first) {
      // The first pass on trust too: its status words go to their own slot (nothing overwrites them), Q <- Q R^-1 follows at
      // once and NO host round trip interrupts the solve -- the host runs ahead of the device from here to the final
      // synchronisation, so the small kernels of the tail are queued back to back.  The words are read with the second
      // pass's (below); a shifted / failed first pass sends the whole solve to the checked path (double_pass_impl).
      hfmi_status_words* const keep = ctx->status_dev;
      ctx->status_dev = keep + 1;
      const int cs = launch_chol_inv(ctx, k, SM_GRAM, SM_R, SM_RINV, SM_RTOT, rtot_mode, want_r ? 1 : 0, shift_rel, pivot_tol);
      ctx->status_dev = keep;
      HFMI_TRY(cs);
      HFMI_TRY(launch_nn_upper(ctx, Q->p, Q->ld, k, sm_ptr(ctx, SM_RINV), SM_LD, k, Q->p, Q->ld, N));
      opt->first_trusted = true;
      first_pass_clean = true;
      ++passes;
      continue;
    }
    HFMI_TRY(launch_chol_inv(ctx, k, SM_GRAM, SM_R, SM_RINV, SM_RTOT, rtot_mode, want_r ? 1 : 0, shift_rel, pivot_tol));
    hfmi_status_words st;
    if (deferred && !B && passes == 1 && opt && first_pass_clean) {
      HFMI_TRY(side_copies_begin(ctx));
      if (opt->first_trusted)
        HIP_TRY(hipMemcpyAsync(opt->st1, ctx->status_dev + 1, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
      HIP_TRY(hipMemcpyAsync(opt->st2, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
      HIP_TRY(hipMemcpyAsync(opt->aux, sm_ptr(ctx, SM_AUX), ((size_t)SM_LD + k) * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream));
      HFMI_TRY(side_copies_end(ctx));                      // the eigensolver (next writer of the status words) waits for ev_side
      opt->used = true;
      opt->k = k;
      ++passes;
      *deferred = true;
      if (passes_out) *passes_out = passes;
      return HFMI_OK;                                    // the checks below are the caller's, after its own synchronisation
    }
    if (deferred && !B && passes >= 1) {
      // candidate last pass: look at the status words first (the read-back is not hidden here) and stop WITHOUT
      // applying R^-1 if this pass would have been the last one anyway
      HFMI_TRY(read_status(ctx, &st));
      if (st.failed) HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: Gram matrix not positive definite even after shifting (pass %d)", passes + 1);
      if (!st.shifted && st.gram_dev < 1e-2) {
        ++passes;
        *deferred = true;
        break;
      }
      HFMI_TRY(launch_nn_upper(ctx, Q->p, Q->ld, k, sm_ptr(ctx, SM_RINV), SM_LD, k, Q->p, Q->ld, N));
    } else {
      // snapshot the status words on the auxiliary stream and enqueue Q <- Q R^-1 BEFORE waiting for them: the host
      // round trip then overlaps the contraction.  If the factorisation failed, R^-1 was never written by this pass
      // and Q is about to be discarded anyway (the callers restore / recompute the block on HFMI_ERR_NUMERIC).
      HFMI_TRY(read_status_begin(ctx));
      HFMI_TRY(launch_nn_upper(ctx, Q->p, Q->ld, k, sm_ptr(ctx, SM_RINV), SM_LD, k, Q->p, Q->ld, N));
      HFMI_TRY(read_status_finish(ctx, &st));
      if (st.failed) HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: Gram matrix not positive definite even after shifting (pass %d)", passes + 1);
      if (passes == 0) first_pass_clean = !st.shifted;
    }
    ++passes;
    // The input of this pass had orthonormality defect st.gram_dev (column-scaled).  If it was already
    // small and no shift was needed, the output is orthonormal to round-off: done.
    if (passes >= 2 && !st.shifted && st.gram_dev < 1e-2) break;
    if (passes >= max_passes) HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: no convergence in %d Cholesky-QR passes (defect %.2e)", passes, st.gram_dev);
  }
  // The reference's MGS zeroes a column whose norm drops below 10 eps of its pre-sweep norm
  // (numerically dependent); Cholesky-QR would instead normalise round-off noise.  R_jj / ||z_j|| is that
  // drop: hand such blocks to the Gram-Schmidt route, which reproduces the reference's behaviour.
  {
    std::vector<double> aux((size_t)SM_LD + k);       // [0, k): original column norms; [SM_LD, SM_LD + k): diag(R)
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_AUX), (size_t)SM_LD + k, aux.data()));
    for (int j = 0; j < k; ++j)
      if (!(aux[SM_LD + j] > 100.0 * 2.220446049250313e-16 * aux[j]))
        HFMI_FAIL(HFMI_ERR_NUMERIC, "borth_qr: vector %d is numerically dependent on its predecessors (R_jj/||z_j|| = %.2e)", j,
                  aux[j] > 0 ? aux[SM_LD + j] / aux[j] : 0.0);
  }
  (void)want_r;
  if (B && BQ) HFMI_TRY(hfmi_op_apply(B, Q, BQ, 0));
  if (passes_out) *passes_out = passes;
  return HFMI_OK;
}

// Column-by-column Gram-Schmidt with the reference's re-orthogonalisation rule (hippylib
// MultiVector._mgs_stable / _mgs_reortho as restated in oracle/hippylib_restated.py): each sweep projects
// column j against all previous columns at once (classical GS per sweep; with the "twice is enough"
// repetition this is as stable as the modified variant) and repeats while 10 eps t < ||q|| < t/10.
static int qr_mgs(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* R_host /* k*k or null */, int* passes_out) {
  hfmi_ctx* ctx = Q->ctx;
  const int64_t N = Q->N;
  const int k = Q->nvec;
  const double eps = 2.220446049250313e-16;
  hfmi_block* BZ = nullptr;
  hfmi_block bz_view;
  if (B) {
    if (BQ) BZ = BQ;
    else {
      HFMI_TRY(ctx_tmp_block(ctx, 4, N, k, &BZ));
      bz_view = *BZ;
      bz_view.nvec = k;
      BZ = &bz_view;
    }
  }
  std::vector<double> R((size_t)k * k, 0.0), s(k);
  void* dv = nullptr;
  // its own slot: hfmi_op_apply(B, ...) inside the column loop may regrow WS_G (Gram-form / composed / PCG operators)
  HFMI_TRY(ctx_ws(ctx, WS_MGS, (size_t)(k + 16) * 16 * sizeof(double), &dv));
  double* dsmall = (double*)dv;  // device scratch: coefficient column (ld 16) / scalars
  int total_sweeps = 0;
  for (int j = 0; j < k; ++j) {
    hfmi_block qj = *Q;
    qj.p = Q->p + (int64_t)j * Q->ld;
    qj.nvec = 1;
    hfmi_block bqj = qj;
    if (B) {
      bqj = *BZ;
      bqj.p = BZ->p + (int64_t)j * BZ->ld;
      bqj.nvec = 1;
      HFMI_TRY(hfmi_op_apply(B, &qj, &bqj, 0));
    }
    double t2 = 0.0;
    HFMI_TRY(launch_col_dots(ctx, bqj.p, bqj.ld, qj.p, qj.ld, N, 1, dsmall));
    HFMI_TRY(read_back(ctx, dsmall, 1, &t2));
    double t = sqrt(std::max(t2, 0.0));
    double tt = t;
    bool again = true;
    while (again) {
      ++total_sweeps;
      if (j > 0) {
        // s = (B Q_prev)^T q_j
        const double* left = B ? BZ->p : Q->p;
        const int64_t ldl = B ? BZ->ld : Q->ld;
        HFMI_TRY(launch_tsgemm_tn(ctx, left, ldl, j, qj.p, qj.ld, 1, N, 1.0, 0.0, dsmall, 16, 1, 0));
        std::vector<double> tmp((size_t)j * 16);
        HFMI_TRY(read_back(ctx, dsmall, (size_t)j * 16, tmp.data()));
        for (int i = 0; i < j; ++i) {
          s[i] = tmp[(size_t)i * 16];
          R[(size_t)i * k + j] += s[i];
        }
        // q_j -= Q_prev s   (the device copy of s already sits in dsmall with ld 16)
        HFMI_TRY(launch_tsgemm_nn(ctx, Q->p, Q->ld, j, dsmall, 16, 1, -1.0, 1.0, qj.p, qj.ld, N));
      }
      if (B) HFMI_TRY(hfmi_op_apply(B, &qj, &bqj, 0));
      double tt2 = 0.0;
      HFMI_TRY(launch_col_dots(ctx, bqj.p, bqj.ld, qj.p, qj.ld, N, 1, dsmall));
      HFMI_TRY(read_back(ctx, dsmall, 1, &tt2));
      tt = sqrt(std::max(tt2, 0.0));
      if (tt > t * 10.0 * eps && tt < t / 10.0) {
        again = true;
        t = tt;
      } else {
        again = false;
        if (tt < 10.0 * eps * t) tt = 0.0;
      }
    }
    R[(size_t)j * k + j] = tt;
    const double inv = (fabs(tt * eps) > 0.0) ? 1.0 / tt : 0.0;
    HFMI_TRY(launch_scale(ctx, qj.p, qj.ld, N, 1, inv));
    if (B) HFMI_TRY(launch_scale(ctx, bqj.p, bqj.ld, N, 1, inv));
  }
  if (R_host) memcpy(R_host, R.data(), (size_t)k * k * sizeof(double));
  if (passes_out) *passes_out = total_sweeps;
  return HFMI_OK;
}

// want_r: exact triangular factors in every Cholesky pass.  Without it a pass whose input is already orthonormal to ~1e-7
// takes the kernel's first-order inverse square root, which left a 74-column single-pass sketch orthonormal to only ~1e-10.
static int borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, bool want_r, int method, int* passes);
extern "C" int hfmi_borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, int method, int* passes) {
  return borth_qr(Q, B, BQ, host_R, host_R != nullptr, method, passes);
}
static int borth_qr(hfmi_block* Q, hfmi_op* B, hfmi_block* BQ, double* host_R, bool want_r, int method, int* passes) {
  if (!Q) HFMI_FAIL(HFMI_ERR_INVALID, "null block");
  if (BQ) HFMI_TRY(check_same_shape(Q, BQ, "borth_qr"));
  if (BQ && !B) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: BQ requested without B");
  hfmi_ctx* ctx = Q->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int k = Q->nvec;
  if (method == HFMI_QR_MGS) return qr_mgs(Q, B, BQ, host_R, passes);
  if (method != HFMI_QR_CHOL && method != HFMI_QR_AUTO) HFMI_FAIL(HFMI_ERR_INVALID, "borth_qr: unknown method %d", method);
  hfmi_block* save = nullptr;
  if (method == HFMI_QR_AUTO) {  // keep the input so that a breakdown can fall back to Gram-Schmidt
    HFMI_TRY(ctx_tmp_block(ctx, 5, Q->N, k, &save));
    HFMI_TRY(launch_copy(ctx, save->p, save->ld, Q->p, Q->ld, Q->N, k));
  }
  int s = qr_chol(Q, B, BQ, want_r, passes);
  if (s == HFMI_ERR_NUMERIC && method == HFMI_QR_AUTO) {
    HFMI_TRY(launch_copy(ctx, Q->p, Q->ld, save->p, save->ld, Q->N, k));
    return qr_mgs(Q, B, BQ, host_R, passes);
  }
  if (s != HFMI_OK) return s;
  if (host_R) {
    std::vector<double> tmp((size_t)k * SM_LD);
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_RTOT), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_R + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  return HFMI_OK;
}

// ------------------------------------------------------------------ Rayleigh-Ritz
extern "C" int hfmi_sym_eig_small(hfmi_ctx* ctx, const double* host_T, int k, int sort_by_abs, double* host_d, double* host_V) {
  if (!ctx || !host_T || !host_d) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > HFMI_EIG_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "sym_eig_small: k=%d out of range [1,%d]", k, HFMI_EIG_MAXN);
  HIP_TRY(hipSetDevice(ctx->device));
  if (k > SM_MAXK) return sym_eig_large(ctx, host_T, k, sort_by_abs, host_d, host_V);   // whole-GPU blocked solver (checks its input on the device)
  for (size_t i = 0; i < (size_t)k * k; ++i)
    if (!std::isfinite(host_T[i])) HFMI_FAIL(HFMI_ERR_NUMERIC, "sym_eig (n=%d): the matrix has non-finite entries", k);
  HFMI_TRY(upload_small(ctx, host_T, k, k, sm_ptr(ctx, SM_T), SM_LD));
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  HFMI_TRY(launch_sym_eig(ctx, k, SM_T, SM_V, (double*)dv, sort_by_abs & 1, (sort_by_abs >> 1) & 1));
  hfmi_status_words st;
  HFMI_TRY(read_status(ctx, &st));
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "sym_eig_small: eigensolver did not converge (off-diagonal %.2e)", st.offdiag);
  HFMI_TRY(read_back(ctx, (const double*)dv, k, host_d));
  if (host_V) {
    std::vector<double> tmp((size_t)k * SM_LD);
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_V), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_V + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  return HFMI_OK;
}

// np.linalg.svd of the small triangular factor inside hp.accuracyEnhancedSVD
// the same with only the nvec leading eigenvectors (in output order) returned: host_V is k x nvec row-major.  What the deterministic
// POD needs of la.eigh(G) (PODProjector.py:821-826: U[:, :u_rank]); beyond 256 the back-transformation and the read-back then run
// over nvec columns instead of k
extern "C" int hfmi_sym_eig_leading(hfmi_ctx* ctx, const double* host_T, int k, int sort_by_abs, int nvec, double* host_d, double* host_V) {
  if (!ctx || !host_T || !host_d || !host_V) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > HFMI_EIG_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "sym_eig_leading: k=%d out of range [1,%d]", k, HFMI_EIG_MAXN);
  if (nvec < 1 || nvec > k) HFMI_FAIL(HFMI_ERR_INVALID, "sym_eig_leading: nvec=%d out of range [1,%d]", nvec, k);
  HIP_TRY(hipSetDevice(ctx->device));
  if (k > SM_MAXK) return sym_eig_large(ctx, host_T, k, sort_by_abs, host_d, host_V, nvec);
  std::vector<double> full((size_t)k * k);
  HFMI_TRY(hfmi_sym_eig_small(ctx, host_T, k, sort_by_abs, host_d, full.data()));
  for (int i = 0; i < k; ++i) memcpy(host_V + (size_t)i * nvec, full.data() + (size_t)i * k, (size_t)nvec * sizeof(double));
  return HFMI_OK;
}

// la.eigh(X^T (M X)) of the deterministic POD in one call (PODProjector.py:818-826: UtMU = u_data @ M @ u_data.T; eigh; U[:, :u_rank]):
// the n x n Gram matrix of two blocks is formed on the device and goes straight into the eigensolver -- no n x n matrix crosses
// PCIe in either direction, only the n eigenvalues and the nvec wanted eigenvectors come back (host_V: n x nvec row-major).
extern "C" int hfmi_block_gram_eig(const hfmi_block* A, const hfmi_block* B, int sort_by_abs, int nvec, double* host_d, double* host_V) {
  if (!A || !B || !host_d || !host_V) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (A->N != B->N) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: vector lengths differ (%lld vs %lld)", (long long)A->N, (long long)B->N);
  if (A->nvec != B->nvec) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: the blocks hold %d and %d vectors", A->nvec, B->nvec);
  const int n = A->nvec;
  if (n < 1 || n > HFMI_EIG_MAXN) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: n=%d out of range [1,%d]", n, HFMI_EIG_MAXN);
  if (nvec < 1 || nvec > n) HFMI_FAIL(HFMI_ERR_INVALID, "block_gram_eig: nvec=%d out of range [1,%d]", nvec, n);
  hfmi_ctx* ctx = A->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  void* out = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)n * n * sizeof(double), &out));
  HFMI_TRY(launch_tsgemm_tn(ctx, A->p, A->ld, n, B->p, B->ld, n, A->N, 1.0, 0.0, (double*)out, n, 1, 0));
  if (n > SM_MAXK) return sym_eig_large(ctx, nullptr, n, sort_by_abs, host_d, host_V, nvec, (const double*)out);
  std::vector<double> G((size_t)n * n);
  HFMI_TRY(read_back(ctx, (const double*)out, (size_t)n * n, G.data()));
  return hfmi_sym_eig_leading(ctx, G.data(), n, sort_by_abs, nvec, host_d, host_V);
}

extern "C" int hfmi_svd_small(hfmi_ctx* ctx, const double* host_R, int k, double* host_sigma, double* host_U, double* host_V) {
  if (!ctx || !host_R || !host_sigma) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (k < 1 || k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "svd_small: k=%d out of range [1,%d]", k, SM_MAXK);
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(upload_small(ctx, host_R, k, k, sm_ptr(ctx, SM_T), SM_LD));
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  HFMI_TRY(launch_jacobi_svd(ctx, k, SM_T, SM_R, SM_V, (double*)dv));
  hfmi_status_words st;
  HFMI_TRY(read_status(ctx, &st));
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "svd_small: one-sided Jacobi did not converge (max cosine %.2e)", st.offdiag);
  HFMI_TRY(read_back(ctx, (const double*)dv, k, host_sigma));
  std::vector<double> tmp((size_t)k * SM_LD);
  if (host_U) {
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_R), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_U + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  if (host_V) {
    HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_V), (size_t)k * SM_LD, tmp.data()));
    for (int i = 0; i < k; ++i) memcpy(host_V + (size_t)i * k, tmp.data() + (size_t)i * SM_LD, (size_t)k * sizeof(double));
  }
  return HFMI_OK;
}

// ------------------------------------------------------------------ fused double pass
// Rayleigh quotient T = Q^T A Q for operators of Gram form A = scale * X^T Gamma X (snapshot Gram, mean J^T J):
//   T = scale * (X Q)^T Gamma (X Q)
// -- the same matrix as the reference's (A Q)^T Q by associativity, symmetric by construction, and it needs only the
// reduction GEMM G = X Q (no N x k block A Q, i.e. one of the four big contractions of the solve disappears).  A rank
// average attached to the operator (CollectiveOperator 'avg'/'sum') is linear, so the hook is applied to T itself: the
// second all-reduce of the solve shrinks from N x k to k x k.
static bool op_has_gram_form(const hfmi_op* A) { return (A->kind == OP_SNAPSHOT_GRAM && !A->weights) || A->kind == OP_JTJ; }

// fold_rinv: Q stands for Q R^-1 with R^-1 in SM_RINV (deferred last QR pass): X (Q R^-1) = (X Q) R^-1 is applied to
// the small m x k intermediate instead of the N x k block.
static int op_rayleigh_quotient_gram(hfmi_op* A, const hfmi_block* Q, int slot_T, bool fold_rinv = false) {
  hfmi_ctx* ctx = A->ctx;
  const hfmi_block& X = A->X;
  if (X.N != Q->N) HFMI_FAIL(HFMI_ERR_INVALID, "operator acts on vectors of length %lld, got %lld", (long long)X.N, (long long)Q->N);
  const int m = X.nvec, k = Q->nvec;
  const int64_t ldm = round_up(m, 32);
  const bool gam = (A->kind == OP_JTJ && A->gamma_inv != nullptr);
  void* gv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)ldm * k * sizeof(double) * (gam ? 2 : 1), &gv));
  double* Gc = (double*)gv;                          // (m x k), column-major: a block of k vectors of length m
  double* Gc2 = gam ? Gc + ldm * k : Gc;
  HFMI_TRY(launch_tsgemm_tn(ctx, X.p, X.ld, m, Q->p, Q->ld, k, X.N, 1.0, 0.0, Gc, 1, ldm, 0));
  HFMI_TRY(launch_zero_pad(ctx, Gc, m, k, ldm));
  if (fold_rinv) HFMI_TRY(launch_nn_upper(ctx, Gc, ldm, k, sm_ptr(ctx, SM_RINV), SM_LD, k, Gc, ldm, m));
  if (gam) {
    HFMI_TRY(launch_gamma_apply_cm(ctx, Gc, Gc2, ldm, A->ndata, A->q, k, A->gamma_inv, (int)round_up(A->q, 16)));
    HFMI_TRY(launch_zero_pad(ctx, Gc2, m, k, ldm));
  }
  HFMI_TRY(launch_tsgemm_tn(ctx, Gc, ldm, k, Gc2, ldm, k, m, A->scale, 0.0, sm_ptr(ctx, slot_T), SM_LD, 1, 0));
  if (A->comm) {
    const int ph = phase_begin(ctx, HFMI_PHASE_ALLREDUCE);
    HFMI_TRY(comm_allreduce_device(A->comm, sm_ptr(ctx, slot_T), (int64_t)SM_LD * k, A->comm_op));
    phase_end(ctx, ph);
  }
  if (A->post_fn) {
    hfmi_block t;
    t.ctx = ctx;
    t.p = sm_ptr(ctx, slot_T);
    t.N = SM_LD;
    t.nvec = k;
    t.ld = SM_LD;
    t.owner = false;
    const int rc = A->post_fn(A->post_user, &t);
    if (rc != 0) HFMI_FAIL(HFMI_ERR_CALLBACK, "post-apply hook returned %d", rc);
  }
  return HFMI_OK;
}

static int double_pass_impl(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                            double* host_d, hfmi_block* U, bool late_checks = true) {
  if (!A || !Omega || !host_d || !U) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = Omega->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t N = Omega->N;
  const int k = Omega->nvec;
  if (k < r) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: Omega has %d vectors, need at least the rank %d", k, r);
  if (r < 1) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: rank must be positive");
  if (U->N != N || U->nvec != r) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: U must be %lld x %d", (long long)N, r);
  if (k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: at most %d probe vectors (got %d)", SM_MAXK, k);
  if (s < 1) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass: s must be >= 1");
  hfmi_block *Qb, *Yb;
  HFMI_TRY(ctx_tmp_block(ctx, 0, N, k, &Qb));
  HFMI_TRY(ctx_tmp_block(ctx, 1, N, k, &Yb));
  hfmi_block Q = *Qb, Y = *Yb;
  Q.nvec = k;
  Y.nvec = k;
  // power iterations: Q <- (B^-1) A Q, starting from Omega (never modified)
  const hfmi_block* cur = Omega;
  auto power_iterations = [&]() -> int {
    cur = Omega;
    for (int it = 0; it < s; ++it) {
      if (Binv) {
        int ph = phase_begin(ctx, HFMI_PHASE_APPLY);
        HFMI_TRY(hfmi_op_apply(A, cur, &Y, 0));
        phase_end(ctx, ph);
        ph = phase_begin(ctx, HFMI_PHASE_BINV);
        HFMI_TRY(hfmi_op_apply(Binv, &Y, &Q, 0));
        phase_end(ctx, ph);
        cur = &Q;
      } else {
        hfmi_block* dst = (cur == &Q) ? &Y : &Q;
        const int ph = phase_begin(ctx, HFMI_PHASE_APPLY);
        HFMI_TRY(hfmi_op_apply(A, cur, dst, 0));
        phase_end(ctx, ph);
        cur = dst;
      }
    }
    return HFMI_OK;
  };
  HFMI_TRY(power_iterations());
  bool deferred = false;                                   // last Cholesky-QR pass left as R^-1 in SM_RINV
  qr_late_checks late = {false, nullptr, nullptr, 0, nullptr, false};
  hfmi_block* Qp = const_cast<hfmi_block*>(cur);           // holds the block to orthogonalise
  hfmi_block* AQ = (Qp == &Q) ? &Y : &Q;
  int ph = phase_begin(ctx, HFMI_PHASE_QR);
  if (flags & 2) {
    HFMI_TRY(hfmi_borth_qr(Qp, B, nullptr, nullptr, HFMI_QR_MGS, nullptr));
  } else {
    // Cholesky-QR in place WITHOUT the safety copy hfmi_borth_qr(AUTO) keeps (a pass over N x k): if a column turns
    // out to be numerically dependent, the block is recomputed from Omega (deterministic, every rank takes the same
    // branch) and handed to the reference's Gram-Schmidt rule
    const bool gram_path = op_has_gram_form(A) && !(flags & 4);
    if (gram_path && late_checks && !B) {
      void* pin = nullptr;
      HFMI_TRY(ctx_late_pinned(ctx, &pin));
      late.st2 = (hfmi_status_words*)pin;
      late.st1 = (hfmi_status_words*)((char*)pin + 128);
      late.aux = (double*)((char*)pin + 256);
    }
    const int qs = qr_chol(Qp, B, nullptr, false, nullptr, gram_path ? &deferred : nullptr, late.st2 ? &late : nullptr);
    if (qs == HFMI_ERR_NUMERIC) {
      deferred = false;
      HFMI_TRY(power_iterations());
      HFMI_TRY(hfmi_borth_qr(Qp, B, nullptr, nullptr, HFMI_QR_MGS, nullptr));
    } else if (qs != HFMI_OK) {
      return qs;
    }
  }
  phase_end(ctx, ph);
  ph = phase_begin(ctx, HFMI_PHASE_RAYLEIGH);
  if (op_has_gram_form(A) && !(flags & 4)) {
    HFMI_TRY(op_rayleigh_quotient_gram(A, Qp, SM_T, deferred));
  } else {
    // T = (AQ)^T Q as the reference forms it
    HFMI_TRY(hfmi_op_apply(A, Qp, AQ, 0));
    HFMI_TRY(launch_tsgemm_tn(ctx, AQ->p, AQ->ld, k, Qp->p, Qp->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_T), SM_LD, 1, 0));
  }
  phase_end(ctx, ph);
  // small eigensolve, U = Q V[:, :r]
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  ph = phase_begin(ctx, HFMI_PHASE_EIG);
  if (late.used) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));   // the late-check copies read the status words (done ms ago)
  HFMI_TRY(launch_sym_eig(ctx, k, SM_T, SM_V, (double*)dv, flags & 1, (flags >> 3) & 1));
  phase_end(ctx, ph);
  // eigenvalues and status words leave for the host now, beside the back-transformation, instead of behind it
  void* dpin = nullptr;
  HFMI_TRY(ctx_pinned(ctx, (size_t)r * sizeof(double), &dpin));
  HFMI_TRY(side_copies_begin(ctx));
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HIP_TRY(hipMemcpyAsync(dpin, dv, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream));
  ph = phase_begin(ctx, HFMI_PHASE_BACK);
  if (deferred) {   // U = (Q R^-1) V = Q (R^-1 V)
    HFMI_TRY(launch_small_matmul(ctx, k, r, SM_RINV, SM_V, SM_TMP2));
    HFMI_TRY(launch_tsgemm_nn(ctx, Qp->p, Qp->ld, k, sm_ptr(ctx, SM_TMP2), SM_LD, r, 1.0, 0.0, U->p, U->ld, N));
  } else {
    HFMI_TRY(launch_tsgemm_nn(ctx, Qp->p, Qp->ld, k, sm_ptr(ctx, SM_V), SM_LD, r, 1.0, 0.0, U->p, U->ld, N));
  }
  phase_end(ctx, ph);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
  memcpy(host_d, dpin, (size_t)r * sizeof(double));
  const hfmi_status_words st = *ctx->status_host;
  print_status_dbg(&st);
  if (late.used) {
    // the second orthogonalisation pass was taken on trust: look at what it reported, now that the stream has drained
    bool ok = !late.st2->failed && !late.st2->shifted && late.st2->gram_dev < 1e-2;
    if (late.first_trusted && (late.st1->failed || late.st1->shifted)) ok = false;
    for (int j = 0; j < late.k && ok; ++j)
      if (!(late.aux[SM_LD + j] > 100.0 * 2.220446049250313e-16 * late.aux[j])) ok = false;
    if (!ok) return double_pass_impl(A, B, Binv, Omega, r, s, flags, host_d, U, false);   // the checked path decides (MGS fall-back, errors)
  }
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "double_pass: small eigensolve did not converge (off-diagonal %.2e)", st.offdiag);
  return HFMI_OK;
}

extern "C" int hfmi_double_pass(hfmi_op* A, const hfmi_block* Omega, int r, int s, int flags, double* host_d, hfmi_block* U) {
  return double_pass_impl(A, nullptr, nullptr, Omega, r, s, flags, host_d, U);
}
extern "C" int hfmi_double_pass_g(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                                  double* host_d, hfmi_block* U) {
  if (!B || !Binv) HFMI_FAIL(HFMI_ERR_INVALID, "double_pass_g: B and Binv are required");
  return double_pass_impl(A, B, Binv, Omega, r, s, flags, host_d, U);
}

// ------------------------------------------------------------------ fused single pass
// hippylib's singlePass / singlePassG (randomizedEigensolver): the Rayleigh-Ritz matrix comes from the sketch itself instead of
// a further application of the operator.  With P = X_{s-1}, Y = X_s (X_0 = Omega, X_i = (B^-1) A X_{i-1}) and Q an
// orthonormal (B-orthonormal) basis of range(Y):
//   A ~ Q T Q^T (B Q T Q^T B)  =>  Q^T B Y = T (Q^T B P)  =>  Wt T^T = Zt,  Wt = P^T (B Q),  Zt = Ybar^T Q
// (Ybar = A X_{s-1}; Ybar = Y without B), so T^T = Wt^-1 Zt, symmetrised.  The core below works on a sketch the caller
// holds (hfmi_sketch_eig, streamed sketches) or the one single_pass_impl has just built: Q = orth(Y) with the same
// Cholesky-QR / Gram-Schmidt rule as the double pass, the two m x m products, the LU solve (k_lu_solve writes T straight
// into the eigensolver's slot), the eigensolve and U = Q V[:, :r], all on the context's stream.  The host waits only where the
// double pass's checked route does (the status words of each orthogonalisation pass) and once at the end.
// Q_work may alias Y for the generalized problem (Y itself is not needed after its orthogonalisation there).
static int sketch_eig_core(const hfmi_block* P, const hfmi_block* Y, const hfmi_block* Ybar, hfmi_op* B, hfmi_block* Q_work,
                           hfmi_block* BQ_work, int r, int flags, double* host_d, hfmi_block* U, const char* who) {
  hfmi_ctx* ctx = P->ctx;
  const int64_t N = P->N;
  const int k = P->nvec;
  if (Q_work->p != Y->p) HFMI_TRY(launch_copy(ctx, Q_work->p, Q_work->ld, Y->p, Y->ld, N, k));
  int ph = phase_begin(ctx, HFMI_PHASE_QR);
  // exact triangular factors in every pass (want_r, see borth_qr), nothing read back: U = Q V orthonormal to round-off
  HFMI_TRY(borth_qr(Q_work, B, B ? BQ_work : nullptr, nullptr, true, (flags & 2) ? HFMI_QR_MGS : HFMI_QR_AUTO, nullptr));
  phase_end(ctx, ph);
  ph = phase_begin(ctx, HFMI_PHASE_RAYLEIGH);
  const hfmi_block* right = B ? BQ_work : Q_work;
  const hfmi_block* left = B ? Ybar : Y;
  HFMI_TRY(launch_tsgemm_tn(ctx, P->p, P->ld, k, right->p, right->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_GRAM), SM_LD, 1, 0));
  HFMI_TRY(launch_tsgemm_tn(ctx, left->p, left->ld, k, Q_work->p, Q_work->ld, k, N, 1.0, 0.0, sm_ptr(ctx, SM_R), SM_LD, 1, 0));
  HFMI_TRY(launch_lu_solve(ctx, k, SM_GRAM, SM_R, SM_TMP, SM_TMP2, SM_T));
  phase_end(ctx, ph);
  // the solve's status words leave for pinned memory before the eigensolver reuses them
  void* pin = nullptr;
  HFMI_TRY(ctx_late_pinned(ctx, &pin));
  hfmi_status_words* lu_st = (hfmi_status_words*)pin;
  HFMI_TRY(side_copies_begin(ctx));
  HIP_TRY(hipMemcpyAsync(lu_st, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HFMI_TRY(side_copies_end(ctx));
  HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));
  void* dv = nullptr;
  HFMI_TRY(ctx_ws(ctx, WS_G, (size_t)SM_MAXK * sizeof(double), &dv));
  ph = phase_begin(ctx, HFMI_PHASE_EIG);
  HFMI_TRY(launch_sym_eig(ctx, k, SM_T, SM_V, (double*)dv, flags & 1, (flags >> 3) & 1));
  phase_end(ctx, ph);
  void* dpin = nullptr;
  HFMI_TRY(ctx_pinned(ctx, (size_t)r * sizeof(double), &dpin));
  HFMI_TRY(side_copies_begin(ctx));
  HIP_TRY(hipMemcpyAsync(ctx->status_host, ctx->status_dev, sizeof(hfmi_status_words), hipMemcpyDeviceToHost, ctx->aux_stream));
  HIP_TRY(hipMemcpyAsync(dpin, dv, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, ctx->aux_stream));
  ph = phase_begin(ctx, HFMI_PHASE_BACK);
  // V[:, :r] zero padded to 16 columns, as tsgemm_nn expects (the eigensolver leaves SM_V's pad columns as they were)
  HFMI_TRY(launch_small_set_identity(ctx, k, SM_GRAM));
  HFMI_TRY(launch_small_matmul(ctx, k, r, SM_GRAM, SM_V, SM_TMP2));
  HFMI_TRY(launch_tsgemm_nn(ctx, Q_work->p, Q_work->ld, k, sm_ptr(ctx, SM_TMP2), SM_LD, r, 1.0, 0.0, U->p, U->ld, N));
  phase_end(ctx, ph);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
  HFMI_TRY(ctx_check_comm(ctx));
  if (lu_st->failed == 1) HFMI_FAIL(HFMI_ERR_NUMERIC, "%s: the sketch products W = P^T Q / Z = Y^T Q have non-finite entries", who);
  if (lu_st->failed == 3) HFMI_FAIL(HFMI_ERR_NUMERIC, "%s: the solve W^-1 Z overflowed (non-finite pivot or solution)", who);
  if (lu_st->failed)
    HFMI_FAIL(HFMI_ERR_NUMERIC, "%s: rank-deficient sketch: W = P^T %sQ is singular (min |pivot| %.2e, max |pivot| %.2e); "
              "the probe block has dependent columns or the operator's range is smaller than the sketch", who, B ? "B " : "",
              lu_st->min_pivot_ratio, lu_st->gram_dev);
  memcpy(host_d, dpin, (size_t)r * sizeof(double));
  const hfmi_status_words st = *ctx->status_host;
  print_status_dbg(&st);
  if (st.failed) HFMI_FAIL(HFMI_ERR_NOT_CONVERGED, "%s: small eigensolve did not converge (off-diagonal %.2e)", who, st.offdiag);
  return HFMI_OK;
}

static int check_sketch_args(const hfmi_block* Omega, int r, const hfmi_block* U, const char* who) {
  const int k = Omega->nvec;
  if (r < 1) HFMI_FAIL(HFMI_ERR_INVALID, "%s: rank must be positive", who);
  if (k < r) HFMI_FAIL(HFMI_ERR_INVALID, "%s: the sketch has %d vectors, need at least the rank %d", who, k, r);
  if (k > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "%s: at most %d probe vectors (got %d)", who, SM_MAXK, k);
  if (U->N != Omega->N || U->nvec != r) HFMI_FAIL(HFMI_ERR_INVALID, "%s: U must be %lld x %d (got %lld x %d)", who, (long long)Omega->N, r,
                                                  (long long)U->N, U->nvec);
  return HFMI_OK;
}

static int single_pass_impl(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags, double* host_d,
                            hfmi_block* U) {
  const char* who = B ? "single_pass_g" : "single_pass";
  if (!A || !Omega || !host_d || !U) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  hfmi_ctx* ctx = Omega->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(check_sketch_args(Omega, r, U, who));
  if (s < 1) HFMI_FAIL(HFMI_ERR_INVALID, "%s: s must be >= 1", who);
  const int64_t N = Omega->N;
  const int k = Omega->nvec;
  hfmi_block *b0, *b1, *b2, *b3 = nullptr;
  HFMI_TRY(ctx_tmp_block(ctx, 0, N, k, &b0));
  HFMI_TRY(ctx_tmp_block(ctx, 1, N, k, &b1));
  HFMI_TRY(ctx_tmp_block(ctx, 2, N, k, &b2));
  if (B) HFMI_TRY(ctx_tmp_block(ctx, 3, N, k, &b3));
  hfmi_block X0 = *b0, X1 = *b1, W2 = *b2, W3;
  X0.nvec = X1.nvec = W2.nvec = k;
  if (B) {
    W3 = *b3;
    W3.nvec = k;
  }
  // power iterations without orthogonalisation (the loop of double_pass_impl); the last two iterates are kept
  const hfmi_block* prev = Omega;
  const hfmi_block* cur = Omega;
  for (int it = 0; it < s; ++it) {
    hfmi_block* dst = (cur == &X0) ? &X1 : &X0;
    if (Binv) {
      int ph = phase_begin(ctx, HFMI_PHASE_APPLY);
      HFMI_TRY(hfmi_op_apply(A, cur, &W2, 0));                 // Ybar
      phase_end(ctx, ph);
      ph = phase_begin(ctx, HFMI_PHASE_BINV);
      HFMI_TRY(hfmi_op_apply(Binv, &W2, dst, 0));
      phase_end(ctx, ph);
    } else {
      const int ph = phase_begin(ctx, HFMI_PHASE_APPLY);
      HFMI_TRY(hfmi_op_apply(A, cur, dst, 0));
      phase_end(ctx, ph);
    }
    prev = cur;
    cur = dst;
  }
  hfmi_block* Yb = const_cast<hfmi_block*>(cur);
  if (B) return sketch_eig_core(prev, Yb, &W2, B, Yb, &W3, r, flags, host_d, U, who);   // Q in place of Y, B Q in W3
  return sketch_eig_core(prev, Yb, nullptr, nullptr, &W2, nullptr, r, flags, host_d, U, who);
}

extern "C" int hfmi_single_pass(hfmi_op* A, const hfmi_block* Omega, int r, int s, int flags, double* host_d, hfmi_block* U) {
  return single_pass_impl(A, nullptr, nullptr, Omega, r, s, flags, host_d, U);
}
extern "C" int hfmi_single_pass_g(hfmi_op* A, hfmi_op* B, hfmi_op* Binv, const hfmi_block* Omega, int r, int s, int flags,
                                  double* host_d, hfmi_block* U) {
  if (!B || !Binv) HFMI_FAIL(HFMI_ERR_INVALID, "single_pass_g: B and Binv are required");
  return single_pass_impl(A, B, Binv, Omega, r, s, flags, host_d, U);
}

extern "C" int hfmi_sketch_eig(const hfmi_block* P, const hfmi_block* Y, const hfmi_block* Ybar, hfmi_op* B, int r, int flags,
                               double* host_d, hfmi_block* U) {
  if (!P || !Y || !host_d || !U) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (!Ybar != !B) HFMI_FAIL(HFMI_ERR_INVALID, "sketch_eig: Ybar and B go together (generalized problem) or are both absent");
  HFMI_TRY(check_same_shape(P, Y, "sketch_eig"));
  if (Ybar) HFMI_TRY(check_same_shape(P, Ybar, "sketch_eig"));
  hfmi_ctx* ctx = P->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(check_sketch_args(P, r, U, "sketch_eig"));
  const int64_t N = P->N;
  const int k = P->nvec;
  hfmi_block *b2, *b3 = nullptr;
  HFMI_TRY(ctx_tmp_block(ctx, 2, N, k, &b2));
  if (B) HFMI_TRY(ctx_tmp_block(ctx, 3, N, k, &b3));
  hfmi_block Qw = *b2, BQw;
  Qw.nvec = k;
  if (B) {
    BQw = *b3;
    BQw.nvec = k;
  }
  return sketch_eig_core(P, Y, Ybar, B, &Qw, B ? &BQw : nullptr, r, flags, host_d, U, "sketch_eig");
}

// np.linalg.solve(W, Z) of the single-pass methods on the device, host in and host out (kernel tests)
extern "C" int hfmi_small_solve(hfmi_ctx* ctx, const double* host_W, const double* host_Z, int m, double* host_X) {
  if (!ctx || !host_W || !host_Z || !host_X) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  if (m < 1 || m > SM_MAXK) HFMI_FAIL(HFMI_ERR_INVALID, "small_solve: m=%d out of range [1,%d]", m, SM_MAXK);
  HIP_TRY(hipSetDevice(ctx->device));
  HFMI_TRY(upload_small(ctx, host_W, m, m, sm_ptr(ctx, SM_GRAM), SM_LD));
  HFMI_TRY(upload_small(ctx, host_Z, m, m, sm_ptr(ctx, SM_R), SM_LD));
  HFMI_TRY(launch_lu_solve(ctx, m, SM_GRAM, SM_R, SM_TMP, SM_TMP2, -1));
  hfmi_status_words st;
  HFMI_TRY(read_status(ctx, &st));
  if (st.failed == 1) HFMI_FAIL(HFMI_ERR_NUMERIC, "small_solve (m=%d): non-finite input", m);
  if (st.failed == 3) HFMI_FAIL(HFMI_ERR_NUMERIC, "small_solve (m=%d): the elimination overflowed (non-finite pivot or solution)", m);
  if (st.failed) HFMI_FAIL(HFMI_ERR_NUMERIC, "small_solve (m=%d): the matrix is singular (min |pivot| %.2e, max |pivot| %.2e)", m,
                           st.min_pivot_ratio, st.gram_dev);
  std::vector<double> tmp((size_t)m * SM_LD);
  HFMI_TRY(read_back(ctx, sm_ptr(ctx, SM_TMP2), (size_t)m * SM_LD, tmp.data()));
  for (int i = 0; i < m; ++i) memcpy(host_X + (size_t)i * m, tmp.data() + (size_t)i * SM_LD, (size_t)m * sizeof(double));
  return HFMI_OK;
}

// ------------------------------------------------------------------ instrumentation
int prof_start(hfmi_ctx* ctx, int kind, int64_t m, int64_t k, int64_t N) {
  if (!ctx->profiling) return -1;
  if (g_prof_level < 2 && 2.0 * (double)N * (double)m * (double)k < 2.0e9) return -1;
  hfmi_ctx::prof_rec r;
  r.kind = kind;
  r.m = m;
  r.k = k;
  r.N = N;
  // algorithmic work (each operand touched once): flops 2 N m k, bytes 8 (N m + N k + m k)
  r.flops = 2.0 * (double)N * (double)m * (double)k;
  r.bytes = 8.0 * ((double)N * m + (double)N * k + (double)m * k);
  if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
  (void)hipEventRecord(r.e0, ctx->stream);
  ctx->prof.push_back(r);
  return (int)ctx->prof.size() - 1;
}
int prof_stop(hfmi_ctx* ctx, int idx) {
  if (idx >= 0) (void)hipEventRecord(ctx->prof[idx].e1, ctx->stream);
  return HFMI_OK;
}
static int phase_begin_on(hfmi_ctx* ctx, int phase, hipStream_t st) {
  if (!ctx->profiling || g_prof_level < 2) return -1;
  hfmi_ctx::phase_rec r;
  r.phase = phase;
  if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
  (void)hipEventRecord(r.e0, st);
  ctx->phase_events.push_back(r);
  return (int)ctx->phase_events.size() - 1;
}
static void phase_end_on(hfmi_ctx* ctx, int idx, hipStream_t st) {
  if (idx >= 0) (void)hipEventRecord(ctx->phase_events[idx].e1, st);
}
int phase_begin(hfmi_ctx* ctx, int phase) { return phase_begin_on(ctx, phase, ctx->stream); }
void phase_end(hfmi_ctx* ctx, int idx) { phase_end_on(ctx, idx, ctx->stream); }
extern "C" int hfmi_profile_phases(hfmi_ctx* ctx, double* ms_out) {
  if (!ctx || !ms_out) HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  for (int i = 0; i < HFMI_PHASE_COUNT; ++i) ms_out[i] = ctx->phase_ms[i];
  return HFMI_OK;
}
extern "C" int hfmi_profile_begin(hfmi_ctx* ctx) {
  if (!ctx) HFMI_FAIL(HFMI_ERR_INVALID, "null ctx");
  for (auto& r : ctx->prof) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  ctx->prof.clear();
  for (auto& r : ctx->phase_events) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  ctx->phase_events.clear();
  for (int i = 0; i < HFMI_PHASE_COUNT; ++i) ctx->phase_ms[i] = 0.0;
  ctx->profiling = true;
  return HFMI_OK;
}
extern "C" int hfmi_profile_end(hfmi_ctx* ctx, int max_groups, int* ngroups, int* kind, int64_t* shape, double* ms,
                                int64_t* launches, double* flops_per_launch, double* bytes_per_launch) {
  if (!ctx || !ngroups || !kind || !shape || !ms || !launches || !flops_per_launch || !bytes_per_launch)
    HFMI_FAIL(HFMI_ERR_INVALID, "null argument");
  ctx->profiling = false;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  int ng = 0;
  for (auto& r : ctx->prof) {
    float t = 0.f;
    const bool ok = hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess;
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    if (!ok) continue;
    int g = 0;
    for (; g < ng; ++g)
      if (kind[g] == r.kind && shape[3 * g] == r.m && shape[3 * g + 1] == r.k && shape[3 * g + 2] == r.N) break;
    if (g == ng) {
      if (ng >= max_groups) continue;
      kind[g] = r.kind;
      shape[3 * g] = r.m;
      shape[3 * g + 1] = r.k;
      shape[3 * g + 2] = r.N;
      ms[g] = 0.0;
      launches[g] = 0;
      flops_per_launch[g] = r.flops;
      bytes_per_launch[g] = r.bytes;
      ++ng;
    }
    ms[g] += t;
    launches[g] += 1;
  }
  ctx->prof.clear();
  for (auto& r : ctx->phase_events) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) ctx->phase_ms[r.phase] += t;
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  ctx->phase_events.clear();
  *ngroups = ng;
  return HFMI_OK;
}
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
// C (M x N) = op(A) op(B) on the device's general fp64 MFMA product (hfmi_eig_blocked.hip), host column-major operands in and out: the two
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
extern "C" int hfmi_ctx_pci_bus_id(hfmi_ctx* ctx, char* buf, int len) {
  if (!ctx || !buf || len < 16) HFMI_FAIL(HFMI_ERR_INVALID, "ctx_pci_bus_id: bad argument");
  HIP_TRY(hipDeviceGetPCIBusId(buf, len, ctx->device));
  return HFMI_OK;
}
