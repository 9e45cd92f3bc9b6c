// The choke point of hfmi_own.h: every device buffer, pinned buffer, event and stream of the library (hfmi_comm.hip excepted) is made
// and given back here, counted per kind, and the tests can make the n-th acquisition fail on the host.  Host side only.
#include <atomic>

#include "hfmi_internal.h"

static std::atomic<int64_t> g_acquired[OWN_NKINDS], g_released[OWN_NKINDS];
// hfmi_test_own_fail: acquisitions number g_fail_first .. g_fail_first + g_fail_count - 1 after arming fail; 0 = disarmed
static std::atomic<int64_t> g_fail_seen{0};
static std::atomic<int> g_fail_first{0}, g_fail_count{0};

int own_acquire(own_kind kind, size_t size_or_flags, void** handle) {
  *handle = nullptr;
  const int first = g_fail_first.load(std::memory_order_relaxed);
  if (first > 0) {
    const int64_t n = g_fail_seen.fetch_add(1, std::memory_order_relaxed) + 1;
    if (n >= first && n < (int64_t)first + g_fail_count.load(std::memory_order_relaxed)) return (int)hipErrorOutOfMemory;
  }
  hipError_t e = hipErrorInvalidValue;
  switch (kind) {
    case OWN_DEVICE: e = hipMalloc(handle, size_or_flags); break;
    case OWN_PINNED: e = hipHostMalloc(handle, size_or_flags, hipHostMallocDefault); break;
    case OWN_EVENT: e = hipEventCreateWithFlags((hipEvent_t*)handle, (unsigned)size_or_flags); break;
    case OWN_STREAM: e = hipStreamCreateWithFlags((hipStream_t*)handle, (unsigned)size_or_flags); break;
    default: break;
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();      // reported to the caller: the next launch check must not find it again
    *handle = nullptr;
  } else if (*handle) {
    g_acquired[kind].fetch_add(1, std::memory_order_relaxed);
  }
  return (int)e;
}

void own_release(own_kind kind, void* handle) {
  if (!handle) return;
  switch (kind) {
    case OWN_DEVICE: (void)hipFree(handle); break;
    case OWN_PINNED: (void)hipHostFree(handle); break;
    case OWN_EVENT: (void)hipEventDestroy((hipEvent_t)handle); break;
    case OWN_STREAM: (void)hipStreamDestroy((hipStream_t)handle); break;
    default: return;
  }
  g_released[kind].fetch_add(1, std::memory_order_relaxed);
}

extern "C" int hfmi_test_own_fail(int first, int count) {
  if (first < 0 || count < 0) HFMI_FAIL(HFMI_ERR_INVALID, "test_own_fail: negative argument");
  g_fail_first.store(0);
  g_fail_seen.store(0);
  g_fail_count.store(count);
  g_fail_first.store(count > 0 ? first : 0);
  return HFMI_OK;
}
extern "C" int hfmi_test_own_counts(hfmi_ctx* ctx, int64_t* live, int64_t* acquired, int64_t* pooled) {
  for (int k = 0; k < OWN_NKINDS; ++k) {
    const int64_t a = g_acquired[k].load(), r = g_released[k].load();
    if (live) live[k] = a - r;
    if (acquired) acquired[k] = a;
  }
  if (pooled) *pooled = ctx ? (int64_t)ctx->pool.size() : 0;
  return HFMI_OK;
}
