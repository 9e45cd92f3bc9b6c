// The owners of hippyflow_amd/csrc/hfmi_own.h over a fake own_acquire / own_release that records every call and can fail the n-th.
// Host only: no HIP header, no device.  Built with -fsanitize=address,undefined and run by tests/test_own_handles_cpu.py.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>

#include "hfmi_own.h"

static int g_acquires[OWN_NKINDS], g_releases[OWN_NKINDS];
static int g_fail_nth = 0, g_seen = 0;                 // fail the g_fail_nth-th acquisition from now (0: none)
static std::map<void*, int> g_live;                    // handle -> kind of everything handed out and not yet given back
static int g_failures = 0;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                      \
    }                                                                    \
  } while (0)

int own_acquire(own_kind kind, size_t size_or_flags, void** handle) {
  *handle = nullptr;
  if (g_fail_nth > 0 && ++g_seen == g_fail_nth) return 2;      // hipErrorOutOfMemory
  void* p = malloc(kind == OWN_DEVICE || kind == OWN_PINNED ? (size_or_flags ? size_or_flags : 1) : 1);
  g_live[p] = kind;
  ++g_acquires[kind];
  *handle = p;
  return 0;
}
void own_release(own_kind kind, void* handle) {
  auto it = g_live.find(handle);
  CHECK(it != g_live.end() && it->second == kind);      // a handle this fake handed out, of that kind, released once
  if (it == g_live.end()) return;
  g_live.erase(it);
  ++g_releases[kind];
  free(handle);
}
static void fail_nth(int n) { g_fail_nth = n, g_seen = 0; }
static int live(own_kind k) { return g_acquires[k] - g_releases[k]; }

template <class Buf>
static void check_buffer(own_kind K) {
  const int r0 = g_releases[K];
  {
    Buf a;
    CHECK(!a && a.get() == nullptr && a.count() == 0);
    CHECK(a.alloc(10) == 0 && a && a.count() == 10 && a.bytes() == 10 * sizeof(*a.get()));
    a.get()[9] = 0;                                     // the whole extent is there (the sanitizer watches)
    Buf b(std::move(a));                                // a moved-from handle is empty
    CHECK(!a && a.count() == 0 && b && b.count() == 10 && live(K) == 1);
    Buf c;
    CHECK(c.alloc(3) == 0 && live(K) == 2);
    void* old = c.get();
    c = std::move(b);                                   // move-assignment onto a live handle releases the old resource once
    CHECK(!b && b.count() == 0 && c.count() == 10 && live(K) == 1 && g_releases[K] == r0 + 1 && !g_live.count(old));
    c.reset();                                          // reset releases once ...
    CHECK(!c && c.count() == 0 && live(K) == 0 && g_releases[K] == r0 + 2);
    c.reset();                                          // ... and an empty handle releases nothing
    CHECK(g_releases[K] == r0 + 2);
    CHECK(c.alloc(4) == 0 && live(K) == 1);             // left to the destructor
    fail_nth(1);
    Buf d;
    CHECK(d.alloc(5) != 0 && !d && d.count() == 0);     // a failed acquisition leaves the handle empty
    fail_nth(0);
  }
  CHECK(live(K) == 0 && g_releases[K] == r0 + 3);       // destruction released c once, the empty ones nothing
}

static void check_grow(own_kind K) {
  int drains = 0;
  auto drain = [&] { return ++drains, 0; };
  dev_buf<double> b;
  const int a0 = g_acquires[K], r0 = g_releases[K];
  CHECK(grow(b, 8, drain) == 0 && b.count() == 8 && drains == 1 && g_acquires[K] == a0 + 1);            // grown from empty
  double* p = b.get();
  CHECK(grow(b, 8, drain) == 0 && grow(b, 5, drain) == 0 && b.get() == p && drains == 1 && g_acquires[K] == a0 + 1);   // large enough
  CHECK(grow(b, 9, drain, 4) == 0 && b.count() == 13 && drains == 2 && g_acquires[K] == a0 + 2 && g_releases[K] == r0 + 1);   // grown
  b.get()[12] = 0;
  fail_nth(1);
  CHECK(grow(b, 14, drain) == 2 && !b && b.count() == 0 && drains == 3 && g_releases[K] == r0 + 2 && live(K) == 0);   // failed: empty
  fail_nth(0);
  CHECK(grow(b, 14, drain) == 0 && b.count() == 14);                                                       // and usable again
  CHECK(grow(b, 20, [] { return 7; }) == 7 && !b && b.count() == 0 && g_acquires[K] == a0 + 3 && live(K) == 0);   // a failed drain: empty, nothing acquired
}

static void check_event_and_stream() {
  {
    hip_event e, f;
    CHECK(e.create(2) == 0 && e && live(OWN_EVENT) == 1);
    f = std::move(e);
    CHECK(!e && f && live(OWN_EVENT) == 1);
    CHECK(f.create() == 0 && live(OWN_EVENT) == 1);     // creating again releases what the handle held
  }
  CHECK(live(OWN_EVENT) == 0);
  ihipStream_t* const callers = (ihipStream_t*)&g_failures;      // any address: a caller's stream is never dereferenced or released
  const int r0 = g_releases[OWN_STREAM];
  {
    hip_stream s;
    CHECK(s.create(1) == 0 && s.owned() && live(OWN_STREAM) == 1);
    s.borrow(callers);                                  // referring to the caller's stream lets go of the own one
    CHECK(!s.owned() && s.get() == callers && live(OWN_STREAM) == 0 && g_releases[OWN_STREAM] == r0 + 1);
    hip_stream t(std::move(s));                         // the non-owning state moves with the handle
    CHECK(!s && !t.owned() && t.get() == callers);
    hip_stream own;
    CHECK(own.create(1) == 0);
    hip_stream saved = std::move(own);                  // the swap of the ingest upload: borrow for one launch, then put back
    own.borrow(callers);
    own = std::move(saved);
    CHECK(own.owned() && live(OWN_STREAM) == 1 && g_releases[OWN_STREAM] == r0 + 1);
    t.reset();
    CHECK(!t && g_releases[OWN_STREAM] == r0 + 1);
    hip_stream u;
    u.borrow(callers);                                  // destroyed while non-owning
  }
  CHECK(live(OWN_STREAM) == 0 && g_releases[OWN_STREAM] == r0 + 2);      // only the two own streams were ever released
}

int main() {
  check_buffer<dev_buf<double>>(OWN_DEVICE);
  check_buffer<pinned_buf<char>>(OWN_PINNED);
  check_grow(OWN_DEVICE);
  check_event_and_stream();
  for (int k = 0; k < OWN_NKINDS; ++k) CHECK(g_acquires[k] > 0 && g_acquires[k] == g_releases[k]);      // every acquire matched at exit
  CHECK(g_live.empty());
  if (g_failures) {
    fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  printf("own handles OK: acquired/released %d %d %d %d\n", g_acquires[0], g_acquires[1], g_acquires[2], g_acquires[3]);
  return 0;
}
