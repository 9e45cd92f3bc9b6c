// Ownership of device resources (hfmi_own.hip is the unit behind it).  own_acquire / own_release are the only callers of hipMalloc,
// hipFree, hipHostMalloc, hipHostFree, hipEventCreate*, hipEventDestroy, hipStreamCreate* and hipStreamDestroy in the library
// (hfmi_comm.hip excepted: its buffers are a protocol between ranks); they count what they hand out.  The owners on top of them are
// move-only, release in their destructor and include nothing from HIP: a host-only program instantiates them over its own
// own_acquire / own_release (tests/native/own_handles_test.cpp).
#pragma once
#include <stddef.h>

typedef struct ihipStream_t* hipStream_t;   // as <hip/hip_runtime_api.h> declares them
typedef struct ihipEvent_t* hipEvent_t;

enum own_kind { OWN_DEVICE = 0, OWN_PINNED, OWN_EVENT, OWN_STREAM, OWN_NKINDS };
// size_or_flags: bytes of a buffer, the flags of hipEventCreateWithFlags / hipStreamCreateWithFlags.  Returns the hipError_t as an
// int (0 = hipSuccess); *handle is null after a failure.
int own_acquire(own_kind kind, size_t size_or_flags, void** handle);
void own_release(own_kind kind, void* handle);

// one handle of kind K; `count_` rides along for the buffers so that a pointer and its size move, grow and empty together
template <own_kind K>
class own_raw {
 public:
  own_raw() = default;
  own_raw(own_raw&& o) noexcept : h_(o.h_), count_(o.count_), owned_(o.owned_) { o.forget(); }
  own_raw& operator=(own_raw&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_, count_ = o.count_, owned_ = o.owned_;
      o.forget();
    }
    return *this;
  }
  own_raw(const own_raw&) = delete;
  own_raw& operator=(const own_raw&) = delete;
  ~own_raw() { reset(); }
  void reset() {
    if (owned_ && h_) own_release(K, h_);
    forget();
  }
  explicit operator bool() const { return h_ != nullptr; }

 protected:
  int acquire(size_t size_or_flags, size_t count) {
    reset();
    const int e = own_acquire(K, size_or_flags, &h_);
    if (e != 0) {
      h_ = nullptr;
      return e;
    }
    owned_ = true;
    count_ = count;
    return 0;
  }
  void forget() { h_ = nullptr, count_ = 0, owned_ = false; }
  void* h_ = nullptr;
  size_t count_ = 0;
  bool owned_ = false;
};

// `count` elements of T in device (dev_buf) or pinned host (pinned_buf) memory; reads as a T*
template <class T, own_kind K>
class own_buf : public own_raw<K> {
 public:
  int alloc(size_t count) { return this->acquire(count * sizeof(T), count); }
  T* get() const { return static_cast<T*>(this->h_); }
  operator T*() const { return get(); }
  T* operator->() const { return get(); }
  size_t count() const { return this->count_; }
  size_t bytes() const { return this->count_ * sizeof(T); }
};
template <class T>
using dev_buf = own_buf<T, OWN_DEVICE>;
template <class T>
using pinned_buf = own_buf<T, OWN_PINNED>;

// reads as the HIP handle H
template <own_kind K, class H>
class own_res : public own_raw<K> {
 public:
  int create(unsigned flags = 0) { return this->acquire(flags, 0); }
  H get() const { return static_cast<H>(this->h_); }
  operator H() const { return get(); }
};
using hip_event = own_res<OWN_EVENT, hipEvent_t>;
// a stream of the library's own, or a caller's that it only refers to (hfmi_ctx_set_stream) and never releases
class hip_stream : public own_res<OWN_STREAM, hipStream_t> {
 public:
  void borrow(hipStream_t s) {
    reset();
    h_ = s;
  }
  bool owned() const { return owned_; }
};

// Make `buf` hold at least `count` elements.  Large enough already: a compare and a return.  Otherwise drain() (an int, 0 = go on:
// wait for whatever may still use the old memory), release, acquire count + slack elements.  A failure of either is returned and
// leaves the buffer empty with count 0.
template <class Buf, class Drain>
inline int grow(Buf& buf, size_t count, Drain&& drain, size_t slack = 0) {
  if (count <= buf.count()) return 0;
  int e = drain();
  buf.reset();
  if (e == 0) e = buf.alloc(count + slack);
  return e;
}
