/* gq_host_res.h - what the host API (gq_api.hip) owns: move-only holders of device buffers, pinned host buffers, streams and events, and
 * the staged upload of a small argument block.  Host only. */
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>

#define GQ_ARG_SLOTS 8
namespace gq {

/* where a Buf takes its memory from: these two in the product, a counting fake in tests/test_host_resources.py */
struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
  static hipError_t zero(void* p, size_t bytes) { return hipMemset(p, 0, bytes); }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
  static hipError_t zero(void* p, size_t bytes) { std::memset(p, 0, bytes); return hipSuccess; }
};

template <class T, class Mem = DeviceMem>
class Buf {
  T* p_ = nullptr; size_t n_ = 0;
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
  ~Buf() { reset(); }
  T* get() const { return p_; }
  size_t count() const { return n_; }
  void reset() { if (p_) Mem::free(p_); p_ = nullptr; n_ = 0; }
  /* at least `count` elements: keeps a block that is large enough, otherwise releases it FIRST (the two never add up in the footprint) and
   * allocates anew, zero-filled on request.  A failure leaves the holder empty. */
  hipError_t ensure(size_t count, bool zero) {
    if (count <= n_) return hipSuccess;
    reset();
    void* q = nullptr;
    hipError_t e = Mem::alloc(&q, count * sizeof(T));
    if (e != hipSuccess) return e;
    if (zero && (e = Mem::zero(q, count * sizeof(T))) != hipSuccess) { Mem::free(q); return e; }
    p_ = static_cast<T*>(q);
    n_ = count;
    return hipSuccess;
  }
};
/* two buffers that are only ever valid together: both hold their counts afterwards, or both are empty */
template <class A, class B>
hipError_t ensure_both(A& a, size_t na, B& b, size_t nb, bool zero) {
  hipError_t e = a.ensure(na, zero);
  if (e == hipSuccess) e = b.ensure(nb, zero);
  if (e != hipSuccess) { a.reset(); b.reset(); }
  return e;
}

/* a stream or an event: created into put(), destroyed with the holder */
template <class H, hipError_t (*Destroy)(H)>
class Handle {
  H h_ = nullptr;
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Handle& operator=(Handle&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
  ~Handle() { reset(); }
  H get() const { return h_; }
  H* put() { reset(); return &h_; }
  void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

/* A small block the kernels read from device memory, and the stream-ordered way to change it: launches already queued on the stream keep
 * seeing the old block.  `shadow` is what the device holds once the copies issued so far have run.  Callers build `want` as a COPY of the
 * shadow and overwrite its fields: the padding bytes must match for the memcmp.  Known limit: when the ring has wrapped, only the stream of
 * the current call is drained - a slot last used on another stream is not waited for. */
template <class T>
struct Staged {
  Buf<T> dev;
  Buf<T, PinnedMem> ring;   /* GQ_ARG_SLOTS entries */
  T shadow;
  int next = 0; bool valid = false;
  Staged() { std::memset(&shadow, 0, sizeof shadow); }
  hipError_t create() { const hipError_t e = dev.ensure(1, false); return e != hipSuccess ? e : ring.ensure(GQ_ARG_SLOTS, false); }
  hipError_t push(const T& want, hipStream_t s, bool force) { /* force: skip the comparison (the caller knows, or wants the block sent anyway) */
    if (valid && !force && std::memcmp(&want, &shadow, sizeof(T)) == 0) return hipSuccess;
    if (next == GQ_ARG_SLOTS) { /* every slot may still be in flight: drain before reusing the ring */
      if (const hipError_t e = hipStreamSynchronize(s); e != hipSuccess) return e;
      next = 0;
    }
    T* slot = ring.get() + next++;
    std::memcpy(slot, &want, sizeof(T));
    if (const hipError_t e = hipMemcpyAsync(dev.get(), slot, sizeof(T), hipMemcpyHostToDevice, s); e != hipSuccess) return e;
    shadow = want;
    valid = true;
    return hipSuccess;
  }
};

}  // namespace gq
