// devbuf.hpp - owners of device memory and of pinned host memory (host code only; no HIP header is needed to read it).
// DevBuf<T> / PinBuf<T> hold one block and its capacity IN ELEMENTS OF T, free it when they go, move but do not copy.  Every handle type
// of the library keeps its memory in them, so a handle's destructor is its release list.
#pragma once
#include <atomic>
#include <cstddef>
#include <utility>

namespace dust {
// The allocator seam: four functions the including unit defines (dust_amd.hip: hipMalloc / hipFree / hipHostMalloc / hipHostFree through
// HIP_TRY; tests/devbuf_check.cpp: malloc / free with a "fail the k-th allocation" switch).  0 is success, anything else the error code
// the owner hands on.
int devbuf_dev_alloc(void **p, size_t bytes);
int devbuf_dev_free(void *p);
int devbuf_pin_alloc(void **p, size_t bytes, unsigned flags);
int devbuf_pin_free(void *p);
// blocks and bytes the owners hold at this moment, process-wide (dust_debug_live_allocs)
inline std::atomic<long long> g_live_allocs{0}, g_live_bytes{0};

template <class T, bool PINNED>
class OwnedBuf {
  T *p_ = nullptr;
  size_t cap_ = 0;

 public:
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  OwnedBuf(OwnedBuf &&o) noexcept { swap(o); }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    if (this != &o) {
      (void)reset();
      swap(o);
    }
    return *this;
  }
  ~OwnedBuf() { (void)reset(); }

  T *get() const { return p_; }
  operator T *() const & { return p_; }  // a non-owning view: kernel arguments, copies, offsets - never handed to hipFree or delete
  operator T *() && = delete;            // (a temporary's block goes with the temporary)
  size_t cap() const { return cap_; }  // elements of T
  void swap(OwnedBuf &o) {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
  }
  // frees the block, if any; empty afterwards whatever the free returned
  int reset() {
    if (!p_) return 0;
    T *p = p_;
    g_live_allocs.fetch_sub(1);
    g_live_bytes.fetch_sub((long long)(cap_ * sizeof(T)));
    p_ = nullptr;
    cap_ = 0;
    return PINNED ? devbuf_pin_free(p) : devbuf_dev_free(p);
  }
  // a fresh block of n elements (0: one element); a block held before is freed first.  `flags`: hipHostMalloc's, pinned memory only
  int alloc(size_t n, unsigned flags = 0) {
    if (int s = reset()) return s;
    if (n == 0) n = 1;
    void *p = nullptr;
    if (int s = PINNED ? devbuf_pin_alloc(&p, n * sizeof(T), flags) : devbuf_dev_alloc(&p, n * sizeof(T))) return s;
    p_ = static_cast<T *>(p);
    cap_ = n;
    g_live_allocs.fetch_add(1);
    g_live_bytes.fetch_add((long long)(n * sizeof(T)));
    return 0;
  }
  // room for n elements: nothing happens while the capacity suffices, otherwise free, then allocate (contents are not kept)
  int ensure(size_t n) { return cap_ >= n ? 0 : alloc(n); }
};
template <class T>
using DevBuf = OwnedBuf<T, false>;
template <class T>
using PinBuf = OwnedBuf<T, true>;
}  // namespace dust
