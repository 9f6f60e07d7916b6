// devbuf_check.cpp - csrc/devbuf.hpp on the CPU: the allocator seam is malloc / free with a "fail the k-th allocation" switch, the program
// is built with -fsanitize=address,undefined and run as a child process (tests/test_devbuf_cpu.py).  Exit status 0 and "devbuf ok" on
// success; the first failed check prints its line and exits 1 (a leak or a double free is the sanitizer's to report).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "devbuf.hpp"

static int g_allocs = 0, g_frees = 0, g_fail_at = 0;  // g_fail_at = k > 0: the k-th allocation from now on fails
static unsigned g_last_flags = 0;
static std::set<void *> g_live;
enum { ERR_ALLOC = 7 };

static int seam_alloc(void **p, size_t bytes) {
  if (g_fail_at > 0 && --g_fail_at == 0) {
    *p = nullptr;
    return ERR_ALLOC;
  }
  *p = malloc(bytes);
  ++g_allocs;
  g_live.insert(*p);
  return 0;
}
static int seam_free(void *p) {
  if (!g_live.erase(p)) {
    printf("free of a block that is not live\n");
    exit(1);
  }
  ++g_frees;
  free(p);
  return 0;
}
namespace dust {
int devbuf_dev_alloc(void **p, size_t bytes) { return seam_alloc(p, bytes); }
int devbuf_dev_free(void *p) { return seam_free(p); }
int devbuf_pin_alloc(void **p, size_t bytes, unsigned flags) {
  g_last_flags = flags;
  return seam_alloc(p, bytes);
}
int devbuf_pin_free(void *p) { return seam_free(p); }
}  // namespace dust
using namespace dust;

#define CHECK(x)                                      \
  do {                                                \
    if (!(x)) {                                       \
      printf("line %d: %s\n", __LINE__, #x);          \
      exit(1);                                        \
    }                                                 \
  } while (0)

static long long live_blocks() { return g_live_allocs.load(); }
static long long live_bytes() { return g_live_bytes.load(); }

// a handle in miniature: several owners of several types, allocated in order until one fails
struct Handle {
  DevBuf<float> a, b;
  DevBuf<long long> idx;
  PinBuf<unsigned char> host;
  DevBuf<unsigned short> z;
  int fill() {
    if (int s = a.alloc(10)) return s;
    if (int s = b.ensure(3)) return s;
    if (int s = idx.alloc(5)) return s;
    if (int s = host.alloc(64, 3u)) return s;
    return z.ensure(9);
  }
};

int main() {
  {  // alloc(0) gives one element; sizes are elements of T
    DevBuf<double> d;
    CHECK(d.get() == nullptr && d.cap() == 0);
    CHECK(d.alloc(0) == 0);
    CHECK(d.get() != nullptr && d.cap() == 1);
    CHECK(live_blocks() == 1 && live_bytes() == (long long)sizeof(double));
    d[0] = 1.0;  // (the element is there: the sanitizer watches)
  }
  CHECK(live_blocks() == 0 && live_bytes() == 0);
  {  // ensure below, at and above the capacity
    DevBuf<int> d;
    CHECK(d.ensure(0) == 0 && d.get() == nullptr);  // (nothing asked for: nothing allocated, as ever)
    CHECK(d.ensure(8) == 0 && d.cap() == 8);
    int *p = d.get();
    const int a0 = g_allocs, f0 = g_frees;
    CHECK(d.ensure(5) == 0 && d.get() == p && d.cap() == 8);
    CHECK(d.ensure(8) == 0 && d.get() == p && d.cap() == 8);
    CHECK(g_allocs == a0 && g_frees == f0);
    CHECK(d.ensure(9) == 0 && d.cap() == 9);
    CHECK(g_allocs == a0 + 1 && g_frees == f0 + 1);  // the old block freed exactly once (before the new one came: it was not live)
    CHECK(live_blocks() == 1 && live_bytes() == 9 * (long long)sizeof(int));
    d[8] = 1;
    // a failed growth leaves the owner empty, and a later ensure succeeds
    g_fail_at = 1;
    CHECK(d.ensure(100) == ERR_ALLOC);
    CHECK(d.get() == nullptr && d.cap() == 0);
    CHECK(live_blocks() == 0 && live_bytes() == 0);
    CHECK(d.ensure(100) == 0 && d.cap() == 100);
    d[99] = 2;
  }
  CHECK(live_blocks() == 0 && g_live.empty());
  {  // swap between two buffers of different capacity
    DevBuf<float> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(16) == 0);
    float *pa = a.get(), *pb = b.get();
    a.swap(b);
    CHECK(a.get() == pb && a.cap() == 16 && b.get() == pa && b.cap() == 4);
    a[15] = 1.f;
    b[3] = 1.f;
    DevBuf<float> e;
    a.swap(e);  // ... and with an empty one
    CHECK(a.get() == nullptr && a.cap() == 0 && e.get() == pb && e.cap() == 16);
  }
  CHECK(live_blocks() == 0 && g_live.empty());
  {  // move construction, and move assignment onto a live buffer
    DevBuf<float> a;
    CHECK(a.alloc(4) == 0);
    float *pa = a.get();
    DevBuf<float> b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 4);
    DevBuf<float> c;
    CHECK(c.alloc(7) == 0);
    const int f0 = g_frees;
    c = std::move(b);
    CHECK(g_frees == f0 + 1);  // c's own block went
    CHECK(c.get() == pa && c.cap() == 4 && b.get() == nullptr && b.cap() == 0);
    CHECK(live_blocks() == 1);
  }
  CHECK(live_blocks() == 0 && g_live.empty());
  {  // reset twice; pinned memory keeps its flags
    PinBuf<unsigned int> h;
    CHECK(h.alloc(8, 5u) == 0 && g_last_flags == 5u && h.cap() == 8);
    h[7] = 1u;
    CHECK(h.reset() == 0 && h.get() == nullptr && h.cap() == 0);
    CHECK(h.reset() == 0);
    CHECK(live_blocks() == 0);
  }
  // a struct of several owners, destroyed after the k-th allocation failed, for every k (k = 6: none fails)
  for (int k = 1; k <= 6; ++k) {
    {
      Handle h;
      g_fail_at = k;
      const int s = h.fill();
      CHECK(k <= 5 ? s == ERR_ALLOC : s == 0);
      CHECK(live_blocks() == (k <= 5 ? k - 1 : 5));
      g_fail_at = 0;
    }
    CHECK(live_blocks() == 0 && live_bytes() == 0 && g_live.empty());
  }
  CHECK(g_allocs == g_frees);
  printf("devbuf ok\n");
  return 0;
}
