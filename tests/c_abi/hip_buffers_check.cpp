// Stand-alone host check of csrc/hip_buffers.h (built with -fsanitize=address,undefined by tests/test_host_abi.py).  The six HIP runtime
// functions the header calls are defined HERE, over malloc / free with a count of live blocks and a switch that fails the k-th
// allocation: nothing links the HIP library, nothing touches a device, and a leak, a double free or a use of a freed block is a
// sanitizer report or a wrong count.  Exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "hip_buffers.h"

using namespace se3tn;

static int g_live = 0;        // blocks allocated and not freed
static int g_fail_at = 0;     // k > 0: the k-th allocation from now fails
static const size_t kAlias = 64;   // the stand-in runtime maps a pinned block kAlias bytes above its host address

static hipError_t stand_in_alloc(void** p, size_t bytes) {
  if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;   // (*p is left alone, as the runtime may leave it)
  *p = std::malloc(bytes ? bytes : 1);
  ++g_live;
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stand_in_alloc(p, bytes); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stand_in_alloc(p, bytes); }
hipError_t hipFree(void* p) { std::free(p); --g_live; return hipSuccess; }
hipError_t hipHostFree(void* p) { std::free(p); --g_live; return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) { *dev = (char*)host + kAlias; return hipSuccess; }
hipError_t hipMemset(void* p, int v, size_t bytes) { std::memset(p, v, bytes); return hipSuccess; }
}

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

struct Holder {   // as se3tn_ctx / se3tn_mesh hold theirs
  DeviceBuf<float> a;
  DeviceBuf<int> b[2];
  PinnedBuf<unsigned char> h, mapped;
  RasterScratch rs;
};

static int check() {
  {   // a struct of several buffers frees them all
    Holder s;
    CHECK(!s.a && s.a.get() == nullptr && s.a.count() == 0 && !s.h && s.h.count() == 0);
    CHECK(s.a.alloc(10, true) == hipSuccess && s.b[0].alloc(3) == hipSuccess && s.b[1].alloc(4) == hipSuccess);
    CHECK(s.h.alloc(100) == hipSuccess && s.mapped.alloc(256, true, true) == hipSuccess && s.rs.alloc(5, 7, 2) == hipSuccess);
    CHECK(g_live == 9 && s.a && s.a.count() == 10 && s.rs.vpost.count() == 10 && s.rs.big.count() == 16 && s.rs.clipq.count() == 16);
    for (int i = 0; i < 10; ++i) CHECK(s.a.get()[i] == 0.f);
    for (int i = 0; i < 256; ++i) CHECK(s.mapped.get()[i] == 0);
    s.a.get()[9] = 1.f; s.rs.clipq.get()[15] = 1; s.h.get()[99] = 1;   // (the last element of each: inside the block)
    // a mapped block reports its device alias, a default one has none
    CHECK(s.mapped.dev() == s.mapped.get() + kAlias && s.h.dev() == nullptr);
    // alloc over a held block frees it
    CHECK(s.a.alloc(20) == hipSuccess && g_live == 9 && s.a.count() == 20);
    CHECK(s.h.alloc(50) == hipSuccess && g_live == 9 && s.h.count() == 50);
    // an alloc that fails leaves the object empty -- not the old block -- and the others as they were
    g_fail_at = 1;
    CHECK(s.a.alloc(30) == hipErrorOutOfMemory && !s.a && s.a.get() == nullptr && s.a.count() == 0 && g_live == 8);
    g_fail_at = 1;
    CHECK(s.mapped.alloc(64, true, true) == hipErrorOutOfMemory && !s.mapped && s.mapped.dev() == nullptr && g_live == 7);
    s.b[0].reset();
    CHECK(!s.b[0] && s.b[0].count() == 0 && g_live == 6);
    s.b[0].reset();   // (twice: nothing held, nothing freed)
    CHECK(g_live == 6);
  }
  CHECK(g_live == 0);
  // the group of four: whichever allocation fails, it can be grown again and destroyed -- no leak, no double free
  for (int k = 1; k <= 4; ++k)
    for (int held = 0; held < 2; ++held) {   // (growing from empty, and over a held scratch)
      {
        RasterScratch rs;
        if (held) CHECK(rs.alloc(3, 2, 1) == hipSuccess && g_live == 4);
        g_fail_at = k;
        CHECK(rs.alloc(8, 6, 3) == hipErrorOutOfMemory);
        g_fail_at = 0;
        const bool set[4] = {(bool)rs.vpost, (bool)rs.vsnap, (bool)rs.big, (bool)rs.clipq};
        for (int j = 1; j <= 4; ++j) CHECK(set[j - 1] == (j < k || (held && j > k)));   // new | the failed one: empty | not reached
        CHECK(g_live == set[0] + set[1] + set[2] + set[3]);
        CHECK(rs.alloc(8, 6, 3) == hipSuccess && g_live == 4 && rs.vpost.count() == 24 && rs.vsnap.count() == 24 && rs.big.count() == 21);
        rs.clipq.get()[20] = 1;
      }
      CHECK(g_live == 0);
    }
  {   // a move transfers ownership and leaves the source empty
    DeviceBuf<float> a, b;
    CHECK(a.alloc(4) == hipSuccess && b.alloc(5) == hipSuccess && g_live == 2);
    float* const pa = a.get();
    b = std::move(a);   // (frees what b held)
    CHECK(g_live == 1 && !a && a.count() == 0 && b.get() == pa && b.count() == 4);
    DeviceBuf<float> c(std::move(b));
    CHECK(g_live == 1 && !b && c.get() == pa && c.count() == 4);
    PinnedBuf<int> h, g;
    CHECK(h.alloc(2, false, true) == hipSuccess && g_live == 2);
    int* const ph = h.get();
    g = std::move(h);
    CHECK(!h && h.dev() == nullptr && g.get() == ph && (char*)g.dev() == (char*)ph + kAlias && g.count() == 2 && g_live == 2);
    RasterScratch r1, r2;
    CHECK(r1.alloc(2, 2, 1) == hipSuccess && g_live == 6);
    r2 = std::move(r1);
    CHECK(g_live == 6 && !r1.vpost && !r1.clipq && r2.big.count() == 3);
  }
  CHECK(g_live == 0);
  return 0;
}

int main() {
  if (check()) return 1;
  std::printf("hip_buffers_check: ok\n");
  return 0;
}
