// Stand-alone check of DevOwn<T> (graphminer_amd/csrc/gm_devown.h) on the host: the library's allocator is replaced by counting stand-ins on
// the host heap, so the address / undefined-behaviour sanitizers see every block.  Built and run by tests/test_devown_host.py:
//   g++ -std=c++17 -fsanitize=address,undefined -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ devown_host_check.cc
// Exit status 0 and "devown ok" when every check holds (a leak, a double free or a use after free ends the run through the sanitizer).
#include "../graphminer_amd/csrc/gm_devown.h"

#include <cstdio>
#include <cstdlib>
#include <list>
#include <utility>
#include <vector>

static long g_allocs = 0, g_frees = 0;
static void *g_last_freed = nullptr;
hipError_t dev_malloc_bytes(void **p, size_t bytes) {
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return hipErrorOutOfMemory;
  ++g_allocs;
  return hipSuccess;
}
void dev_free(void *p) {
  if (!p) return;
  ++g_frees;
  g_last_freed = p;
  free(p);
}
static long live() { return g_allocs - g_frees; }

static int g_bad = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

struct KeptBuf {  // what DevOwn::take needs of a DevBuf<T> allocated with keep = true
  int *p = nullptr;
  int *release() { int *q = p; p = nullptr; return q; }
};

struct Table {  // a struct of owners, as ChunkTable / CliqueRound are
  DevOwn<int> a, b;
  DevOwn<double> c;
  int tag = 0;
};

static hipError_t three_locals(bool fail_at_third) {
  DevOwn<int> x, y, z;
  if (x.alloc(64) != hipSuccess) return hipErrorOutOfMemory;
  if (y.alloc(64) != hipSuccess) return hipErrorOutOfMemory;
  if (fail_at_third) return hipErrorUnknown;  // (two filled, one empty)
  return z.alloc(64);
}

int main() {
  {  // the destructor frees once; an empty owner frees nothing
    const long f0 = g_frees;
    {
      DevOwn<int> o, empty;
      CHECK(o.get() == nullptr && !o);
      CHECK(o.alloc(128) == hipSuccess);
      CHECK(o.get() != nullptr && live() == 1);
      int *raw = o;  // the implicit conversion
      CHECK(raw == o.get() && o + 1 == raw + 1);
      raw[31] = 7;  // (the block is really there)
    }
    CHECK(g_frees == f0 + 1 && live() == 0);
  }
  {  // allocate over a held block: the old one goes back FIRST
    DevOwn<int> o;
    CHECK(o.alloc(16) == hipSuccess);
    int *first = o;
    const long f0 = g_frees, a0 = g_allocs;
    CHECK(o.alloc(32) == hipSuccess);
    CHECK(g_frees == f0 + 1 && g_allocs == a0 + 1 && g_last_freed == first && live() == 1);
  }
  CHECK(live() == 0);
  {  // move construction: the source is empty, nothing is freed
    DevOwn<int> a;
    CHECK(a.alloc(16) == hipSuccess);
    int *p = a;
    const long f0 = g_frees;
    DevOwn<int> b(std::move(a));
    CHECK(a.get() == nullptr && b.get() == p && g_frees == f0);
    // move assignment: the target's block is freed, the source is empty
    DevOwn<int> c;
    CHECK(c.alloc(16) == hipSuccess);
    int *old = c;
    c = std::move(b);
    CHECK(b.get() == nullptr && c.get() == p && g_frees == f0 + 1 && g_last_freed == old && live() == 1);
    // self-move-assign is harmless
    DevOwn<int> &alias = c;
    c = std::move(alias);
    CHECK(c.get() == p && g_frees == f0 + 1 && live() == 1);
    c.get()[0] = 1;
  }
  CHECK(live() == 0);
  {  // reset, and reset of an empty owner
    DevOwn<int> o;
    const long f0 = g_frees;
    o.reset();
    CHECK(g_frees == f0);
    CHECK(o.alloc(16) == hipSuccess);
    o.reset();
    CHECK(o.get() == nullptr && g_frees == f0 + 1);
    o.reset();
    CHECK(g_frees == f0 + 1);
  }
  CHECK(live() == 0);
  {  // take-over from a kept buffer (and over a held block)
    KeptBuf buf;
    void *q = nullptr;
    CHECK(dev_malloc_bytes(&q, 64) == hipSuccess);
    buf.p = static_cast<int *>(q);
    DevOwn<int> o;
    CHECK(o.alloc(16) == hipSuccess);
    const long f0 = g_frees;
    o.take(buf);
    CHECK(buf.p == nullptr && o.get() == q && g_frees == f0 + 1 && live() == 1);
  }
  CHECK(live() == 0);
  {  // a struct of owners moved into a list / a vector and cleared returns every block
    std::list<Table> tables;
    std::vector<Table> rounds;
    for (int i = 0; i < 5; ++i) {
      Table t;
      t.tag = i;
      CHECK(t.a.alloc(8) == hipSuccess && t.c.alloc(8) == hipSuccess);  // (b stays empty: a borrowed array's owner)
      tables.push_back(std::move(t));
      Table r;
      CHECK(r.a.alloc(8) == hipSuccess && r.b.alloc(8) == hipSuccess && r.c.alloc(8) == hipSuccess);
      rounds.push_back(std::move(r));  // (reallocations move the elements)
    }
    CHECK(live() == 5 * 2 + 5 * 3);
    CHECK(tables.back().tag == 4 && tables.back().a.get() != nullptr && tables.back().b.get() == nullptr);
    tables.clear();
    CHECK(live() == 5 * 3);
    rounds.clear();
    CHECK(live() == 0);
  }
  {  // an early return out of a function with three local owners, two of them filled, returns exactly two blocks
    const long f0 = g_frees, a0 = g_allocs;
    CHECK(three_locals(true) == hipErrorUnknown);
    CHECK(g_allocs == a0 + 2 && g_frees == f0 + 2);
    CHECK(three_locals(false) == hipSuccess);
    CHECK(g_allocs == a0 + 5 && g_frees == f0 + 5);
  }
  CHECK(live() == 0);
  if (g_bad) return 1;
  printf("devown ok: %ld blocks allocated, %ld freed\n", g_allocs, g_frees);
  return 0;
}
