// Stand-alone check of Once<T> (graphminer_amd/csrc/gm_once.h) on the host, with DevOwn<T> values over the counting allocator of
// devown_host_check.cc.  Built and run twice by tests/test_once_host.py:
//   g++ -std=c++17 -pthread -fsanitize=address,undefined -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ once_host_check.cc
//   g++ -std=c++17 -pthread -fsanitize=thread            -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ once_host_check.cc
// Exit status 0 and "once ok" when every check holds (a leak, a use after free or a data race ends the run through the sanitizer).
#include "../graphminer_amd/csrc/gm_devown.h"
#include "../graphminer_amd/csrc/gm_once.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static std::atomic<long> g_allocs{0}, g_frees{0};
hipError_t dev_malloc_bytes(void **p, size_t bytes) {
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return hipErrorOutOfMemory;
  ++g_allocs;
  return hipSuccess;
}
void dev_free(void *p) {
  if (!p) return;
  ++g_frees;
  free(p);
}
static long live() { return g_allocs - g_frees; }

static std::atomic<int> g_bad{0};
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

constexpr int kErr = 3;  // (an error code of the library: any value other than the two results of a builder)

struct Lists {  // a group as gm_graph holds them: several owners and the scalars that describe them
  DevOwn<int> rp, edge;
  DevOwn<double> desc;
  int n = 0;
  int skip_from = 0x7fffffff;
  long long info[4] = {0, 0, 0, 0};
};

static int build_lists(Lists &l, int n, int fail_after) {  // fail_after: allocations that succeed before the error (< 0: none fails)
  if (fail_after == 0) return kErr;
  if (l.rp.alloc(sizeof(int) * n) != hipSuccess) return kErr;
  for (int i = 0; i < n; ++i) l.rp.get()[i] = i;
  if (fail_after == 1) return kErr;
  if (l.edge.alloc(sizeof(int) * n) != hipSuccess) return kErr;
  if (fail_after == 2) return kErr;
  if (l.desc.alloc(sizeof(double) * n) != hipSuccess) return kErr;
  for (int i = 0; i < n; ++i) l.desc.get()[i] = 0.5 * i;
  l.n = n;
  l.skip_from = 7;
  for (int i = 0; i < 4; ++i) l.info[i] = 100 + i;
  return kOnceBuilt;
}
static bool complete(const Lists &l, int n) {
  if (l.n != n || l.skip_from != 7 || !l.rp || !l.edge || !l.desc) return false;
  for (int i = 0; i < 4; ++i)
    if (l.info[i] != 100 + i) return false;
  return l.rp.get()[n - 1] == n - 1 && l.desc.get()[n - 1] == 0.5 * (n - 1);
}

int main() {
  {  // before anything ran: unknown, and a reader gets the defaults of an empty value, not the members
    Once<Lists> o;
    CHECK(!o.known() && !o.built());
    CHECK(o->rp.get() == nullptr && o->n == 0 && o->skip_from == 0x7fffffff);
  }
  {  // eight threads race on the first ensure: the builder runs exactly once, every thread reads the complete value
    Once<Lists> o;
    std::mutex mu;
    std::atomic<int> runs{0}, go{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
      th.emplace_back([&] {
        ++go;
        while (go.load() < 8) std::this_thread::yield();
        const int rc = o.ensure(mu, [&](Lists &l) {
          ++runs;
          std::this_thread::yield();
          return build_lists(l, 1000, -1);
        });
        CHECK(rc == 0);
        CHECK(o.built() && complete(*o, 1000));
        CHECK(o->desc.get()[999] == 499.5);
      });
    for (auto &t : th) t.join();
    CHECK(runs.load() == 1);
    CHECK(live() == 3);
    int again = 0;  // and not again later
    CHECK(o.ensure(mu, [&](Lists &) { ++again; return kOnceBuilt; }) == 0 && again == 0);
  }
  CHECK(live() == 0);  // (the value's owners free with the Once)
  {  // a builder that fails: nothing is published, what it had allocated is freed, the next call builds
    Once<Lists> o;
    std::mutex mu;
    for (int fail_after = 0; fail_after <= 2; ++fail_after) {
      const long a0 = g_allocs, f0 = g_frees;
      CHECK(o.ensure(mu, [&](Lists &l) { return build_lists(l, 64, fail_after); }) == kErr);
      CHECK(g_allocs - a0 == fail_after && g_frees - f0 == fail_after);
      CHECK(!o.known() && !o.built() && o->rp.get() == nullptr && o->n == 0);
    }
    CHECK(live() == 0);
    int runs = 0;
    CHECK(o.ensure(mu, [&](Lists &l) { ++runs; return build_lists(l, 64, -1); }) == 0);
    CHECK(runs == 1 && o.built() && complete(*o, 64) && live() == 3);
  }
  CHECK(live() == 0);
  {  // not applicable is remembered with the value the builder left, and the builder is not run again
    Once<Lists> o;
    std::mutex mu;
    int runs = 0;
    auto na = [&](Lists &l) { ++runs; l.n = -5; return kOnceNotApplicable; };
    CHECK(o.ensure(mu, na) == 0);
    CHECK(o.known() && !o.built() && o->n == -5 && o->rp.get() == nullptr);
    CHECK(o.ensure(mu, na) == 0 && o.ensure(mu, [&](Lists &l) { ++runs; return build_lists(l, 8, -1); }) == 0);
    CHECK(runs == 1 && !o.built() && live() == 0);
  }
  {  // reset (the row-order facts of gm_graph_sort_neighbors), followed by a rebuild; a value with owners gives them back on reset
    Once<bool> sorted;
    std::mutex mu;
    int runs = 0;
    CHECK(sorted.ensure(mu, [&](bool &b) { ++runs; b = false; return kOnceBuilt; }) == 0 && sorted.built() && !*sorted);
    sorted.reset();
    CHECK(!sorted.known() && !*sorted);
    CHECK(sorted.ensure(mu, [&](bool &b) { ++runs; b = true; return kOnceBuilt; }) == 0 && sorted.built() && *sorted && runs == 2);
    Once<Lists> o;
    CHECK(o.ensure(mu, [&](Lists &l) { return build_lists(l, 16, -1); }) == 0 && live() == 3);
    o.reset();
    CHECK(live() == 0 && !o.known() && o->n == 0);
    CHECK(o.ensure(mu, [&](Lists &l) { return build_lists(l, 32, -1); }) == 0 && complete(*o, 32) && live() == 3);
  }
  CHECK(live() == 0);
  {  // a value with several owners is moved in whole: the arrays the builder allocated are the arrays the reader sees, none copied or freed
    Once<Lists> o;
    std::mutex mu;
    int *rp = nullptr, *edge = nullptr;
    double *desc = nullptr;
    const long a0 = g_allocs, f0 = g_frees;
    CHECK(o.ensure(mu, [&](Lists &l) {
      const int rc = build_lists(l, 128, -1);
      rp = l.rp; edge = l.edge; desc = l.desc;
      return rc;
    }) == 0);
    CHECK(o->rp.get() == rp && o->edge.get() == edge && o->desc.get() == desc && complete(*o, 128));
    CHECK(g_allocs - a0 == 3 && g_frees == f0);
  }
  CHECK(live() == 0);
  if (g_bad) return 1;
  printf("once ok: %ld blocks allocated, %ld freed\n", g_allocs.load(), g_frees.load());
  return 0;
}
