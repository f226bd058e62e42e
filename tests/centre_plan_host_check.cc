// Stand-alone check of the centre plans of the map solvers (graphminer_amd/csrc/gm_centre_plan.h) on the host, with tiny parameters: ranges of
// 64 ids or fewer, 2 to 16 threads per workgroup, a heavy-centre limit of 8.  Built and run by tests/test_centre_plan_host.py:
//   g++ -std=c++17 -fsanitize=address,undefined -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ centre_plan_host_check.cc
// Exit status 0 and "centre plan ok" when every check holds.  The literal cases were worked out by hand from the loops run_rect_acc /
// run_house_acc / run_wrect held before the plans moved into the header.
#include "../graphminer_amd/csrc/gm_centre_plan.h"

#include <cstdio>
#include <map>
#include <random>
#include <set>

using namespace gm;
typedef unsigned long long ull;
typedef std::vector<ull> W;
typedef std::vector<int> I;

static int g_bad = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

static CentreTasks rect_tasks(size_t nv, const W &work, const W &wcut, const I &idx0, const int *rb, int n, ull lds_min, int per_wg, ull heavy) {
  return plan_rect_tasks(nv, work.data(), wcut.data(), idx0.data(), rb, n, lds_min, per_wg, heavy);
}
static CentreTasks house_tasks(size_t nv, const W &work, const W &wcut, const I &deg, int n, ull lds_min, bool given, ull per_walk, int per_wg, ull heavy) {
  return plan_house_tasks(nv, work.data(), wcut.data(), deg.data(), n, lds_min, given, per_walk, per_wg, heavy);
}

struct T2 { int x, y; };
struct T4 { int x, y, z, w; };
static bool same(const std::vector<int2> &got, const std::vector<T2> &want) {
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i].x != want[i].x || got[i].y != want[i].y) return false;
  return true;
}
static bool same(const std::vector<int4> &got, const std::vector<T4> &want) {
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i].x != want[i].x || got[i].y != want[i].y || got[i].z != want[i].z || got[i].w != want[i].w) return false;
  return true;
}
#define CHECK_PLAN(t, lds, acc, ncut) \
  do {                                \
    CHECK(same((t).lds_tasks, lds));  \
    CHECK(same((t).acc_tasks, acc));  \
    CHECK((t).n_cut == (ncut));       \
  } while (0)

// ---- literal cases -------------------------------------------------------------------------------------------------------------------
static void rect_literals() {
  {  // two ranges [4, 8) [8, 12), 2 threads per workgroup, LDS from 4 2-paths on
    //             v:  0  1  2  3  4  5  6  7  8   9  10 11
    const W work = {0, 5, 3, 2, 9, 6, 6, 0, 0, 20, 7, 4};
    const W wcut = {0, 5, 3, 2, 9, 0, 2, 0, 0, 10, 2, 1};
    const I idx0 = {0, 1, 1, 1, 2, 3, 1, 0, 0, 4, 3, 2};
    const int rb[] = {4, 8, 12};
    const CentreTasks t = rect_tasks(12, work, wcut, idx0, rb, 2, 4, 2, 8);
    // LDS: 9 (20), 10 (7), 5 and 6 (6 each: by id), 11 (4).  1 has the work but lies below the cut, 4 AT the cut: no end of theirs is in a range.
    // 9, 10, 5 have more rows than threads: 9 and 10 start in range 1 (8 and 9 are the highest ends), 5 in range 0, each its top range first.
    const std::vector<T2> lds = {{9, 1}, {10, 1}, {5, 0}, {9, 0}, {10, 0}, {6, -1}, {11, -1}};
    // front: 5 has no end below the cut and is left out; by wcut 9 (10: heavy), 10 and 6 (2 each: in the order by work), 11 (1).
    // the rest by work: 4 (9: heavy), 1, 2, 3
    const std::vector<T4> acc = {{9, -2, -2, -2}, {10, 6, 11, -1}, {4, -2, -2, -2}, {1, 2, 3, -1}};
    CHECK_PLAN(t, lds, acc, 2);
  }
  {  // one range over the whole graph: nothing is left of an LDS centre, the front is empty; vertex 0 is not above the cut
    const W work = {3, 2, 2, 8, 0, 2}, wcut = {0, 0, 0, 0, 0, 0};
    const I idx0 = {0, 1, 2, 3, 0, 3};
    const int rb[] = {0, 6};
    const CentreTasks t = rect_tasks(6, work, wcut, idx0, rb, 1, 1, 2, 8);
    const std::vector<T2> lds = {{3, 0}, {5, 0}, {1, -1}, {2, -1}};
    const std::vector<T4> acc = {{0, -1, -1, -1}};
    CHECK_PLAN(t, lds, acc, 0);
  }
  {  // no LDS centre: the threshold is above every centre; five light ones make two groups
    const W work = {1, 7, 7, 2, 0, 3, 7}, wcut = {1, 7, 7, 2, 0, 1, 1};
    const I idx0 = {0, 1, 2, 3, 0, 5, 6};
    const int rb[] = {2, 7};
    const CentreTasks t = rect_tasks(7, work, wcut, idx0, rb, 1, 100, 2, 8);
    const std::vector<T4> acc = {{1, 2, 6, 5}, {3, 0, -1, -1}};
    CHECK_PLAN(t, std::vector<T2>{}, acc, 0);
  }
  {  // the form with every end in the global maps asks the planner for no LDS centre at all: every centre with work, heaviest first
    const W work = {1, 9, 7, 2, 0, 3, 7};
    const CentreTasks t = plan_centre_tasks(7, work.data(), nullptr, 0, 0, 8, [](int) { return false; }, [](int) { return 0; }, [](int) { return 0ull; }, false);
    const std::vector<T4> acc = {{1, -2, -2, -2}, {2, 6, 5, 3}, {0, -1, -1, -1}};
    CHECK_PLAN(t, std::vector<T2>{}, acc, 0);
  }
  {  // an empty graph: no range (rb[0] = nv = 0), no task
    const int rb[] = {0};
    const CentreTasks t = rect_tasks(0, W(1, 0), W(1, 0), I(1, 0), rb, 0, 4096, 1024, 1ull << 15);
    CHECK_PLAN(t, std::vector<T2>{}, std::vector<T4>{}, 0);
  }
}

static void house_literals() {
  {  // two ranges, 4 threads per workgroup, threshold 4, 10 2-paths per walk: a centre of at most 4 neighbours needs 10 (one walk of its 2 ranges)
    //             v:  0   1  2  3  4   5  6  7
    const W work = {10, 9, 5, 0, 12, 4, 3, 12};
    const W wcut = {0, 5, 1, 0, 3, 0, 3, 1};
    const I deg = {2, 3, 6, 0, 5, 5, 9, 1};
    const CentreTasks t = house_tasks(8, work, wcut, deg, 2, 4, false, 10, 4, 8);
    // LDS by work: 4 and 7 (12 each: by id), 0 (10), 2 (5), 5 (4).  1 (9 < 10, degree 3) and 6 (3 < 4) stay in the global maps.
    // 4, 2, 5 have more neighbours than threads: every range, from the top down, all of them per range.
    const std::vector<T2> lds = {{4, 1}, {2, 1}, {5, 1}, {4, 0}, {2, 0}, {5, 0}, {7, -1}, {0, -1}};
    // front: all five, by wcut + degree: 4 (8: heavy), 2 (7), 5 (0 + 5), then 7 and 0 (2 each: in the order by work, 7 first)
    const std::vector<T4> acc = {{4, -2, -2, -2}, {2, 5, 7, 0}, {1, -2, -2, -2}, {6, -1, -1, -1}};
    CHECK_PLAN(t, lds, acc, 2);
  }
  {  // a given threshold is taken as given (2 instead of 10 per walk); six front centres make two groups
    const W work = {2, 2, 2, 2, 2, 1, 2}, wcut = {0, 0, 0, 0, 0, 0, 0};
    const I deg = {1, 1, 1, 1, 1, 1, 5};
    const CentreTasks t = house_tasks(7, work, wcut, deg, 1, 2, true, 10, 4, 100);
    const std::vector<T2> lds = {{6, 0}, {0, -1}, {1, -1}, {2, -1}, {3, -1}, {4, -1}};
    const std::vector<T4> acc = {{6, 0, 1, 2}, {3, 4, -1, -1}, {5, -1, -1, -1}};
    CHECK_PLAN(t, lds, acc, 2);
    const CentreTasks u = house_tasks(7, work, wcut, deg, 1, 2, false, 10, 4, 100);  // not given: only 6 (degree above the threads) passes
    const std::vector<T2> lds_u = {{6, 0}};
    const std::vector<T4> acc_u = {{6, -1, -1, -1}, {0, 1, 2, 3}, {4, 5, -1, -1}};
    CHECK_PLAN(u, lds_u, acc_u, 1);
  }
  {  // no range: every centre in the global maps
    const W work = {3, 0, 9, 3, 1}, wcut = {3, 0, 9, 3, 1};
    const I deg = {1, 0, 7, 2, 1};
    const CentreTasks t = house_tasks(5, work, wcut, deg, 0, 1, true, 1, 4, 8);
    const std::vector<T4> acc = {{2, -2, -2, -2}, {0, 3, 4, -1}};
    CHECK_PLAN(t, std::vector<T2>{}, acc, 0);
  }
  {  // an empty graph
    const CentreTasks t = house_tasks(0, W(1, 0), W(1, 0), I(1, 0), 0, 4096, false, 200, 1024, 1ull << 15);
    CHECK_PLAN(t, std::vector<T2>{}, std::vector<T4>{}, 0);
  }
}

// ---- properties on random inputs -------------------------------------------------------------------------------------------------------
struct Policy {  // what the lists must hold, worked out here independently of the planner
  std::set<int> lds, front, rest;
  std::vector<ull> front_key;
  std::vector<int> top;  // per LDS centre: its highest range
};
static void check_properties(const CentreTasks &t, size_t nv, const W &work, const I &rows, int per_wg, ull heavy, const Policy &pol) {
  CHECK(t.n_cut <= t.acc_tasks.size());
  std::map<int, int> seen;
  for (size_t i = 0; i < t.acc_tasks.size(); ++i) {
    const bool in_front = i < t.n_cut;
    const int4 a = t.acc_tasks[i];
    const int c[4] = {a.x, a.y, a.z, a.w};
    auto key = [&](int v) { return in_front ? pol.front_key[(size_t)v] : work[(size_t)v]; };
    CHECK(a.x >= 0 && (size_t)a.x < nv);
    if (a.x < 0 || (size_t)a.x >= nv) continue;
    if (a.y == -2) {
      CHECK(a.z == -2 && a.w == -2 && key(a.x) >= heavy);
      ++seen[a.x];
    } else {
      bool ended = false;
      for (int j = 0; j < 4; ++j) {
        if (c[j] == -1) { ended = true; continue; }
        CHECK(!ended && c[j] >= 0 && (size_t)c[j] < nv);  // (the empty slots are the last ones)
        if (c[j] < 0 || (size_t)c[j] >= nv) continue;
        CHECK(key(c[j]) < heavy);
        ++seen[c[j]];
      }
    }
  }
  for (size_t v = 0; v < nv; ++v) {
    const bool want = pol.front.count((int)v) || pol.rest.count((int)v);
    CHECK((seen.count((int)v) ? seen[(int)v] : 0) == (want ? 1 : 0));
    if (work[v] == 0) CHECK(!seen.count((int)v));
  }
  // the front holds exactly the front set, the keys fall (or stay) inside the front and inside the rest
  std::set<int> got_front, got_rest;
  ull last = ~0ull;
  for (size_t i = 0; i < t.acc_tasks.size(); ++i) {
    if (i == t.n_cut) last = ~0ull;
    const int4 a = t.acc_tasks[i];
    const int c[4] = {a.x, a.y, a.z, a.w};
    for (int j = 0; j < 4; ++j) {
      if (c[j] < 0 || (size_t)c[j] >= nv) continue;
      (i < t.n_cut ? got_front : got_rest).insert(c[j]);
      const ull k = i < t.n_cut ? pol.front_key[(size_t)c[j]] : work[(size_t)c[j]];
      CHECK(k <= last);
      last = k;
    }
  }
  CHECK(got_front == pol.front);
  CHECK(got_rest == pol.rest);
  // LDS tasks: one {v, -1} or exactly the ranges 0 .. top, every centre's own top range first, the {v, -1} tasks last
  std::map<int, std::vector<int>> ranges;
  int last_j = 0;
  bool whole = false;
  for (const int2 &l : t.lds_tasks) {
    CHECK(pol.lds.count(l.x) == 1);
    if (!pol.lds.count(l.x)) continue;
    ranges[l.x].push_back(l.y);
    if (l.y == -1) {
      whole = true;
      continue;
    }
    const int j = pol.top[(size_t)l.x] - l.y;
    CHECK(!whole && j >= last_j);
    last_j = std::max(last_j, j);
  }
  for (int v : pol.lds) {
    const std::vector<int> &r = ranges[v];
    if (rows[(size_t)v] <= per_wg) {
      CHECK(r.size() == 1 && r[0] == -1);
    } else {
      CHECK((int)r.size() == pol.top[(size_t)v] + 1);
      for (size_t i = 0; i < r.size(); ++i) CHECK(r[i] == pol.top[(size_t)v] - (int)i);  // (top .. 0, in that order)
    }
  }
}

static void random_properties() {
  std::mt19937 rng(20260119u);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  const int per_wg = 16;
  const ull heavy = 8;
  for (int draw = 0; draw < 300; ++draw) {
    const size_t nv = (size_t)(draw < 4 ? draw : rnd(0, 300));
    W work(std::max<size_t>(nv, 1), 0), wcut(work.size(), 0);
    I rows(work.size(), 0);
    for (size_t v = 0; v < nv; ++v) {
      work[v] = rnd(0, 9) < 3 ? 0 : (ull)rnd(1, 30);
      wcut[v] = rnd(0, 1) ? 0 : (ull)rnd(0, (int)work[v]);
      rows[v] = rnd(0, 3) ? rnd(0, 16) : rnd(17, 40);
    }
    const ull lds_min = (ull)rnd(1, 12);
    {  // rectangle, on ranges made by rect_lds_ranges out of random block maxima (16 words: ranges of 64 / 32 / 16 ids)
      const int words = 16, max_ranges = rnd(1, 6);
      I bmax(std::max<size_t>((nv + words - 1) / words, 1), 0);
      for (int &b : bmax) b = rnd(0, 5) ? rnd(0, 255) : rnd(0, 1) ? 300 : 70000;
      I rb((size_t)max_ranges + 1, -1), lb((size_t)max_ranges, -1);
      const int n = rect_lds_ranges((long long)nv, bmax, words, max_ranges, rb.data(), lb.data());
      CHECK(n <= max_ranges && (n > 0) == (nv > 0) && rb[(size_t)n] == (int)nv && rb[0] >= 0);
      for (int k = 0; k < n; ++k) CHECK(lb[(size_t)k] >= 3 && lb[(size_t)k] <= 5 && rb[(size_t)k] == std::max(0, rb[(size_t)k + 1] - (words << (5 - lb[(size_t)k]))));
      CHECK(n == max_ranges || rb[0] == 0);
      Policy pol;
      pol.front_key = wcut;
      pol.top.assign(work.size(), 0);
      for (size_t v = 0; v < nv; ++v) {
        if (work[v] == 0) continue;
        if (work[v] >= lds_min && (int)v > rb[0]) {
          pol.lds.insert((int)v);
          if (wcut[v] > 0) pol.front.insert((int)v);
          for (int k = 0; k < n; ++k)
            if (rb[(size_t)k] <= (int)v - 1) pol.top[v] = k;
        } else {
          pol.rest.insert((int)v);
        }
      }
      check_properties(rect_tasks(nv, work, wcut, rows, rb.data(), n, lds_min, per_wg, heavy), nv, work, rows, per_wg, heavy, pol);
    }
    {  // house
      const int n = rnd(0, 5);
      const bool given = rnd(0, 1);
      const ull per_walk = (ull)rnd(1, 10);
      Policy pol;
      pol.front_key.assign(work.size(), 0);
      pol.top.assign(work.size(), n - 1);
      for (size_t v = 0; v < nv; ++v) {
        if (work[v] == 0) continue;
        ull need = lds_min;  // (16 threads: every centre that fits them has at most 32 neighbours, four ranges per walk)
        if (!given && rows[v] <= per_wg) need = std::max<ull>(lds_min, per_walk * (ull)((n + 3) / 4));
        if (n > 0 && work[v] >= need) {
          pol.lds.insert((int)v);
          pol.front.insert((int)v);
          pol.front_key[v] = wcut[v] + (ull)rows[v];
        } else {
          pol.rest.insert((int)v);
        }
      }
      const CentreTasks t = house_tasks(nv, work, wcut, rows, n, lds_min, given, per_walk, per_wg, heavy);
      check_properties(t, nv, work, rows, per_wg, heavy, pol);
      size_t with_work = 0, in_acc = 0;  // the house keeps every centre with work in the acc list
      for (size_t v = 0; v < nv; ++v) with_work += work[v] > 0;
      for (const int4 &a : t.acc_tasks) in_acc += (a.x >= 0) + (a.y >= 0) + (a.z >= 0) + (a.w >= 0);
      CHECK(with_work == in_acc);
    }
  }
}

// ---- the ranges ------------------------------------------------------------------------------------------------------------------------
static void rect_ranges() {
  const int words = 16;  // ranges of 64 / 32 / 16 ids for 8- / 16- / 32-bit counters
  int rb[8], lb[8];
  auto is = [&](int n, const I &want_rb, const I &want_lb) {
    bool ok = (int)want_lb.size() == n && (int)want_rb.size() == n + 1;
    for (int k = 0; ok && k <= n; ++k) ok = rb[k] == want_rb[(size_t)k];
    for (int k = 0; ok && k < n; ++k) ok = lb[k] == want_lb[(size_t)k];
    return ok;
  };
  I small(13, 10);  // 200 ids = 13 blocks of 16
  CHECK(is(rect_lds_ranges(200, small, words, 7, rb, lb), {0, 8, 72, 136, 200}, {3, 3, 3, 3}));
  CHECK(is(rect_lds_ranges(200, small, words, 2, rb, lb), {72, 136, 200}, {3, 3}));  // max_ranges
  CHECK(is(rect_lds_ranges(200, small, words, 1, rb, lb), {136, 200}, {3}));
  CHECK(is(rect_lds_ranges(10, I(1, 10), words, 7, rb, lb), {0, 10}, {3}));  // less than one range
  CHECK(is(rect_lds_ranges(10, I(1, 70000), words, 7, rb, lb), {0, 10}, {5}));
  CHECK(is(rect_lds_ranges(0, I(1, 0), words, 7, rb, lb), {0}, {}));
  {  // a hub block at the top, a 16-bit block below it: 16 ids, then 32 (blocks 1 - 2), then 8-bit ranges of 64
    I b = small;
    b[0] = 70000;
    b[1] = 300;
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 24, 88, 152, 184, 200}, {3, 3, 3, 4, 5}));
  }
  {  // 255 / 256 at the edge of the 4-block look-ahead: block 3 is inside it from blocks 0 and 2, block 4 is not from block 0
    I b = small;
    b[3] = 255;
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 8, 72, 136, 200}, {3, 3, 3, 3}));
    b[3] = 256;
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 8, 72, 136, 168, 200}, {3, 3, 3, 4, 4}));
    b[3] = 10;
    b[4] = 256;
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 40, 104, 136, 200}, {3, 3, 4, 3}));  // (8 bits for blocks 0 - 3, then 16 for 4 - 5)
  }
  {  // 65535 / 65536 at the edge of the 2-block look-ahead
    I b = small;
    b[1] = 65535;
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 40, 104, 168, 200}, {3, 3, 3, 4}));
    b[1] = 65536;
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 40, 104, 168, 184, 200}, {3, 3, 3, 5, 5}));
    b[1] = 10;
    b[2] = 65536;  // (not among blocks 0 - 1: 16 bits there; the first of blocks 2 - 3: 32 bits)
    CHECK(is(rect_lds_ranges(200, b, words, 7, rb, lb), {0, 24, 88, 152, 168, 200}, {3, 3, 3, 5, 4}));
  }
}

// Seeded random block maxima, nv no multiple of the block: the ranges tile [rb[0], nv) without gap or overlap, and every range's counters
// hold the largest degree among the blocks it covers -- "degree < 2^(2^lb)" is what keeps a field of rect_lds_kernel from carrying into
// the next end's (a width one step too narrow is a wrong COUNT, not lost time).  blockmax[b] covers the ids [nv - (b + 1) words, nv - b words).
static void rect_ranges_random() {
  std::mt19937 rng(20261020u);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  const int edge[] = {0, 1, 254, 255, 256, 257, 65534, 65535, 65536, 65537, 1 << 20};
  for (int draw = 0; draw < 2000; ++draw) {
    const int words = 1 << rnd(2, 5), max_ranges = rnd(1, 12);
    const int nblk = rnd(1, 40);
    const long long nv = (long long)(nblk - 1) * words + rnd(1, words - 1);  // (the lowest block is a partial one)
    I bmax((size_t)nblk);
    for (int &b : bmax) b = rnd(0, 2) ? edge[rnd(0, 10)] : rnd(0, 3) ? rnd(0, 300) : rnd(0, 70000);
    I rb((size_t)max_ranges + 1, -1), lb((size_t)max_ranges, -1);
    const int n = rect_lds_ranges(nv, bmax, words, max_ranges, rb.data(), lb.data());
    CHECK(n >= 1 && n <= max_ranges && rb[(size_t)n] == (int)nv && rb[0] >= 0 && (n == max_ranges || rb[0] == 0));
    for (int k = 0; k < n; ++k) {
      const int lo = rb[(size_t)k], hi = rb[(size_t)k + 1], w = lb[(size_t)k];
      CHECK(lo < hi);  // ascending, no overlap; [rb[k], rb[k + 1]) follow each other by construction of the array: no gap
      CHECK(w >= 3 && w <= 5 && hi - lo <= (words << (5 - w)) && (hi - lo == (words << (5 - w)) || lo == 0));
      CHECK((nv - hi) % words == 0);  // ranges are whole blocks counted from the top
      if (lo >= hi) continue;
      int m = 0;  // largest degree among the blocks that hold an id of [lo, hi)
      for (long long b = (nv - hi) / words; b <= (nv - 1 - lo) / words; ++b) m = std::max(m, bmax[(size_t)b]);
      CHECK(w == 5 || (long long)m < (1ll << (1 << w)));
      if (w == 5) continue;
      // ... and not wider than the rule asks: the look-ahead window of the next narrower width holds a degree that needs this one
      int mw = 0;
      const long long b0 = (nv - hi) / words;
      for (long long b = b0; b < std::min<long long>(b0 + (w == 4 ? 4 : 0), nblk); ++b) mw = std::max(mw, bmax[(size_t)b]);
      if (w == 4) CHECK(mw >= 256);
    }
  }
}

static void house_ranges() {
  int cut = -1;
  CHECK(house_lds_ranges(200, 64, 256, &cut) == 4 && cut == 0);
  CHECK(house_lds_ranges(256, 64, 256, &cut) == 4 && cut == 0);
  CHECK(house_lds_ranges(200, 64, 2, &cut) == 2 && cut == 72);
  CHECK(house_lds_ranges(10, 64, 256, &cut) == 1 && cut == 0);
  CHECK(house_lds_ranges(0, 64, 256, &cut) == 0 && cut == 0);
  // the 4 GB cap of the row-bound table, (n + 1) ints per vertex: 10^8 vertices -> 10 columns -> 9 ranges; 2^31 - 1 -> one range
  CHECK(house_lds_ranges(100000000ll, 16384, 256, &cut) == 9 && cut == 100000000 - 9 * 16384);
  CHECK(house_lds_ranges(2147483647ll, 16384, 256, &cut) == 1 && cut == 2147483647 - 16384);
  CHECK(house_lds_ranges(1 << 20, 16384, 256, &cut) == 64 && cut == 0);  // (not engaged: 64 ranges cover the graph)
}

static void house_threshold() {
  // at most 32 neighbours: four ranges per walk; up to one per thread: two; more: per-range tasks, the plain threshold
  CHECK(house_lds_min_of(10, 111, 4096, false, 200, 1024) == 200ull * 28);
  CHECK(house_lds_min_of(32, 111, 4096, false, 200, 1024) == 200ull * 28);
  CHECK(house_lds_min_of(33, 111, 4096, false, 200, 1024) == 200ull * 56);
  CHECK(house_lds_min_of(1024, 111, 4096, false, 200, 1024) == 200ull * 56);
  CHECK(house_lds_min_of(1025, 111, 4096, false, 200, 1024) == 4096);
  CHECK(house_lds_min_of(10, 8, 4096, false, 200, 1024) == 4096);  // (never below the threshold itself)
  CHECK(house_lds_min_of(10, 111, 1, true, 200, 1024) == 1);      // a given threshold is taken as given
  CHECK(house_lds_min_of(100, 111, 9000, true, 200, 1024) == 9000);
}

static void wrect() {
  // ranges of 4 ids, 2 threads: 9, 7, 4 have more rows -- from the last id down, each from its top range ((v - 1) / 4) down; then the
  // centres with exactly 2 rows (one row cannot hold a 4-cycle), last id first
  const I idx0 = {0, 1, 1, 2, 3, 0, 2, 5, 1, 3};
  const std::vector<T2> want = {{9, 2}, {9, 1}, {9, 0}, {7, 1}, {7, 0}, {4, 0}, {6, -1}, {3, -1}};
  CHECK(same(wrect_tasks(idx0.data(), idx0.size(), 4, 2), want));
  CHECK(wrect_tasks(idx0.data(), 0, 4, 2).empty());
}

int main() {
  rect_literals();
  house_literals();
  random_properties();
  rect_ranges();
  rect_ranges_random();
  house_ranges();
  house_threshold();
  wrect();
  if (g_bad) {
    fprintf(stderr, "%d checks failed\n", g_bad);
    return 1;
  }
  printf("centre plan ok\n");
  return 0;
}
