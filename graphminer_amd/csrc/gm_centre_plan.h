// gm_centre_plan.h -- the once-per-graph plans of the map solvers (rectangle / house by wedge accumulation, the weighted 4-cycles) as pure
// functions of host arrays: no HIP runtime, no globals, no developer options (gm_solve_sgl.hip reads those and builds the device side).  A slip
// in the ORDER or the grouping of the tasks costs time, not counts, so no parity test sees it: tests/centre_plan_host_check.cc checks them
// with a plain host compiler.  The counter widths lb[] of rect_lds_ranges and the row limits that choose a field width are another matter: one
// step too narrow and a counter carries into the field of the neighbouring end -- a wrong count.  The host check holds every range's lb against
// the degrees of the blocks it covers, and tests/test_gpu_map_kernels.py puts counters on the last value of every width.
#pragma once
#include <hip/hip_vector_types.h>

#include <algorithm>
#include <vector>

namespace gm {

// house_lds_kernel, a one-task centre: up to this many neighbours its ends count in 6 + 10-bit fields (n <= 32, S <= 32 * 31 = 992 < 2^10), two to a
// word and four ranges per walk; above it 11 + 21-bit fields, two ranges per walk.  The kernel and house_lds_min_of below read the same constant.
constexpr int kHouseFw16Rows = 32;

// The tasks of the map kernels (rect_acc_kernel / pent_acc_kernel / house_acc_kernel) from centres ordered heaviest first: a centre with at
// least `heavy` 2-paths gets a whole workgroup (a task of its own), the light ones go four to a task
inline void emit_centre_tasks(const std::vector<int> &vs, const unsigned long long *w, unsigned long long heavy, std::vector<int4> &tasks) {
  size_t i = 0;
  for (; i < vs.size() && w[(size_t)vs[i]] >= heavy; ++i) tasks.push_back(make_int4(vs[i], -2, -2, -2));
  for (; i < vs.size(); i += 4) {
    int4 t = make_int4(vs[i], -1, -1, -1);
    if (i + 1 < vs.size()) t.y = vs[i + 1];
    if (i + 2 < vs.size()) t.z = vs[i + 2];
    if (i + 3 < vs.size()) t.w = vs[i + 3];
    tasks.push_back(t);
  }
}

// The rectangle's ranges, from the last ids down (the hubs of a graph numbered ascending in degree): a range's counters are as wide as the largest
// degree among its vertices needs -- 8 / 16 bits while the next 4 / 2 blocks stay below 256 / 65536 -- so it covers words << (5 - lb) ids.  blockmax[b] =
// largest degree among the ids [nv - (b + 1) words, nv - b words).  Fills rb[0 .. n] (ascending, rb[0] = the cut, rb[n] = nv), lb[0 .. n); returns n <= max_ranges.
inline int rect_lds_ranges(long long nv, const std::vector<int> &blockmax, int words, int max_ranges, int *rb, int *lb) {
  auto max_deg_of_blocks = [&](int b0, int nb) {  // blocks b0 .. b0 + nb - 1 (counted from the top), those that exist
    int m = 0;
    for (int b = b0; b < std::min(b0 + nb, (int)blockmax.size()); ++b) m = std::max(m, blockmax[(size_t)b]);
    return m;
  };
  int n = 0, blk = 0;
  rb[0] = (int)nv;
  for (long long hi = nv; hi > 0 && n < max_ranges; ++n) {  // (from the top down, turned round below)
    lb[n] = max_deg_of_blocks(blk, 4) < 256 ? 3 : max_deg_of_blocks(blk, 2) < 65536 ? 4 : 5;
    blk += 1 << (5 - lb[n]);
    hi = std::max<long long>(0, hi - ((long long)words << (5 - lb[n])));
    rb[n + 1] = (int)hi;
  }
  std::reverse(rb, rb + n + 1);
  std::reverse(lb, lb + n);
  return n;
}
// The house's: n ranges (returned) of `ids` ids from the last id down, *cut = their first id; the row-bound table, n + 1 ints per vertex, stays within 4 GB
inline int house_lds_ranges(long long nv, int ids, int max_ranges, int *cut) {
  const long long by_memory = std::max<long long>(1, (4ll << 30) / (4ll * std::max<long long>(nv, 1)) - 1);
  const int n = (int)std::min<long long>(std::min<long long>(max_ranges, by_memory), (nv + ids - 1) / ids);
  *cut = (int)std::max<long long>(0, nv - (long long)n * ids);
  return n;
}
// The 2-paths from which a centre of the house goes to the LDS maps.  A centre with at most one neighbour per thread (per_wg) is ONE task
// that walks every range -- two per walk -- at ~2.5 us of a CU per walk whatever it finds there, against ~12 ns per 2-path in the global
// maps (both measured on R-MAT-20): it pays from ~200 2-paths per walk on.  (On a LiveJournal-sized power-law graph -- 4.8 M vertices,
// 111 walks -- the fixed 4096 made the house 1.27 x SLOWER than the global maps.)  A developer option that sets the threshold is taken as given.
inline unsigned long long house_lds_min_of(int degree, int n_ranges, unsigned long long lds_min, bool lds_min_given, unsigned long long per_walk, int per_wg) {
  if (lds_min_given || degree > per_wg) return lds_min;
  const int per = degree <= kHouseFw16Rows ? 4 : 2;  // ranges per walk (house_lds_kernel: 16-bit counters up to kHouseFw16Rows neighbours)
  return std::max<unsigned long long>(lds_min, per_walk * (unsigned long long)((n_ranges + per - 1) / per));
}
struct CentreTasks {
  std::vector<int2> lds_tasks;  // {v, k}: range k of centre v; {v, -1}: every range of a centre with at most per_wg rows
  std::vector<int4> acc_tasks;  // emit_centre_tasks' form; the first n_cut: LDS centres, which walk only their ends below the cut
  unsigned long long n_cut = 0;
};
// Both task lists of a pattern; where the rectangle and the house differ is what the caller passes:
//   is_lds(v)     the centre counts in LDS maps (asked of the centres with work[v] > 0)
//   top_range(v)  the highest range its ends can lie in: a centre with more rows[v] than the workgroup has threads (per_wg) gets a task per
//                 range top_range(v) .. 0, every centre's own top range first; the others one {v, -1} task
//   front_key(v)  what is left of an LDS centre for the acc kernel, which takes those centres first, ordered by it;
//   keep_zero_key those with nothing left too, or not
// Within a list the centres go heaviest first (by work[]; the front by its key), equal ones in the order they had before.
template <class IsLds, class TopRange, class FrontKey>
CentreTasks plan_centre_tasks(size_t nv, const unsigned long long *work, const int *rows, int n_ranges, int per_wg, unsigned long long heavy, IsLds is_lds, TopRange top_range,
                              FrontKey front_key, bool keep_zero_key) {
  std::vector<int> lds, rest, front;
  for (size_t v = 0; v < nv; ++v)
    if (work[v] > 0) (is_lds((int)v) ? lds : rest).push_back((int)v);
  auto by = [](const unsigned long long *w) { return [w](int a, int b) { return w[(size_t)a] > w[(size_t)b]; }; };
  std::stable_sort(lds.begin(), lds.end(), by(work));
  std::stable_sort(rest.begin(), rest.end(), by(work));
  CentreTasks out;
  for (int j = 0; j < n_ranges; ++j)
    for (int v : lds)
      if (const int k = top_range(v) - j; rows[(size_t)v] > per_wg && k >= 0) out.lds_tasks.push_back(make_int2(v, k));
  for (int v : lds)
    if (rows[(size_t)v] <= per_wg) out.lds_tasks.push_back(make_int2(v, -1));
  std::vector<unsigned long long> key(nv, 0);
  for (int v : lds)
    if ((key[(size_t)v] = front_key(v)) > 0 || keep_zero_key) front.push_back(v);
  std::stable_sort(front.begin(), front.end(), by(key.data()));
  emit_centre_tasks(front, key.data(), heavy, out.acc_tasks);
  out.n_cut = out.acc_tasks.size();
  emit_centre_tasks(rest, work, heavy, out.acc_tasks);
  return out;
}
// The rectangle's policy: a centre's ends lie below it, so only a centre above the cut rb[0] has any in the ranges, the highest of them in
// the range of v - 1; what the ranges leave of it are its ends below the cut (wcut) -- none when they cover the whole graph
inline CentreTasks plan_rect_tasks(size_t nv, const unsigned long long *work, const unsigned long long *wcut, const int *idx0, const int *rb, int n, unsigned long long lds_min, int per_wg,
                                   unsigned long long heavy) {
  auto range_of = [&](int w) { return (int)(std::upper_bound(rb + 1, rb + std::max(n, 1), w) - rb) - 1; };  // the range that holds id w >= rb[0]
  return plan_centre_tasks(
      nv, work, idx0, n, per_wg, heavy, [&](int v) { return work[(size_t)v] >= lds_min && v > rb[0]; }, [&](int v) { return range_of(v - 1); }, [&](int v) { return wcut[(size_t)v]; }, false);
}
// The house's: a threshold per walk, every range for every centre -- the hubs' ranges first: they hold most ends -- and EVERY LDS centre in
// front of house_acc_kernel's list: its phase 0 -- the table terms and the intersections -- is done there, and of its 2-paths the ends
// below the cut; ordered by that remainder, the intersections taken as its degree
inline CentreTasks plan_house_tasks(size_t nv, const unsigned long long *work, const unsigned long long *wcut, const int *deg, int n, unsigned long long lds_min, bool lds_min_given,
                                    unsigned long long per_walk, int per_wg, unsigned long long heavy) {
  return plan_centre_tasks(
      nv, work, deg, n, per_wg, heavy, [&](int v) { return n > 0 && work[(size_t)v] >= house_lds_min_of(deg[(size_t)v], n, lds_min, lds_min_given, per_walk, per_wg); },
      [&](int) { return n - 1; }, [&](int v) { return wcut[(size_t)v] + (unsigned long long)deg[(size_t)v]; }, true);
}
// The tasks of wrect_kernel: the centres with more neighbours below them (idx0) than the workgroup has threads first, a task per range of
// `range` ids (from the last id down, every centre's top range first), then one task per remaining centre that can hold a 4-cycle
inline std::vector<int2> wrect_tasks(const int *idx0, size_t nv, int range, int per_wg) {
  std::vector<int2> tasks;
  for (long long v0 = (long long)nv - 1; v0 >= 0; --v0)
    if (idx0[(size_t)v0] > per_wg)
      for (int k = (int)((v0 - 1) / range); k >= 0; --k) tasks.push_back(make_int2((int)v0, k));
  for (long long v0 = (long long)nv - 1; v0 >= 0; --v0)
    if (idx0[(size_t)v0] >= 2 && idx0[(size_t)v0] <= per_wg) tasks.push_back(make_int2((int)v0, -1));
  return tasks;
}

}  // namespace gm
