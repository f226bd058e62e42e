// gm_solve_local.hip -- local counts, the k-truss, the triangle and k-clique listings, the local k-clique and 4-cycle counts over the launch layer (gm_launch.h):
// gm_tc_local, gm_ktruss, gm_truss_decompose, gm_tc_list, gm_clique_list, gm_clique_local, gm_rect_local, gm_motif_local, gm_clique_kcore,
// gm_clique_core_decompose, gm_clique_ktruss, gm_clique_truss_decompose, gm_tri_clique4_local, gm_nucleus34, gm_nucleus34_decompose.  Host code only: the kernels are
// gm_local.hip's, gm_list.hip's, gm_clique_list.hip's, gm_kcl_local.hip's, gm_kcl_core.hip's, gm_kcl_truss.hip's, gm_nucleus34.hip's, gm_rect_local.hip's and gm_orbit_local.hip's, so this unit has no code object and no warm-up.
#include "gm_launch.h"
#include "gm_orbit.h"

// ---- local counts and the k-truss (gm_local.hip; DESIGN.md "Local counts and k-truss") ----------------------------------------------------
// the arrays of the symmetric handle, in the caller's entry order (peel: also the marks, the frontier list and the round counters)
static int ensure_local_buffers(gm_graph *g, bool peel, bool truss) {
  std::lock_guard<std::mutex> lk(g->mu);
  HIP_TRY(hipSetDevice(g->device));
  const size_t ne = (size_t)std::max<long long>(g->ne, 1);
  if (!g->local.ent) HIP_TRY(g->local.ent.alloc(sizeof(unsigned) * ne));
  if (peel) {
    if (!g->local.mark) HIP_TRY(g->local.mark.alloc(ne));
    if (!g->local.front) HIP_TRY(g->local.front.alloc(sizeof(int) * (ne / 2 + 1)));
    if (!g->local.cnt) HIP_TRY(g->local.cnt.alloc(64));
  }
  if (truss && !g->local.truss) HIP_TRY(g->local.truss.alloc(sizeof(unsigned) * ne));
  return GM_OK;
}

// the refusals the three calls share, in the order of the header
static int local_refusals(const gm_graph *sym, const gm_launch *la) {
  if (!sym) return GM_ERR_INVALID;
  if (int rc = reject_big(sym)) return rc;
  if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;  // (the arrays are whole-graph results, read back by the call)
  return GM_OK;
}

// The supports of every entry of the oriented copy -- one rank's PAT_SUPPORT_PART into run_on->local.sup, every path of the triangle pass --
// and their way back: `c` is the open launch on the SYMMETRIC handle, the mapping kernel writes `out` (caller's entry order) and adds the
// sum of the supports to its counters[0].
static int local_supports(gm_graph *g, const gm_launch *l2, SubLaunches &sub, gm_graph **run_on_out) {
  gm_graph *run_on = nullptr;
  if (int rc = diamond_run_on(g, l2, &run_on)) return rc;
  {
    std::lock_guard<std::mutex> lk(run_on->mu);
    if (!run_on->local.sup) HIP_TRY(run_on->local.sup.alloc(sizeof(unsigned) * (size_t)diamond_support_entries(run_on->ne, 1)));
  }
  uint64_t dummy = 0;
  if (int rc = sub.run([&](gm_stats *s) { return run_pattern({PAT_SUPPORT_PART, 3, -1, 0, run_on->local.sup}, run_on, l2, &dummy, 1, s); })) return rc;
  *run_on_out = run_on;
  return GM_OK;
}
static int local_map(LaunchCtx &c, gm_graph *run_on, unsigned *out) {
  gm_graph *g = c.g;
  const gm_graph *dag = g->dag_cache;
  if (run_on != dag && !run_on->d_newid) return GM_ERR_INVALID;  // (a renumbered copy always remembers its numbering)
  LocalMapParams mp;
  memset(&mp, 0, sizeof mp);
  mp.nv = g->nv; mp.ne = g->ne; mp.rp = g->d_rp; mp.col = g->d_col;
  mp.newid = run_on != dag ? run_on->d_newid : nullptr;  // (the oriented copy keeps the symmetric graph's ids: one level of numbering)
  mp.drp = run_on->d_rp; mp.dcol = run_on->d_col; mp.dsup = run_on->local.sup;
  mp.topo = *run_on->facts.topological ? 1 : 0;
  mp.out = out; mp.sum = g->d_counters;
  HIP_TRY(launch_local_map(mp, g->cu_count, c.stream));
  return GM_OK;
}

extern "C" int gm_tc_local(const gm_graph *sym, const gm_launch *la, uint64_t *d_vertex_tri, uint32_t *d_entry_sup, uint64_t *total, gm_stats *st) {
  if (int rc = local_refusals(sym, la)) return rc;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  uint64_t sum = 0;
  if (total) *total = 0;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &sum, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  if (sym->ne == 0) {
    if (d_vertex_tri && sym->nv > 0) HIP_TRY(hipMemsetAsync(d_vertex_tri, 0, sizeof(uint64_t) * (size_t)sym->nv, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    return GM_OK;
  }
  if (int rc = ensure_local_buffers(g, false, false)) return rc;
  SubLaunches sub;
  gm_graph *run_on = nullptr;
  if (int rc = local_supports(g, &l2, sub, &run_on)) return rc;
  HIP_TRY(hipMemsetAsync(g->d_counters, 0, kCounterBlockBytes, ctx.stream));  // (a first call oriented the graph since begin_launch)
  if (int rc = start_timer(ctx)) return rc;
  unsigned *ent = d_entry_sup ? d_entry_sup : g->local.ent;
  if (int rc = local_map(ctx, run_on, ent)) return rc;
  if (d_vertex_tri) HIP_TRY(launch_local_vertices(g->nv, g->d_rp, ent, (unsigned long long *)d_vertex_tri, g->cu_count, ctx.stream));
  if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, &sum, 1, s); })) return rc;
  if (total) *total = sum / 6ull;  // sum_e t(e) over both directions = 2 sum_v T_v = 6 T
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

// ---- local k-clique counts (gm_kcl_local.hip; DESIGN.md "Local k-clique counts") -----------------------------------------------------------
// The k-cliques of every entry of the DAG (the oriented copy, or its topological copy: topo_view) into run_on->local.kcl, then the way back
// the supports take: the 64-bit mapping kernel into the caller's entry order, the row sums / (k - 1) per vertex.
constexpr size_t kKclScratchBudget = (size_t)1 << 30;  // bytes of scratch slots the wide kernel's grid is cut to (at least one slot)
extern "C" int gm_clique_local(const gm_graph *sym, int k, const gm_launch *la, uint64_t *d_vertex_cnt, uint64_t *d_entry_cnt, uint64_t *total,
                               gm_stats *st) {
  if (total) *total = 0;
  if (!sym || k < 3 || k > GM_MAX_CLIQUE_K) return GM_ERR_INVALID;
  if (int rc = local_refusals(sym, la)) return rc;
  if (k > 8) {
    g_last_error = "gm_clique_local: k = 9 .. " + std::to_string(GM_MAX_CLIQUE_K) + " is not supported yet (3 <= k <= 8)";
    return GM_ERR_UNSUPPORTED;
  }
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t out[4] = {0, 0, 0, 0};
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, out, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  if (sym->ne == 0) {
    if (d_vertex_cnt && sym->nv > 0) HIP_TRY(hipMemsetAsync(d_vertex_cnt, 0, sizeof(uint64_t) * (size_t)sym->nv, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    return GM_OK;
  }
  gm_graph *run_on = nullptr;
  if (int rc = diamond_run_on(g, &l2, &run_on)) return rc;  // (the oriented copy, or its topological copy: tune[6] & GM_T6_AS_NUMBERED)
  const gm_graph *dag = g->dag_cache;
  if (run_on != dag && !run_on->d_newid) return GM_ERR_INVALID;  // (a renumbered copy always remembers its numbering)
  const bool wide = run_on->max_deg > kKclLocalLdsRow;
  const size_t slot_bytes = sizeof(unsigned) * (size_t)kcl_local_scratch_words(run_on->max_deg);
  const int grid = grid_for(run_on->nv, g->cu_count, 8);
  const int grid_wide = wide ? clamp_grid((long long)(kKclScratchBudget / slot_bytes), (long long)g->cu_count * 2) : 0;
  const size_t heavy_cap = (size_t)(run_on->ne / (kKclLocalLdsRow + 1)) + 1, mid_cap = (size_t)(run_on->ne / (kKclLocalSplitRow + 1)) + 1;
  const size_t dne = (size_t)std::max<long long>(run_on->ne, 1);
  {
    std::lock_guard<std::mutex> lk(run_on->mu);
    HIP_TRY(hipSetDevice(run_on->device));
    if (!run_on->local.kcl) HIP_TRY(run_on->local.kcl.alloc(sizeof(unsigned long long) * 2 * dne));
    if (!run_on->local.kcl_heavy) HIP_TRY(run_on->local.kcl_heavy.alloc(sizeof(int) * (heavy_cap + mid_cap)));
    if (wide)
      if (int rc = grow_dev(run_on->local.kcl_scratch, &run_on->local.kcl_scratch_bytes, slot_bytes * (size_t)grid_wide)) return rc;
  }
  if (!d_entry_cnt) {
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->local.ent64) HIP_TRY(g->local.ent64.alloc(sizeof(unsigned long long) * (size_t)g->ne));
  }
  HIP_TRY(hipMemsetAsync(g->d_counters, 0, kCounterBlockBytes, ctx.stream));  // (a first call oriented the graph since begin_launch)
  if (int rc = start_timer(ctx)) return rc;
  HIP_TRY(hipMemsetAsync(run_on->local.kcl, 0, sizeof(unsigned long long) * 2 * dne, ctx.stream));
  KclLocalParams kp;
  memset(&kp, 0, sizeof kp);
  kp.nv = run_on->nv; kp.ne = run_on->ne; kp.k = k; kp.max_deg = std::max(run_on->max_deg, 1);
  kp.rp = run_on->d_rp; kp.col = run_on->d_col; kp.cnt = run_on->local.kcl; kp.spk = run_on->local.kcl + dne;
  kp.heavy = run_on->local.kcl_heavy; kp.heavy_cap = (unsigned)heavy_cap;
  kp.mid = run_on->local.kcl_heavy + heavy_cap; kp.mid_cap = (unsigned)mid_cap;
  kp.queue = queue_word(g, QW_MAIN); kp.queue_wide = queue_word(g, QW_CLASS1); kp.n_heavy = queue_word(g, QW_CLASS2);
  kp.queue_mid = queue_word(g, QW_CLASS3); kp.n_mid = queue_word(g, QW_CORNER);
  kp.scratch = run_on->local.kcl_scratch; kp.scratch_words = kcl_local_scratch_words(run_on->max_deg);
  kp.err = g->d_counters + 1;
  HIP_TRY(launch_kcl_local(kp, KCL_STAGE_ROOTS, grid, ctx.stream));
  if (k >= 5 && run_on->max_deg > kKclLocalSplitRow) HIP_TRY(launch_kcl_local(kp, KCL_STAGE_SPLIT, grid, ctx.stream));
  if (wide) HIP_TRY(launch_kcl_local(kp, KCL_STAGE_WIDE, grid_wide, ctx.stream));
  HIP_TRY(launch_kcl_local(kp, KCL_STAGE_FOLD, grid_for((run_on->ne + 255) / 256, g->cu_count, 8), ctx.stream));
  LocalMapParams64 mp;
  memset(&mp, 0, sizeof mp);
  mp.nv = g->nv; mp.ne = g->ne; mp.rp = g->d_rp; mp.col = g->d_col;
  mp.newid = run_on != dag ? run_on->d_newid : nullptr;
  mp.drp = run_on->d_rp; mp.dcol = run_on->d_col; mp.dsup = run_on->local.kcl;
  mp.topo = *run_on->facts.topological ? 1 : 0;
  unsigned long long *ent = d_entry_cnt ? (unsigned long long *)d_entry_cnt : g->local.ent64.get();
  mp.out = ent; mp.sum = g->d_counters;
  HIP_TRY(launch_local_map(mp, g->cu_count, ctx.stream));
  if (d_vertex_cnt) HIP_TRY(launch_local_vertices(g->nv, g->d_rp, ent, (unsigned)(k - 1), (unsigned long long *)d_vertex_cnt, g->cu_count, ctx.stream));
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_RAW4, 0, out, 4, &s)) return rc;
  if (out[1] != 0) {
    g_last_error = "gm_clique_local: the kernel met " + std::to_string(out[1]) + " adjacent pairs without an entry (internal error)";
    return GM_ERR_INVALID;
  }
  if (total) *total = out[0] / ((uint64_t)k * (uint64_t)(k - 1));  // sum_e K_e over both directions = k (k - 1) K
  if (st) {
    st->kernel_ms = s.kernel_ms;
    st->grid = (uint32_t)grid;
  }
  return GM_OK;
}

// ---- local 4-cycle counts (gm_rect_local.hip; DESIGN.md "Local 4-cycle counts") -----------------------------------------------------------
// The credits of every entry of the graph the walk runs on -- the copy numbered ascending in degree (the one run_wrect takes), or the handle
// itself (tune[6] & GM_T6_AS_NUMBERED) -- into run_on->local.racc, then back: the mapping kernel sums the two entries of an edge into the
// caller's entry order, the row sums / 2 per vertex.  The plan is built once per graph that runs it: GM_RECT_LOCAL_RANGE (ids per LDS
// range, default and limit kRectLocalRange) is read then.
extern "C" int gm_rect_local(const gm_graph *sym, const gm_launch *la, uint64_t *d_vertex_cnt, uint64_t *d_entry_cnt, uint64_t *total, gm_stats *st) {
  if (total) *total = 0;
  if (int rc = local_refusals(sym, la)) return rc;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kRectLocalThreads);
  uint64_t out[4] = {0, 0, 0, 0};
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, out, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  if (sym->ne == 0) {
    if (d_vertex_cnt && sym->nv > 0) HIP_TRY(hipMemsetAsync(d_vertex_cnt, 0, sizeof(uint64_t) * (size_t)sym->nv, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    return GM_OK;
  }
  gm_graph *run_on = g;
  if (!(l2.tune[6] & GM_T6_AS_NUMBERED)) {
    if (int rc = get_relabeled(g, 0, &run_on)) return rc;
    if (!run_on->d_newid) return GM_ERR_INVALID;  // (a renumbered copy always remembers its numbering)
  }
  if (int rc = ensure_idx0(run_on, graph_view(run_on))) return rc;
  if (const int rc = run_on->rect_local.ensure(run_on->mu, [&](RectLocalPlan &rl) {  // (two first calls on one handle: one builds, the other waits)
        OtherSetupScope scope(run_on);
        const size_t nv = (size_t)run_on->nv;
        int range = kRectLocalRange;
        if (const char *e = gm_opt("GM_RECT_LOCAL_RANGE")) range = std::max(16, std::min(kRectLocalRange, std::atoi(e)));
        const long long nranges = std::max<long long>(1, ((long long)run_on->nv + range - 1) / range);
        rl.range = range;
        rl.grp = (int)((nranges + 63) / 64);
        HIP_TRY(rl.mask.alloc(sizeof(unsigned long long) * std::max<size_t>(nv, 1)));
        HIP_TRY(launch_wrect_mask(run_on->nv, run_on->d_rp, run_on->d_col, range, rl.grp, rl.mask, run_on->cu_count, 0));
        std::vector<int> idx0h(std::max<size_t>(nv, 1));
        if (nv) HIP_TRY(hipMemcpy(idx0h.data(), run_on->rect_idx->idx0, sizeof(int) * nv, hipMemcpyDeviceToHost));
        const std::vector<int2> tasks = wrect_tasks(idx0h.data(), nv, range, kRectLocalThreads);  // (the hubs' per-range tasks first)
        rl.n_tasks = tasks.size();
        HIP_TRY(rl.tasks.alloc(sizeof(int2) * std::max<size_t>(tasks.size(), 1)));
        if (!tasks.empty()) HIP_TRY(hipMemcpy(rl.tasks, tasks.data(), sizeof(int2) * tasks.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());
        return kOnceBuilt;
      })) return rc;
  const size_t dne = (size_t)std::max<long long>(run_on->ne, 1);
  {
    std::lock_guard<std::mutex> lk(run_on->mu);
    if (!run_on->local.racc) HIP_TRY(run_on->local.racc.alloc(sizeof(unsigned long long) * dne));
  }
  if (!d_entry_cnt) {
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->local.ent64) HIP_TRY(g->local.ent64.alloc(sizeof(unsigned long long) * (size_t)g->ne));
  }
  HIP_TRY(hipMemsetAsync(g->d_counters, 0, kCounterBlockBytes, ctx.stream));  // (a first call renumbered the graph since begin_launch)
  if (int rc = start_timer(ctx)) return rc;
  HIP_TRY(hipMemsetAsync(run_on->local.racc, 0, sizeof(unsigned long long) * dne, ctx.stream));
  const RectLocalPlan &plan = *run_on->rect_local;
  RectLocalParams p;
  memset(&p, 0, sizeof p);
  p.rp = run_on->d_rp; p.col = run_on->d_col; p.idx0 = run_on->rect_idx->idx0;
  p.rmask = plan.mask; p.range = plan.range; p.grp = plan.grp;
  p.tasks = plan.tasks; p.count = plan.n_tasks;
  p.queue = queue_word64(g, QW64_MAIN);
  p.acc = run_on->local.racc;
  const int grid = grid_for((long long)p.count, g->cu_count, rect_local_per_cu());
  if (p.count > 0) HIP_TRY(launch_rect_local(p, grid, ctx.stream));
  RectLocalMapParams mp;
  memset(&mp, 0, sizeof mp);
  mp.nv = g->nv; mp.ne = g->ne; mp.rp = g->d_rp; mp.col = g->d_col;
  mp.newid = run_on != g ? run_on->d_newid.get() : nullptr;
  mp.drp = run_on->d_rp; mp.dcol = run_on->d_col; mp.acc = run_on->local.racc;
  unsigned long long *ent = d_entry_cnt ? (unsigned long long *)d_entry_cnt : g->local.ent64.get();
  mp.out = ent; mp.sum = g->d_counters;
  HIP_TRY(launch_rect_local_map(mp, g->cu_count, ctx.stream));
  // (every 4-cycle at v uses two of v's entries)
  if (d_vertex_cnt) HIP_TRY(launch_local_vertices(g->nv, g->d_rp, ent, 2u, (unsigned long long *)d_vertex_cnt, g->cu_count, ctx.stream));
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_RAW4, 0, out, 4, &s)) return rc;
  if (total) *total = out[0] / 8ull;  // sum_e R_e over both directions = 2 sum_v R_v = 8 R
  if (st) {
    st->kernel_ms = s.kernel_ms;
    st->chunks = (uint64_t)p.count;
    st->grid = (uint32_t)grid;
  }
  return GM_OK;
}

// ---- local motif counts (gm_orbit_local.hip; DESIGN.md "Local motif counts") ---------------------------------------------------------------
// The graphlet-degree orbits of every vertex, put together from the three local counts above on the same handle -- gm_tc_local leaves the
// supports in the caller's entry order in g->local.ent and T_v in the call's own array, gm_rect_local R_v, gm_clique_local(4) K_v -- and
// from the one input none of them has: the diamond-rim credits W of the DAG entries (PAT_ORBIT: the weighted pass's walk over the triangles
// of run_on, reading run_on->local.sup as gm_tc_local left it).  W goes back the k-cliques' way -- the 64-bit mapping kernel into
// g->local.ent64, half the row sums per vertex -- and is reduced to its vertex array BEFORE the rectangles and the k-cliques overwrite
// ent64.  k = 3 stops after gm_tc_local: one gather.  One kernel_ms covers every sub-launch.
extern "C" int gm_motif_local(const gm_graph *sym, int k, const gm_launch *la, uint64_t *d_orbits, uint64_t *counts, int ncounts, gm_stats *st) {
  if (!sym || (k != 3 && k != 4)) return GM_ERR_INVALID;
  const int nc = k == 3 ? 2 : 6, no = k == 3 ? kOrbits3 : kOrbits4;
  if (counts && ncounts != nc) return GM_ERR_INVALID;
  if (counts) for (int i = 0; i < nc; ++i) counts[i] = 0;
  if (int rc = local_refusals(sym, la)) return rc;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  fill_stats(st, (uint64_t)sym->ne, 0, 0, 256);
  uint64_t unused = 0;
  {
    LaunchCtx ctx;
    if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;  // (selects the device; refuses unsorted rows)
    if (sym->ne == 0) {
      if (d_orbits && sym->nv > 0) HIP_TRY(hipMemsetAsync(d_orbits, 0, sizeof(uint64_t) * (size_t)no * (size_t)sym->nv, ctx.stream));
      HIP_TRY(hipStreamSynchronize(ctx.stream));
      return GM_OK;
    }
  }
  const size_t nvz = (size_t)std::max(g->nv, 1);
  {
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->local.orb) HIP_TRY(g->local.orb.alloc(sizeof(unsigned long long) * (5 * nvz + 8)));
  }
  unsigned long long *tv = g->local.orb, *rv = tv + nvz, *kv = rv + nvz, *w2 = kv + nvz, *e1 = w2 + nvz, *sums = e1 + nvz;
  SubLaunches sub;
  if (int rc = sub.run([&](gm_stats *s) { return gm_tc_local(sym, &l2, (uint64_t *)tv, nullptr, nullptr, s); })) return rc;
  if (k == 4) {
    gm_graph *run_on = nullptr;
    if (int rc = diamond_run_on(g, &l2, &run_on)) return rc;  // (the copy gm_tc_local's supports were counted on)
    const gm_graph *dag = g->dag_cache;
    if (!run_on->local.sup || (run_on != dag && !run_on->d_newid)) return GM_ERR_INVALID;
    {
      std::lock_guard<std::mutex> lk(run_on->mu);
      HIP_TRY(hipSetDevice(run_on->device));
      if (!run_on->local.wacc) HIP_TRY(run_on->local.wacc.alloc(sizeof(unsigned long long) * (size_t)std::max<long long>(run_on->ne, 1)));
    }
    PatternReq credits{PAT_ORBIT, 3};
    credits.credit_sup = run_on->local.sup;
    credits.credit_w = run_on->local.wacc;
    if (int rc = sub.run([&](gm_stats *s) { return run_pattern(credits, run_on, &l2, &unused, 1, s); })) return rc;
    {
      std::lock_guard<std::mutex> lk(g->mu);
      if (!g->local.ent64) HIP_TRY(g->local.ent64.alloc(sizeof(unsigned long long) * (size_t)g->ne));
    }
    LaunchCtx ctx;
    if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;
    if (int rc = start_timer(ctx)) return rc;
    LocalMapParams64 mp;
    memset(&mp, 0, sizeof mp);
    mp.nv = g->nv; mp.ne = g->ne; mp.rp = g->d_rp; mp.col = g->d_col;
    mp.newid = run_on != dag ? run_on->d_newid.get() : nullptr;
    mp.drp = run_on->d_rp; mp.dcol = run_on->d_col; mp.dsup = run_on->local.wacc;
    mp.topo = *run_on->facts.topological ? 1 : 0;
    mp.out = g->local.ent64; mp.sum = g->d_counters;
    HIP_TRY(launch_local_map(mp, g->cu_count, ctx.stream));
    // (the row sum of W is even: N12 + N13 = half of it)
    HIP_TRY(launch_local_vertices(g->nv, g->d_rp, g->local.ent64, 2u, w2, g->cu_count, ctx.stream));
    if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, &unused, 1, s); })) return rc;
    if (int rc = sub.run([&](gm_stats *s) { return gm_rect_local(sym, &l2, (uint64_t *)rv, nullptr, nullptr, s); })) return rc;
    if (int rc = sub.run([&](gm_stats *s) { return gm_clique_local(sym, 4, &l2, (uint64_t *)kv, nullptr, nullptr, s); })) return rc;
  }
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;
  if (int rc = start_timer(ctx)) return rc;
  HIP_TRY(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * 8, ctx.stream));
  OrbitFinishParams fp;
  memset(&fp, 0, sizeof fp);
  fp.nv = g->nv; fp.rp = g->d_rp; fp.col = g->d_col; fp.tv = tv;
  fp.orbits = (unsigned long long *)d_orbits; fp.sums = sums;
  if (k == 4) {
    fp.ent = g->local.ent; fp.rv = rv; fp.kv = kv; fp.w2 = w2; fp.e1 = e1;
    HIP_TRY(launch_orbit_e1(g->nv, g->d_rp, g->d_col, e1, g->cu_count, ctx.stream));
  }
  HIP_TRY(launch_orbit_finish(fp, k, g->cu_count, ctx.stream));
  unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, ctx.stream));
  if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, &unused, 1, s); })) return rc;  // (synchronises the stream)
  if (counts) {
    if (k == 3) {
      counts[0] = h[0];
      counts[1] = h[1] / 3ull;
    } else {  // [3-star, 4-path, tailed triangle, 4-cycle, diamond, 4-clique]: sum o7, o4 / 2, o9, o8 / 4, o13 / 2, o14 / 4
      const unsigned long long div[6] = {1, 2, 1, 4, 2, 4};
      for (int i = 0; i < 6; ++i) counts[i] = h[i] / div[i];
    }
  }
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

// gm_ktruss (decompose = false) and gm_truss_decompose: the supports in the caller's order, then whole-frontier rounds.  One 8-byte word
// comes back per round: the frontier's size and the smallest support that stays alive.
static int run_truss(const gm_graph *sym, bool decompose, int k_in, const gm_launch *la, uint32_t *d_out, uint64_t *n_edges, int32_t *k_max,
                     int32_t *rounds_out, gm_stats *st) {
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  if (n_edges) *n_edges = 0;
  if (k_max) *k_max = 0;
  if (rounds_out) *rounds_out = 0;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t alive = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &alive, ctx)) return rc;
  if (sym->ne == 0) return GM_OK;
  if (int rc = ensure_local_buffers(g, true, decompose)) return rc;
  SubLaunches sub;
  gm_graph *run_on = nullptr;
  if (int rc = local_supports(g, &l2, sub, &run_on)) return rc;
  if (int rc = start_timer(ctx)) return rc;
  hipStream_t stream = ctx.stream;
  if (int rc = local_map(ctx, run_on, g->local.ent)) return rc;
  // (once per handle; filled on this call's stream, in front of its first reader: the header allows one call at a time per handle)
  if (int rc = g->lrev.ensure(g->mu, [&](RevIndex &ri) {
        HIP_TRY(ri.rev.alloc(sizeof(int) * (size_t)std::max<long long>(g->ne, 1)));
        HIP_TRY(launch_local_rev(g->nv, g->ne, g->d_rp, g->d_col, ri.rev, g->cu_count, stream));
        return kOnceBuilt;
      })) return rc;
  HIP_TRY(launch_local_peel_init(g->ne, g->lrev->rev, g->local.mark, g->cu_count, stream));
  LocalPeelParams pp;
  memset(&pp, 0, sizeof pp);
  pp.nv = g->nv; pp.ne = g->ne; pp.rp = g->d_rp; pp.col = g->d_col; pp.rev = g->lrev->rev;
  pp.sup = g->local.ent; pp.mark = g->local.mark; pp.front = g->local.front; pp.cnt = g->local.cnt;
  pp.truss = decompose ? g->local.truss : nullptr;
  long long k = decompose ? 3 : k_in, kmax = 0;
  int rounds = 0;
  for (;;) {
    unsigned word[2] = {0u, 0u};
    for (;;) {  // the rounds of level k: threshold k - 2
      pp.thr = (unsigned)(k - 2);
      pp.level = (unsigned)(k - 1);
      HIP_TRY(hipMemsetAsync(g->local.cnt, 0, 8, stream));
      HIP_TRY(launch_local_mark(pp, g->cu_count, stream));
      HIP_TRY(hipMemcpyAsync(word, g->local.cnt, sizeof word, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      ++rounds;
      if (word[0] == 0u) break;
      kmax = k - 1;
      HIP_TRY(launch_local_peel(pp, word[0], g->cu_count, stream));
    }
    if (!decompose || word[1] == 0u) break;  // (decompose: nothing is alive any more)
    // every alive edge has support >= m: the (m + 2)-truss still holds all of them, the first level that removes one is m + 3
    k = (long long)(0xFFFFFFFFu - word[1]) + 3;
  }
  HIP_TRY(hipMemsetAsync(g->d_counters, 0, 8, stream));  // (the mapping kernel's sum is not a result of these calls)
  HIP_TRY(launch_local_truss_out(pp, d_out, g->d_counters, g->cu_count, stream));
  if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, &alive, 1, s); })) return rc;
  if (n_edges) *n_edges = alive;
  if (k_max) *k_max = (int32_t)kmax;  // (the last level that removed an edge)
  if (rounds_out) *rounds_out = rounds;
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

extern "C" int gm_ktruss(const gm_graph *sym, int k, const gm_launch *la, uint32_t *d_entry_sup, uint64_t *n_edges, int32_t *rounds, gm_stats *st) {
  if (!sym || k < 2) return GM_ERR_INVALID;
  if (int rc = local_refusals(sym, la)) return rc;
  return run_truss(sym, false, k, la, d_entry_sup, n_edges, nullptr, rounds, st);
}

extern "C" int gm_truss_decompose(const gm_graph *sym, const gm_launch *la, uint32_t *d_entry_truss, int32_t *k_max, int32_t *rounds, gm_stats *st) {
  if (!sym || !d_entry_truss) return GM_ERR_INVALID;
  if (int rc = local_refusals(sym, la)) return rc;
  return run_truss(sym, true, 0, la, d_entry_truss, nullptr, k_max, rounds, st);
}

// ---- k-clique cores (gm_kcl_core.hip; DESIGN.md "k-clique cores") ------------------------------------------------------------------------
// gm_clique_kcore (decompose = false) and gm_clique_core_decompose: K_v from gm_clique_local on the same handle (k = 2: the row lengths),
// then whole-frontier rounds as run_truss runs them.  24 bytes come back per round: the cliques destroyed so far, the frontier's size and
// the smallest count that stays alive; the densities of the states are compared here.
static int run_clique_core(const gm_graph *sym, bool decompose, int k, uint64_t c_in, const gm_launch *la, uint64_t *d_cnt_out, uint64_t *d_core,
                           uint32_t *d_round, uint64_t *n_vertices, uint64_t *n_cliques, uint64_t *c_max, int32_t *rounds_out, gm_core_dense *dense,
                           gm_stats *st) {
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  if (n_vertices) *n_vertices = 0;
  if (n_cliques) *n_cliques = 0;
  if (c_max) *c_max = 0;
  if (rounds_out) *rounds_out = 0;
  if (dense) *dense = gm_core_dense{1, 0, 0};
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t unused = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  const size_t nvz = (size_t)std::max(g->nv, 1);
  const bool wide = k >= 3 && g->max_deg > kKclLocalLdsRow;  // (a frontier vertex of more than kKclLocalLdsRow survivors needs a row that long)
  const unsigned long long slot_words = kcl_local_scratch_words(g->max_deg);
  const size_t slot_bytes = sizeof(unsigned) * (size_t)slot_words;
  const int grid_wide = wide ? clamp_grid((long long)(kKclScratchBudget / slot_bytes), (long long)g->cu_count * 2) : 0;
  const size_t heavy_cap = (size_t)(g->ne / (kKclLocalLdsRow + 1)) + 1;
  {
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->local.core_cnt) HIP_TRY(g->local.core_cnt.alloc(sizeof(unsigned long long) * nvz));
    if (!g->local.core_mark) HIP_TRY(g->local.core_mark.alloc(nvz));
    if (!g->local.core_front) HIP_TRY(g->local.core_front.alloc(sizeof(int) * nvz));
    if (!g->local.core_words) HIP_TRY(g->local.core_words.alloc(64));
    if (k >= 3 && !g->local.core_heavy) HIP_TRY(g->local.core_heavy.alloc(sizeof(int) * heavy_cap));
    if (wide)  // (a slot that does not fit the device: the allocation fails and the call is refused)
      if (int rc = grow_dev(g->local.core_scratch, &g->local.core_scratch_bytes, slot_bytes * (size_t)grid_wide)) return rc;
  }
  SubLaunches sub;
  uint64_t total = (uint64_t)(sym->ne / 2);  // (k = 2: a clique is an edge)
  if (k >= 3)
    if (int rc = sub.run([&](gm_stats *s) { return gm_clique_local(sym, k, &l2, (uint64_t *)g->local.core_cnt.get(), nullptr, &total, s); })) return rc;
  if (int rc = start_timer(ctx)) return rc;
  hipStream_t stream = ctx.stream;
  KclCoreParams pp;
  memset(&pp, 0, sizeof pp);
  pp.nv = g->nv; pp.k = k; pp.max_deg = std::max(g->max_deg, 1); pp.rp = g->d_rp; pp.col = g->d_col;
  pp.cnt = g->local.core_cnt; pp.mark = g->local.core_mark; pp.front = g->local.core_front; pp.words = g->local.core_words;
  pp.core = decompose ? (unsigned long long *)d_core : nullptr;
  pp.round = decompose ? (unsigned *)d_round : nullptr;
  pp.heavy = g->local.core_heavy; pp.heavy_cap = (unsigned)heavy_cap;
  pp.scratch = g->local.core_scratch; pp.scratch_words = slot_words;
  unsigned long long h[3] = {0ull, 0ull, 0ull};  // [0] destroyed so far, [1] the frontier's size, [2] ~0 - the smallest count that stays (0: none)
  HIP_TRY(hipMemsetAsync(pp.words, 0, 64, stream));
  HIP_TRY(launch_core_init(pp, g->cu_count, stream));
  unsigned long long level = 0, cmax = 0;
  if (decompose) {  // the level the first round runs at: the smallest count of the graph
    HIP_TRY(hipMemcpyAsync(&h[2], pp.words + CW_LEAST, sizeof h[2], hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    level = h[2] ? ~0ull - h[2] : 0ull;
  }
  int rounds = 0;
  uint64_t removed = 0;
  gm_core_dense best{1, 0, 0};
  for (;;) {
    pp.thr = decompose ? level + 1 : (unsigned long long)c_in;
    pp.level = level;
    pp.round_no = (unsigned)(rounds + 1);
    HIP_TRY(hipMemsetAsync(pp.words + CW_FRONT, 0, 32, stream));  // (the frontier's size, the smallest count, the three queue words)
    HIP_TRY(launch_core_mark(pp, g->cu_count, stream));
    HIP_TRY(hipMemcpyAsync(h, pp.words + CW_DESTROYED, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ++rounds;
    if (h[0] > total || h[1] > (uint64_t)g->nv - removed) {
      g_last_error = "gm_clique_core: a round's counters left their range (internal error)";
      return GM_ERR_INVALID;
    }
    const uint64_t vertices = (uint64_t)g->nv - removed, cliques = total - h[0];  // the state at the start of this round
    if (vertices > 0 && (best.vertices == 0 || (unsigned __int128)cliques * best.vertices > (unsigned __int128)best.cliques * vertices))
      best = gm_core_dense{(int32_t)rounds, vertices, cliques};
    if (h[1] == 0ull) {
      if (!decompose || h[2] == 0ull) break;  // (decompose: nothing is alive any more)
      level = ~0ull - h[2];                   // every alive vertex has a count >= this: the first level that removes one
      continue;
    }
    removed += h[1];
    cmax = level;
    HIP_TRY(launch_core_peel(pp, (unsigned)h[1], g->cu_count, stream));
    if (wide) HIP_TRY(launch_core_peel_wide(pp, grid_wide, stream));
  }
  HIP_TRY(launch_core_out(pp, decompose ? nullptr : (unsigned long long *)d_cnt_out, g->cu_count, stream));
  unsigned long long w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(w, pp.words, sizeof w, hipMemcpyDeviceToHost, stream));
  if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, &unused, 1, s); })) return rc;  // (synchronises the stream)
  const uint64_t left = total - w[CW_DESTROYED];
  if (w[CW_ERR] != 0 || w[CW_DESTROYED] > total || w[CW_SUM] != left * (uint64_t)k || w[CW_ALIVE] != (uint64_t)g->nv - removed) {
    g_last_error = "gm_clique_core: " + std::to_string(w[CW_ERR]) + " kernel errors, " + std::to_string(left) + " cliques left against the counts' sum " +
                   std::to_string(w[CW_SUM]) + " / k (internal error)";
    return GM_ERR_INVALID;
  }
  if (n_vertices) *n_vertices = w[CW_ALIVE];
  if (n_cliques) *n_cliques = left;
  if (c_max) *c_max = cmax;
  if (rounds_out) *rounds_out = rounds;
  if (dense) *dense = best;
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

static int clique_core_refusals(const gm_graph *sym, int k, const gm_launch *la, const char *who) {
  if (!sym || k < 2 || k > GM_MAX_CLIQUE_K) return GM_ERR_INVALID;
  if (int rc = local_refusals(sym, la)) return rc;
  if (k > 8) {
    g_last_error = std::string(who) + ": k = 9 .. " + std::to_string(GM_MAX_CLIQUE_K) + " is not supported yet (2 <= k <= 8)";
    return GM_ERR_UNSUPPORTED;
  }
  return GM_OK;
}

extern "C" int gm_clique_kcore(const gm_graph *sym, int k, uint64_t c, const gm_launch *la, uint64_t *d_vertex_cnt, uint64_t *n_vertices,
                               uint64_t *n_cliques, int32_t *rounds, gm_stats *st) {
  if (int rc = clique_core_refusals(sym, k, la, "gm_clique_kcore")) return rc;
  return run_clique_core(sym, false, k, c, la, d_vertex_cnt, nullptr, nullptr, n_vertices, n_cliques, nullptr, rounds, nullptr, st);
}

extern "C" int gm_clique_core_decompose(const gm_graph *sym, int k, const gm_launch *la, uint64_t *d_vertex_core, uint32_t *d_vertex_round,
                                        uint64_t *c_max, int32_t *rounds, gm_core_dense *dense, gm_stats *st) {
  if (!d_vertex_core) return GM_ERR_INVALID;
  if (int rc = clique_core_refusals(sym, k, la, "gm_clique_core_decompose")) return rc;
  return run_clique_core(sym, true, k, 0, la, nullptr, d_vertex_core, d_vertex_round, nullptr, nullptr, c_max, rounds, dense, st);
}

// ---- k-clique trusses (gm_kcl_truss.hip; DESIGN.md "k-clique trusses") -----------------------------------------------------------------------
// gm_clique_ktruss (decompose = false) and gm_clique_truss_decompose: K_e per entry from gm_clique_local on the same handle, then the rounds
// of run_clique_core with the canonical entries in place of the vertices.  24 bytes come back per round: the cliques destroyed so far, the
// frontier's size and the smallest count that stays alive.
static int run_clique_truss(const gm_graph *sym, bool decompose, int k, uint64_t c_in, const gm_launch *la, uint64_t *d_cnt_out, uint64_t *d_theta,
                            uint32_t *d_round, uint64_t *n_edges, uint64_t *n_cliques, uint64_t *c_max, int32_t *rounds_out, gm_stats *st) {
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  if (n_edges) *n_edges = 0;
  if (n_cliques) *n_cliques = 0;
  if (c_max) *c_max = 0;
  if (rounds_out) *rounds_out = 0;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t unused = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  if (sym->ne == 0) {
    if (rounds_out) *rounds_out = 1;  // (the round that finds the frontier empty)
    return GM_OK;
  }
  const size_t nez = (size_t)g->ne, edges = (size_t)(g->ne / 2);
  const bool wide = g->max_deg > kKclLocalLdsRow;  // (a frontier edge of more than kKclLocalLdsRow survivors needs two rows that long)
  const unsigned long long slot_words = kcl_local_scratch_words(g->max_deg);
  const size_t slot_bytes = sizeof(unsigned) * (size_t)slot_words;
  const int grid_wide = wide ? clamp_grid((long long)(kKclScratchBudget / slot_bytes), (long long)g->cu_count * 2) : 0;
  const size_t heavy_cap = wide ? edges + 1 : 1;
  {
    std::lock_guard<std::mutex> lk(g->mu);
    if (!g->local.ktr_cnt) HIP_TRY(g->local.ktr_cnt.alloc(sizeof(unsigned long long) * nez));
    if (!g->local.ktr_mark) HIP_TRY(g->local.ktr_mark.alloc(nez));
    if (!g->local.ktr_front) HIP_TRY(g->local.ktr_front.alloc(sizeof(int) * (edges + 1)));
    if (!g->local.ktr_words) HIP_TRY(g->local.ktr_words.alloc(64));
    if (!g->local.ktr_heavy) HIP_TRY(g->local.ktr_heavy.alloc(sizeof(int) * heavy_cap));
    if (wide)  // (a slot that does not fit the device: the allocation fails and the call is refused)
      if (int rc = grow_dev(g->local.ktr_scratch, &g->local.ktr_scratch_bytes, slot_bytes * (size_t)grid_wide)) return rc;
  }
  SubLaunches sub;
  uint64_t total = 0;
  if (int rc = sub.run([&](gm_stats *s) { return gm_clique_local(sym, k, &l2, nullptr, (uint64_t *)g->local.ktr_cnt.get(), &total, s); })) return rc;
  if (int rc = start_timer(ctx)) return rc;
  hipStream_t stream = ctx.stream;
  // (once per handle, shared with the k-truss; filled on this call's stream, in front of its first reader)
  if (int rc = g->lrev.ensure(g->mu, [&](RevIndex &ri) {
        HIP_TRY(ri.rev.alloc(sizeof(int) * (size_t)std::max<long long>(g->ne, 1)));
        HIP_TRY(launch_local_rev(g->nv, g->ne, g->d_rp, g->d_col, ri.rev, g->cu_count, stream));
        return kOnceBuilt;
      })) return rc;
  KclTrussParams pp;
  memset(&pp, 0, sizeof pp);
  pp.nv = g->nv; pp.k = k; pp.max_deg = std::max(g->max_deg, 1); pp.ne = g->ne; pp.rp = g->d_rp; pp.col = g->d_col; pp.rev = g->lrev->rev;
  pp.cnt = g->local.ktr_cnt; pp.mark = g->local.ktr_mark; pp.front = g->local.ktr_front; pp.words = g->local.ktr_words;
  pp.theta = decompose ? (unsigned long long *)d_theta : nullptr;
  pp.round = decompose ? (unsigned *)d_round : nullptr;
  pp.heavy = g->local.ktr_heavy; pp.heavy_cap = (unsigned)heavy_cap;
  pp.scratch = g->local.ktr_scratch; pp.scratch_words = slot_words;
  unsigned long long h[3] = {0ull, 0ull, 0ull};  // [0] destroyed so far, [1] the frontier's size, [2] ~0 - the smallest count that stays (0: none)
  HIP_TRY(hipMemsetAsync(pp.words, 0, 64, stream));
  HIP_TRY(launch_ktr_init(pp, g->cu_count, stream));
  unsigned long long level = 0, cmax = 0;
  if (decompose) {  // the level the first round runs at: the smallest count of the graph
    HIP_TRY(hipMemcpyAsync(&h[2], pp.words + CW_LEAST, sizeof h[2], hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    level = h[2] ? ~0ull - h[2] : 0ull;
  }
  int rounds = 0;
  uint64_t removed = 0;
  for (;;) {
    pp.thr = decompose ? level + 1 : (unsigned long long)c_in;
    pp.level = level;
    pp.round_no = (unsigned)(rounds + 1);
    HIP_TRY(hipMemsetAsync(pp.words + CW_FRONT, 0, 32, stream));  // (the frontier's size, the smallest count, the three queue words)
    HIP_TRY(launch_ktr_mark(pp, g->cu_count, stream));
    HIP_TRY(hipMemcpyAsync(h, pp.words + CW_DESTROYED, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ++rounds;
    if (h[0] > total || h[1] > (uint64_t)edges - removed) {
      g_last_error = "gm_clique_truss: a round's counters left their range (internal error)";
      return GM_ERR_INVALID;
    }
    if (h[1] == 0ull) {
      if (!decompose || h[2] == 0ull) break;  // (decompose: nothing is alive any more)
      level = ~0ull - h[2];                   // every alive edge has a count >= this: the first level that removes one
      continue;
    }
    removed += h[1];
    cmax = level;
    HIP_TRY(launch_ktr_peel(pp, (unsigned)h[1], g->cu_count, stream));
    if (wide) HIP_TRY(launch_ktr_peel_wide(pp, grid_wide, stream));
  }
  HIP_TRY(launch_ktr_out(pp, decompose ? nullptr : (unsigned long long *)d_cnt_out, g->cu_count, stream));
  unsigned long long w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(w, pp.words, sizeof w, hipMemcpyDeviceToHost, stream));
  if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, &unused, 1, s); })) return rc;  // (synchronises the stream)
  const uint64_t left = total - w[CW_DESTROYED], per_clique = (uint64_t)(k * (k - 1) / 2);
  const bool sums_ok = decompose ? left == 0 : w[CW_SUM] == left * per_clique && w[CW_ALIVE] <= (uint64_t)edges - removed;  // (the decomposition destroys all)
  if (w[CW_ERR] != 0 || w[CW_DESTROYED] > total || !sums_ok) {
    g_last_error = "gm_clique_truss: " + std::to_string(w[CW_ERR]) + " kernel errors, " + std::to_string(left) + " cliques left against the counts' sum " +
                   std::to_string(w[CW_SUM]) + " / C(k, 2) (internal error)";
    return GM_ERR_INVALID;
  }
  if (n_edges) *n_edges = w[CW_ALIVE];
  if (n_cliques) *n_cliques = left;
  if (c_max) *c_max = cmax;
  if (rounds_out) *rounds_out = rounds;
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

static int clique_truss_refusals(const gm_graph *sym, int k, const gm_launch *la, const char *who) {
  if (!sym || k < 3 || k > GM_MAX_CLIQUE_K) return GM_ERR_INVALID;
  if (int rc = local_refusals(sym, la)) return rc;
  if (k > 8) {
    g_last_error = std::string(who) + ": k = 9 .. " + std::to_string(GM_MAX_CLIQUE_K) + " is not supported yet (3 <= k <= 8)";
    return GM_ERR_UNSUPPORTED;
  }
  if (sym->d_symdeg) {  // (an oriented copy has no reverse entries: every edge state sits at the smaller of an entry and its reverse)
    g_last_error = std::string(who) + ": needs the symmetric graph, not its oriented copy";
    return GM_ERR_INVALID;
  }
  return GM_OK;
}

extern "C" int gm_clique_ktruss(const gm_graph *sym, int k, uint64_t c, const gm_launch *la, uint64_t *d_entry_cnt, uint64_t *n_edges,
                                uint64_t *n_cliques, int32_t *rounds, gm_stats *st) {
  if (int rc = clique_truss_refusals(sym, k, la, "gm_clique_ktruss")) return rc;
  return run_clique_truss(sym, false, k, c, la, d_entry_cnt, nullptr, nullptr, n_edges, n_cliques, nullptr, rounds, st);
}

extern "C" int gm_clique_truss_decompose(const gm_graph *sym, int k, const gm_launch *la, uint64_t *d_entry_theta, uint32_t *d_entry_round,
                                         uint64_t *c_max, int32_t *rounds, gm_stats *st) {
  if (!d_entry_theta) return GM_ERR_INVALID;
  if (int rc = clique_truss_refusals(sym, k, la, "gm_clique_truss_decompose")) return rc;
  return run_clique_truss(sym, true, k, 0, la, nullptr, d_entry_theta, d_entry_round, nullptr, nullptr, c_max, rounds, st);
}

// ---- triangle listing (gm_list.hip; DESIGN.md "Triangle listing") -----------------------------------------------------------------------
// On the oriented copy as numbered: it keeps the caller's ids, so a match is written as it is found.  The count stage runs once per handle
// (the batches' first slots stay on the SYMMETRIC handle); a window is one fill launch that walks only the batches it meets.
extern "C" int gm_tc_list(const gm_graph *sym, const gm_launch *la, uint64_t first, uint64_t cap, int32_t *d_tri, uint64_t *total,
                          uint64_t *n_written, gm_stats *st) {
  if (total) *total = 0;
  if (n_written) *n_written = 0;
  if (int rc = local_refusals(sym, la)) return rc;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t unused = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  if (sym->ne == 0) return GM_OK;
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  const gm_graph *dag = g->dag_cache;
  if (int rc = reject_big(dag)) return rc;
  ListParams lp;
  memset(&lp, 0, sizeof lp);
  lp.nv = dag->nv; lp.ne = dag->ne; lp.rp = dag->d_rp; lp.col = dag->d_col;
  if (int rc = start_timer(ctx)) return rc;
  if (int rc = g->list_off.ensure(g->mu, [&](ListOffsets &lo) {  // (once per handle)
        if (dag->ne > 0) {
          const size_t nb = (size_t)((dag->ne + GM_WAVE - 1) / GM_WAVE);
          HIP_TRY(lo.off.alloc(sizeof(unsigned long long) * (nb + 1)));
          lp.off = lo.off;
          HIP_TRY(list_count_scan(lp, g->cu_count, ctx.stream));
          HIP_TRY(hipMemcpyAsync(&lo.total, lo.off + nb, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx.stream));
          HIP_TRY(hipStreamSynchronize(ctx.stream));
        }
        return kOnceBuilt;
      })) return rc;
  const uint64_t T = g->list_off->total;
  const uint64_t nw = (d_tri && first < T) ? std::min<uint64_t>(cap, T - first) : 0;
  if (nw > 0) {
    lp.off = g->list_off->off; lp.first = first; lp.nw = nw; lp.tri = d_tri;
    HIP_TRY(launch_list_fill(lp, g->cu_count, ctx.stream));
  }
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_COPY, 0, &unused, 1, &s)) return rc;
  if (total) *total = T;
  if (n_written) *n_written = nw;
  if (st) st->kernel_ms = s.kernel_ms;
  return GM_OK;
}

// ---- k-clique listing (gm_clique_list.hip; DESIGN.md "k-clique listing") -----------------------------------------------------------------
// On the oriented copy as numbered, for gm_tc_list's reason: it keeps the caller's ids, so a row is written as it is found.  The count
// stage runs once per (handle, k) -- every entry's first slot stays on the SYMMETRIC handle -- and a window is one fill launch (two when a
// row is longer than the LDS matrix) that walks only the roots, entries and pairs it meets.
extern "C" int gm_clique_list(const gm_graph *sym, int k, const gm_launch *la, uint64_t first, uint64_t cap, int32_t *d_cliques, uint64_t *total,
                              uint64_t *n_written, gm_stats *st) {
  if (total) *total = 0;
  if (n_written) *n_written = 0;
  if (!sym || k < 3 || k > GM_MAX_CLIQUE_K) return GM_ERR_INVALID;
  if (int rc = local_refusals(sym, la)) return rc;
  if (k > 8) {
    g_last_error = "gm_clique_list: k = 9 .. " + std::to_string(GM_MAX_CLIQUE_K) + " is not supported yet (3 <= k <= 8)";
    return GM_ERR_UNSUPPORTED;
  }
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t unused = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  if (sym->ne == 0) return GM_OK;
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  const gm_graph *dag = g->dag_cache;
  if (int rc = reject_big(dag)) return rc;
  const bool wide = dag->max_deg > kKclLocalLdsRow;
  const unsigned long long slot_words = kcl_local_scratch_words(dag->max_deg);
  const size_t slot_bytes = sizeof(unsigned) * (size_t)slot_words;
  const int grid = grid_for(((long long)dag->nv + 7) / 8, g->cu_count, 3);
  const int grid_wide = wide ? clamp_grid((long long)(kKclScratchBudget / slot_bytes), (long long)g->cu_count * 2) : 0;
  if (wide) {  // (a slot that does not fit the device: the allocation fails and the call is refused)
    std::lock_guard<std::mutex> lk(g->mu);
    if (int rc = grow_dev(g->local.kcl_list_scratch, &g->local.kcl_list_scratch_bytes, slot_bytes * (size_t)grid_wide)) return rc;
  }
  KclListParams kp;
  memset(&kp, 0, sizeof kp);
  kp.nv = dag->nv; kp.ne = dag->ne; kp.k = k; kp.max_deg = std::max(dag->max_deg, 1);
  kp.rp = dag->d_rp; kp.col = dag->d_col;
  kp.queue = queue_word(g, QW_MAIN); kp.queue_wide = queue_word(g, QW_CLASS1);
  kp.scratch = g->local.kcl_list_scratch; kp.scratch_words = slot_words;
  HIP_TRY(hipMemsetAsync(g->d_counters, 0, kCounterBlockBytes, ctx.stream));  // (a first call oriented the graph since begin_launch)
  if (int rc = start_timer(ctx)) return rc;
  Once<CliqueListOffsets> &state = g->clique_list_off[k - 3];
  if (int rc = state.ensure(g->mu, [&](CliqueListOffsets &lo) {  // (once per handle and k)
        if (dag->ne > 0) {
          const size_t ne = (size_t)dag->ne;
          HIP_TRY(lo.off.alloc(sizeof(unsigned long long) * (ne + 1)));
          HIP_TRY(kcl_list_count_scan(kp, lo.off, grid, grid_wide, ctx.stream));
          HIP_TRY(hipMemcpyAsync(&lo.total, lo.off + ne, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx.stream));
          HIP_TRY(hipMemsetAsync(g->d_counters, 0, kCounterBlockBytes, ctx.stream));  // (the fill dequeues from the same words)
          HIP_TRY(hipStreamSynchronize(ctx.stream));
        }
        return kOnceBuilt;
      })) return rc;
  const uint64_t T = state->total;
  const uint64_t nw = (d_cliques && first < T) ? std::min<uint64_t>(cap, T - first) : 0;
  if (nw > 0) {
    kp.off = state->off; kp.first = first; kp.nw = nw; kp.out = d_cliques;
    HIP_TRY(launch_kcl_list_fill(kp, grid, grid_wide, ctx.stream));
  }
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_COPY, 0, &unused, 1, &s)) return rc;
  if (total) *total = T;
  if (n_written) *n_written = nw;
  if (st) {
    st->kernel_ms = s.kernel_ms;
    st->grid = (uint32_t)grid;
  }
  return GM_OK;
}

// ---- triangle nuclei (gm_nucleus34.hip; DESIGN.md "Triangle nuclei") -------------------------------------------------------------------------
// gm_tri_clique4_local (mode NUC_LOCAL), gm_nucleus34 (NUC_FIXED) and gm_nucleus34_decompose (NUC_DECOMPOSE): the triangle index of the
// oriented copy (once per handle, kept on the SYMMETRIC handle), K4(t) of every triangle, then run_clique_truss's rounds with the triangle
// ids in place of the canonical entries.  24 bytes come back per round: the cliques destroyed so far, the frontier's size and the smallest
// count that stays alive.
enum NucMode : int { NUC_LOCAL = 0, NUC_FIXED = 1, NUC_DECOMPOSE = 2 };
static int run_nucleus34(const gm_graph *sym, NucMode mode, uint32_t c_in, const gm_launch *la, uint64_t n_tri, uint32_t *d_out, uint32_t *d_round,
                         uint64_t *n_triangles, uint64_t *n_cliques, uint32_t *c_max, int32_t *rounds_out, gm_stats *st, const char *who) {
  if (n_triangles) *n_triangles = 0;
  if (n_cliques) *n_cliques = 0;
  if (c_max) *c_max = 0;
  if (rounds_out) *rounds_out = 0;
  if (int rc = local_refusals(sym, la)) return rc;
  if (sym->d_symdeg) {  // (the common neighbours of a triangle's corners are read off the symmetric rows)
    g_last_error = std::string(who) + ": needs the symmetric graph, not its oriented copy";
    return GM_ERR_INVALID;
  }
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  fill_stats(st, 0, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t unused = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &unused, ctx)) return rc;  // (selects the device; refuses unsorted rows)
  const auto wrong_length = [&](uint64_t T) {
    g_last_error = std::string(who) + ": n_tri = " + std::to_string(n_tri) + ", the graph has " + std::to_string(T) + " triangles (the total of gm_tc_list)";
    return GM_ERR_INVALID;
  };
  if (sym->ne == 0) {
    if (n_tri != 0) return wrong_length(0);
    if (rounds_out && mode != NUC_LOCAL) *rounds_out = 1;  // (the round that finds the frontier empty)
    return GM_OK;
  }
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  const gm_graph *dag = g->dag_cache;
  if (int rc = reject_big(dag)) return rc;
  if (int rc = start_timer(ctx)) return rc;
  hipStream_t stream = ctx.stream;
  if (int rc = g->tri_index.ensure(g->mu, [&](TriIndex &ti) -> int {  // (once per handle: built into a local value, moved in whole)
        const size_t dne = (size_t)dag->ne;
        HIP_TRY(ti.off.alloc(sizeof(unsigned long long) * (dne + 1)));
        HIP_TRY(hipMemsetAsync(ti.off, 0, sizeof(unsigned long long) * (dne + 1), stream));
        if (dne == 0) return kOnceBuilt;
        NucIndexParams ip;
        memset(&ip, 0, sizeof ip);
        ip.nv = dag->nv; ip.ne = dag->ne; ip.rp = dag->d_rp; ip.col = dag->d_col;
        {
          DevBuf<unsigned long long> cnt;
          HIP_TRY(cnt.alloc(dne + 1));
          HIP_TRY(hipMemsetAsync(cnt.p + dne, 0, sizeof(unsigned long long), stream));
          ip.cnt = cnt.p;
          HIP_TRY(launch_nuc_index(ip, false, g->cu_count, stream));
          HIP_TRY(nuc_index_scan(cnt.p, ti.off, dne + 1, stream));  // (synchronises the stream)
        }
        HIP_TRY(hipMemcpy(&ti.total, ti.off + dne, sizeof ti.total, hipMemcpyDeviceToHost));
        if (ti.total >= 0xFFFFFFFFull) {
          g_last_error = std::string(who) + ": " + std::to_string(ti.total) + " triangles (>= 2^32 - 1: beyond the 32-bit triangle ids)";
          return GM_ERR_TOO_LARGE;
        }
        const size_t tz = (size_t)std::max<unsigned long long>(ti.total, 1);
        HIP_TRY(ti.w.alloc(sizeof(int) * tz));
        HIP_TRY(ti.e.alloc(sizeof(int) * tz));
        ip.off = ti.off; ip.tri_w = ti.w; ip.tri_e = ti.e;
        if (ti.total > 0) HIP_TRY(launch_nuc_index(ip, true, g->cu_count, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return kOnceBuilt;
      })) return rc;
  const uint64_t T = g->tri_index->total;
  if (n_tri != T) return wrong_length(T);
  if (st) st->tasks = T;
  if (int rc = g->nuc34.ensure(g->mu, [&](Nucleus34State &ns) {
        const size_t tz = (size_t)std::max<uint64_t>(T, 1);
        HIP_TRY(ns.cnt.alloc(sizeof(unsigned) * tz));
        HIP_TRY(ns.mark.alloc(tz));
        HIP_TRY(ns.front.alloc(sizeof(unsigned) * tz));
        HIP_TRY(ns.words.alloc(64));
        return kOnceBuilt;
      })) return rc;
  const bool decompose = mode == NUC_DECOMPOSE;
  Nuc34Params pp;
  memset(&pp, 0, sizeof pp);
  pp.nv = g->nv; pp.nt = T; pp.rp = g->d_rp; pp.col = g->d_col; pp.drp = dag->d_rp; pp.dcol = dag->d_col;
  pp.tri_off = g->tri_index->off; pp.tri_w = g->tri_index->w; pp.tri_e = g->tri_index->e;
  pp.cnt = g->nuc34->cnt; pp.mark = mode == NUC_LOCAL ? nullptr : g->nuc34->mark.get(); pp.front = g->nuc34->front; pp.words = g->nuc34->words;
  pp.theta = decompose ? (unsigned *)d_out : nullptr;
  pp.round = decompose ? (unsigned *)d_round : nullptr;
  unsigned long long w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemsetAsync(pp.words, 0, 64, stream));
  HIP_TRY(launch_nuc_count(pp, mode == NUC_LOCAL && d_out ? (unsigned *)d_out : pp.cnt, g->cu_count, stream));
  HIP_TRY(hipMemcpyAsync(w, pp.words, sizeof w, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (w[NW_TOTAL] % 4ull != 0ull) {
    g_last_error = std::string(who) + ": the sum of K4(t), " + std::to_string(w[NW_TOTAL]) + ", is not a multiple of 4 (internal error)";
    return GM_ERR_INVALID;
  }
  const uint64_t total = w[NW_TOTAL] / 4ull;
  int rounds = 0;
  uint64_t removed = 0;
  unsigned cmax = 0;
  if (mode != NUC_LOCAL) {
    unsigned long long h[3] = {0ull, 0ull, 0ull};  // [0] destroyed so far, [1] the frontier's size, [2] ~0 - the smallest count that stays (0: none)
    unsigned level = decompose && w[CW_LEAST] ? (unsigned)(~0ull - w[CW_LEAST]) : 0u;  // the level the first round runs at: the smallest count
    for (;;) {
      pp.thr = decompose ? level + 1u : c_in;
      pp.level = level;
      pp.round_no = (unsigned)(rounds + 1);
      HIP_TRY(hipMemsetAsync(pp.words + CW_FRONT, 0, 16, stream));  // (the frontier's size, the smallest count)
      HIP_TRY(launch_nuc_mark(pp, g->cu_count, stream));
      HIP_TRY(hipMemcpyAsync(h, pp.words + CW_DESTROYED, sizeof h, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      ++rounds;
      if (h[0] > total || h[1] > T - removed) {
        g_last_error = std::string(who) + ": a round's counters left their range (internal error)";
        return GM_ERR_INVALID;
      }
      if (h[1] == 0ull) {
        if (!decompose || h[2] == 0ull) break;  // (decompose: nothing is alive any more)
        level = (unsigned)(~0ull - h[2]);       // every alive triangle has a count >= this: the first level that removes one
        continue;
      }
      removed += h[1];
      cmax = level;
      HIP_TRY(launch_nuc_peel(pp, (unsigned)h[1], g->cu_count, stream));
    }
    HIP_TRY(launch_nuc_out(pp, decompose ? nullptr : (unsigned *)d_out, g->cu_count, stream));
    HIP_TRY(hipMemcpyAsync(w, pp.words, sizeof w, hipMemcpyDeviceToHost, stream));
  }
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_COPY, 0, &unused, 1, &s)) return rc;  // (synchronises the stream)
  if (st) st->kernel_ms = s.kernel_ms;
  if (mode == NUC_LOCAL) {
    if (n_cliques) *n_cliques = total;
    return GM_OK;
  }
  const uint64_t left = total - w[CW_DESTROYED];
  const bool sums_ok = decompose ? left == 0 && removed == T : w[CW_SUM] == 4ull * left && w[CW_ALIVE] == T - removed;  // (the decomposition destroys all)
  if (w[CW_ERR] != 0 || w[CW_DESTROYED] > total || !sums_ok) {
    g_last_error = std::string(who) + ": " + std::to_string(w[CW_ERR]) + " kernel errors, " + std::to_string(left) +
                   " cliques left against the counts' sum " + std::to_string(w[CW_SUM]) + " / 4 (internal error)";
    return GM_ERR_INVALID;
  }
  if (n_triangles) *n_triangles = w[CW_ALIVE];
  if (n_cliques) *n_cliques = left;
  if (c_max) *c_max = cmax;
  if (rounds_out) *rounds_out = rounds;
  return GM_OK;
}

extern "C" int gm_tri_clique4_local(const gm_graph *sym, const gm_launch *la, uint64_t n_tri, uint32_t *d_tri_cnt, uint64_t *total_k4, gm_stats *st) {
  if (total_k4) *total_k4 = 0;
  return run_nucleus34(sym, NUC_LOCAL, 0, la, n_tri, d_tri_cnt, nullptr, nullptr, total_k4, nullptr, nullptr, st, "gm_tri_clique4_local");
}

extern "C" int gm_nucleus34(const gm_graph *sym, uint32_t c, const gm_launch *la, uint64_t n_tri, uint32_t *d_tri_cnt, uint64_t *n_triangles,
                            uint64_t *n_cliques, int32_t *rounds, gm_stats *st) {
  return run_nucleus34(sym, NUC_FIXED, c, la, n_tri, d_tri_cnt, nullptr, n_triangles, n_cliques, nullptr, rounds, st, "gm_nucleus34");
}

extern "C" int gm_nucleus34_decompose(const gm_graph *sym, const gm_launch *la, uint64_t n_tri, uint32_t *d_tri_theta, uint32_t *d_tri_round,
                                      uint32_t *c_max, int32_t *rounds, gm_stats *st) {
  if (!d_tri_theta) return GM_ERR_INVALID;
  return run_nucleus34(sym, NUC_DECOMPOSE, 0, la, n_tri, d_tri_theta, d_tri_round, nullptr, nullptr, c_max, rounds, st, "gm_nucleus34_decompose");
}
