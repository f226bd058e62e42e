// gm_solve_sgl.hip -- the SgL family over the launch layer (gm_launch.h): gm_sgl; rectangle / house / pentagon by wedge accumulation with their plans;
// the diamond through the edge supports (gm_diamond_support_*); the closed forms gm_sgl4_* / gm_sgl5_* / gm_sgl6_*.  Host code only: no kernel is defined
// here, so the unit has no code object and no warm-up.  Reference launch logic: src/sgl/gpu_base.cu:37-75.
#include "gm_launch.h"

// a host vector as a fresh device array (of at least one element)
template <class T>
static int upload(DevOwn<T> &d, const std::vector<T> &h) {
  HIP_TRY(d.alloc(sizeof(T) * std::max<size_t>(h.size(), 1)));
  if (!h.empty()) HIP_TRY(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  return GM_OK;
}
// the 2-path estimates of every centre on the host (launch: the kernel that writes them, `parts` arrays of nv)
template <class Launch>
static int centre_estimates(size_t nv, int parts, Launch launch, const char *what, std::vector<unsigned long long> &est) {
  DevOwn<unsigned long long> d_work;
  HIP_TRY(d_work.alloc(sizeof(unsigned long long) * parts * std::max<size_t>(nv, 1)));
  est.assign(parts * std::max<size_t>(nv, 1), 0);
  hipError_t e = nv ? launch(d_work) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpy(est.data(), d_work, sizeof(unsigned long long) * parts * nv, hipMemcpyDeviceToHost);
  return e == hipSuccess ? GM_OK : hip_fail(e, what, __FILE__, __LINE__);
}
// Every centre with work, by its 2-path estimate (work_launch: the kernel that writes it per centre), as one task list on the device, once
// per graph (the form with every end in the global maps): heavy first, then light by 4
template <class WorkLaunch>
static int build_centre_tasks(gm_graph *g, WorkLaunch work_launch, const char *what, Once<CentreTaskList> &list) {
  return list.ensure(g->mu, [&](CentreTaskList &out) {
    OtherSetupScope scope(g);
    const size_t nv = (size_t)g->nv;
    std::vector<unsigned long long> work;
    if (int rc = centre_estimates(nv, 1, work_launch, what, work)) return rc;
    std::vector<int> vs;
    vs.reserve(nv);
    for (size_t v = 0; v < nv; ++v)
      if (work[v] > 0) vs.push_back((int)v);
    std::stable_sort(vs.begin(), vs.end(), [&](int a, int b) { return work[(size_t)a] > work[(size_t)b]; });
    std::vector<int4> tasks;
    emit_centre_tasks(vs, work.data(), kHeavyCentre, tasks);
    if (int rc = upload(out.tasks, tasks)) return rc;
    out.n = tasks.size();
    return kOnceBuilt;
  });
}

// rectangle, flattened over wedges (rect_flat_kernel in gm_mine.hip)
int ensure_idx0(gm_graph *g, const GraphView &gv) {
  return g->rect_idx.ensure(g->mu, [&](RectIdx &ri) {
    OtherSetupScope scope(g);
    HIP_TRY(ri.idx0.alloc(sizeof(int) * (size_t)std::max(g->nv, 1)));
    HIP_TRY(launch_idx0(gv, ri.idx0, 0));
    return kOnceBuilt;
  });
}

int run_rect_flat(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st, bool pentagon) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  const GraphView gv = graph_view(g);
  rc = ensure_idx0(g, gv);  // (takes the lock itself)
  if (rc) return rc;
  rc = g->wedge_blocks.ensure(g->mu, [&](WedgeBlocks &wb) {  // once per graph: idx0[v] on the device, wedge-block prefix on the host
    OtherSetupScope scope(g);
    std::vector<int> idx0((size_t)std::max(g->nv, 1));
    HIP_TRY(hipMemcpy(idx0.data(), g->rect_idx->idx0, sizeof(int) * (size_t)g->nv, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> pre((size_t)g->nv + 1);
    unsigned long long acc = 0;
    for (int v = 0; v < g->nv; ++v) {
      pre[v] = acc;
      const unsigned long long n = (unsigned long long)idx0[v];
      acc += (n * (n - (n ? 1ull : 0ull)) / 2ull + 63ull) / 64ull;
    }
    pre[g->nv] = acc;
    wb.n = acc;
    HIP_TRY(wb.prefix.alloc(sizeof(unsigned long long) * ((size_t)g->nv + 1)));
    HIP_TRY(hipMemcpy(wb.prefix, pre.data(), sizeof(unsigned long long) * ((size_t)g->nv + 1), hipMemcpyHostToDevice));
    return kOnceBuilt;
  });
  if (rc) return rc;
  RectParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.idx0 = g->rect_idx->idx0;
  p.block_prefix = g->wedge_blocks->prefix;
  p.nblocks = g->wedge_blocks->n;
  p.group = la->chunk > 0 ? la->chunk : (pentagon ? 2 : 16);
  const long long ngroups = (long long)((p.nblocks + (unsigned long long)p.group - 1) / (unsigned long long)p.group);
  const int64_t count = take_range(ctx, ngroups, p);
  p.counters = g->d_counters;
  p.queue = queue_word64(g, QW64_MAIN);
  const int grid = grid_for((count + 3) / 4, g->cu_count, 8);
  if (int rc_t = start_timer(ctx)) return rc_t;
  if (count > 0) HIP_TRY(launch_rect_flat(p, pentagon, grid, ctx.stream));
  fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)count, grid, 256);
  return end_launch(ctx, FIN_COPY, 0, h_out, 1, st);
}

static int ensure_edge_tables(gm_graph *g, const GraphView &gv);

// A CentrePlan (the logic: gm_centre_plan.h) is built in locals -- a call that fails leaves the handle as it was.  Its last step: both task lists onto the device
static int upload_centre_tasks(const CentreTasks &t, CentrePlan &pl) {
  if (int rc = upload(pl.d_acc_tasks, t.acc_tasks)) return rc;
  if (int rc = upload(pl.d_lds_tasks, t.lds_tasks)) return rc;
  pl.n_acc_tasks = t.acc_tasks.size();
  pl.n_lds_tasks = t.lds_tasks.size();
  pl.n_cut = t.n_cut;
  for (const int2 &l : t.lds_tasks) ++(l.y >= 0 ? pl.n_lds_range : pl.n_lds_whole);
  for (size_t i = 0; i < t.acc_tasks.size(); ++i)
    if (t.acc_tasks[i].y == -2) {
      ++pl.n_acc_heavy;
      if (i < t.n_cut) ++pl.n_front_heavy;
    }
  return GM_OK;
}
static int max_lds_ranges(int limit) {
  const char *e = gm_opt("GM_RECT_LDS_RANGES");
  return e ? std::max(1, std::min(limit, std::atoi(e))) : limit;
}
// rectangle: the 2-path ends in the last ranges of ids (at most kRectLdsRanges) of the centres with >= GM_RECT_LDS_MIN 2-paths are counted in
// LDS maps (rect_lds_kernel): the ranges, the row bounds, the (centre, range) tasks, rect_acc_kernel's list with those centres in front
static int ensure_rect_plan(gm_graph *g, const GraphView &gv) {  // (after ensure_idx0)
  const int *d_idx0 = g->rect_idx->idx0;
  return g->rect_lds.ensure(g->mu, [&](RectLdsPlan &out) {
    OtherSetupScope scope(g);
    const size_t nv = (size_t)g->nv;
    unsigned long long lds_min = kMapLdsMinDefault;
    if (const char *e = gm_opt("GM_RECT_LDS_MIN")) lds_min = std::strtoull(e, nullptr, 10);
    const int nblk = (int)((nv + kRectLdsWords - 1) / kRectLdsWords);
    std::vector<int> bmax((size_t)std::max(nblk, 1), 0);
    if (nv) {
      DevOwn<int> d_bmax;
      HIP_TRY(d_bmax.alloc(sizeof(int) * (size_t)nblk));
      hipError_t e0 = hipMemset(d_bmax, 0, sizeof(int) * (size_t)nblk);
      if (e0 == hipSuccess) e0 = launch_rect_blockmax(gv, d_bmax, 0);
      if (e0 == hipSuccess) e0 = hipMemcpy(bmax.data(), d_bmax, sizeof(int) * (size_t)nblk, hipMemcpyDeviceToHost);
      if (e0 != hipSuccess) return hip_fail(e0, "rect_blockmax_kernel", __FILE__, __LINE__);
    }
    RectLdsRanges &rr = out.ranges = RectLdsRanges{};  // (whatever the numbering: tune[6] & GM_T6_AS_NUMBERED runs on the graph as given)
    rr.n = rect_lds_ranges((long long)g->nv, bmax, kRectLdsWords, max_lds_ranges(kRectLdsRanges), rr.rb, rr.lb);
    setup_trace("rect: ranges");
    CentrePlan &pl = out.plan;
    pl.cut = rr.rb[0];
    pl.bnd_stride = rr.n + 1;
    HIP_TRY(pl.d_bnd.alloc(sizeof(int) * (size_t)pl.bnd_stride * std::max<size_t>(nv, 1)));
    std::vector<unsigned long long> est;  // (both estimates: [0, nv) all ends, [nv, 2 nv) the ends below the cut)
    if (nv) HIP_TRY(launch_rect_bounds(gv, rr, pl.d_bnd, 0));
    if (int rc = centre_estimates(nv, 2, [&](unsigned long long *d_work) { return launch_rect_work_cut(gv, d_idx0, pl.d_bnd, pl.bnd_stride, d_work, 0); }, "rect_work_cut_kernel", est)) return rc;
    setup_trace("rect: bounds + work estimates");
    std::vector<int> idx0h(std::max<size_t>(nv, 1));
    if (nv) HIP_TRY(hipMemcpy(idx0h.data(), d_idx0, sizeof(int) * nv, hipMemcpyDeviceToHost));
    const CentreTasks tasks = plan_rect_tasks(nv, est.data(), est.data() + nv, idx0h.data(), rr.rb, rr.n, lds_min, kRectLdsWaves * GM_WAVE, kHeavyCentre);
    if (int rc = upload_centre_tasks(tasks, pl)) return rc;
    setup_trace("rect: task lists");
    return kOnceBuilt;
  });
}
// house: the same with ranges of kHouseLdsIds ids (at most kHouseLdsRanges) and plan_house_tasks' policy (GM_HOUSE_WALK_MIN: its 2-paths per walk)
static int ensure_house_plan(gm_graph *g, const GraphView &gv) {
  return g->house_lds.ensure(g->mu, [&](HouseLdsPlan &out) {
    OtherSetupScope scope(g);
    const size_t nv = (size_t)g->nv;
    const char *lds_min_given = gm_opt("GM_RECT_LDS_MIN");
    const unsigned long long lds_min = lds_min_given ? std::strtoull(lds_min_given, nullptr, 10) : kMapLdsMinDefault;
    HouseLdsRanges &rr = out.ranges = HouseLdsRanges{0, 0, g->nv};
    rr.n = house_lds_ranges((long long)g->nv, kHouseLdsIds, max_lds_ranges(kHouseLdsRanges), &rr.cut);
    CentrePlan &pl = out.plan;
    pl.cut = rr.cut;
    pl.bnd_stride = rr.n + 1;
    HIP_TRY(pl.d_bnd.alloc(sizeof(int) * (size_t)pl.bnd_stride * std::max<size_t>(nv, 1)));
    std::vector<unsigned long long> est;
    if (nv) HIP_TRY(launch_house_bounds(gv, rr, pl.d_bnd, 0));
    if (int rc = centre_estimates(nv, 2, [&](unsigned long long *d_work) { return launch_house_work_cut(gv, pl.d_bnd, pl.bnd_stride, d_work, 0); }, "house_work_cut_kernel", est)) return rc;
    std::vector<int> deg(nv + 1, 0);  // (the offsets, then their differences)
    if (nv) HIP_TRY(hipMemcpy(deg.data(), g->d_rp, sizeof(int) * (nv + 1), hipMemcpyDeviceToHost));
    for (size_t v = 0; v < nv; ++v) deg[v] = deg[v + 1] - deg[v];
    unsigned long long per_walk = kHouseWalkMinDefault;
    if (const char *e = gm_sweep_env("GM_HOUSE_WALK_MIN")) per_walk = std::strtoull(e, nullptr, 10);
    const CentreTasks tasks = plan_house_tasks(nv, est.data(), est.data() + nv, deg.data(), rr.n, lds_min, lds_min_given != nullptr, per_walk, kRectLdsWaves * GM_WAVE, kHeavyCentre);
    if (int rc = upload_centre_tasks(tasks, pl)) return rc;
    return kOnceBuilt;
  });
}
// what the acc / LDS kernel reads of the plan (the two patterns' parameter structs name these members alike); returns the LDS kernel's share of the tasks
template <class P>
static void acc_params_from_plan(P &p, const CentrePlan &pl) {
  p.tasks = pl.d_acc_tasks;
  p.n_cut = pl.n_cut;
  p.cut = pl.cut;
  p.bnd0 = pl.d_bnd;
  p.bnd_stride = pl.bnd_stride;
}
template <class P, class Ranges>
static int64_t lds_params_from_plan(P &lp, const LaunchCtx &ctx, const GraphView &gv, const CentrePlan &pl, const Ranges &r) {
  lp.g = gv;
  lp.tasks = pl.d_lds_tasks;
  lp.bnd = pl.d_bnd;
  lp.r = r;
  lp.queue = queue_word64(ctx.g, QW64_LDS);  // (its own dequeue word inside the zeroed 64-byte block)
  lp.counters = ctx.g->d_counters;
  return take_range(ctx, (int64_t)pl.n_lds_tasks, lp);
}
// The acc kernel's grid: one counter map (p.acc_stride = nv counters, rounded up to 64) per wave, wgs_per_cu workgroups per CU, within a budget of
// 1 / free_div of the free memory on top of the `held` bytes of the handle's maps, at most 32 GB (maps + touched lists); *need = the bytes of its maps
template <class P>
static int map_grid(const gm_graph *g, int64_t count, P &p, unsigned bytes_per_counter, unsigned free_div, int wgs_per_cu, size_t held, size_t *need) {
  p.acc_stride = ((unsigned long long)g->nv + 63ull) & ~63ull;
  const unsigned long long per_wg = p.acc_stride * bytes_per_counter * kWavesPerBlock;
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  const unsigned long long budget = std::min<unsigned long long>(32ull << 30, (unsigned long long)free_b / free_div + (unsigned long long)held);
  const int grid = clamp_grid(count, std::min<long long>((long long)g->cu_count * wgs_per_cu, (long long)std::max<unsigned long long>(1, budget / std::max<unsigned long long>(per_wg, 1))));
  *need = (size_t)per_wg * (size_t)grid;
  return grid;
}

// rectangle (rect_acc_kernel + rect_lds_kernel) and pentagon (pent_acc_kernel) by wedge accumulation: same centres, same counter maps.
// tune[6] & GM_T6_GLOBAL_MAPS, and the pentagon: every end in the global maps, round 5's form
int run_rect_acc(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st, bool pentagon) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  const GraphView gv = graph_view(g);
  rc = ensure_idx0(g, gv);
  if (rc) return rc;
  const bool lds_maps = !pentagon && !(la->tune[6] & GM_T6_GLOBAL_MAPS);
  if (!lds_maps) rc = build_centre_tasks(g, [&](unsigned long long *d_work) { return launch_rect_work(gv, g->rect_idx->idx0, d_work, 0); }, "rect_work_kernel", g->rect_tasks);
  if (rc) return rc;
  setup_trace("rect: idx0 / old tasks");
  if (lds_maps && (rc = ensure_rect_plan(g, gv))) return rc;
  RectAccParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.idx0 = g->rect_idx->idx0;
  p.tasks = g->rect_tasks->tasks;
  if (lds_maps) acc_params_from_plan(p, g->rect_lds->plan);
  const int64_t count = take_range(ctx, (int64_t)(lds_maps ? g->rect_lds->plan.n_acc_tasks : g->rect_tasks->n), p);
  p.counters = g->d_counters;
  p.queue = queue_word64(g, QW64_MAIN);
  // (with the heavy centres in LDS what is left for the global maps is light: 1 / 2 / 4 / 8 workgroups per CU measured 11.15 / 10.95 /
  // 11.1 / 11.0 ms for the rectangle of R-MAT-20 -- two, so that a first call does not allocate 2 x 32 GB of maps and lists)
  int acc_wgs_per_cu = lds_maps ? 2 : 8;
  if (const char *e = gm_sweep_env("GM_RECT_ACC_WGS")) acc_wgs_per_cu = std::max(1, std::atoi(e));
  size_t need = 0;
  const int grid = map_grid(g, count, p, 4, 4, acc_wgs_per_cu, g->maps.rect_acc_bytes, &need);
  if (need > g->maps.rect_acc_bytes) {
    if (int rc_a = grow_dev(g->maps.rect_acc, &g->maps.rect_acc_bytes, need)) return rc_a;
    HIP_TRY(hipMemset(g->maps.rect_acc, 0, need));  // every launch leaves the maps zeroed again
  }
  p.acc = g->maps.rect_acc;
  // touched-vertex lists: same shape as the maps (one int list of up to nv entries per wave)
  if (int rc_t = grow_dev(g->maps.pent_touched, &g->maps.pent_touched_bytes, need)) return rc_t;
  p.touched = g->maps.pent_touched;
  setup_trace("rect: global maps");
  if (pentagon) {
    rc = ensure_edge_tables(g, gv);
    if (rc) return rc;
    PentAccParams q;
    memset(&q, 0, sizeof q);
    q.g = gv;
    q.idx0 = g->rect_idx->idx0;
    q.tlt = g->house_tables->tlt;
    q.tasks = p.tasks;
    q.first = p.first;
    q.step = p.step;
    q.count = p.count;
    q.acc = p.acc;
    q.touched = g->maps.pent_touched;
    q.acc_stride = p.acc_stride;
    q.queue = p.queue;
    q.counters = p.counters;
    if (int rc_t = start_timer(ctx)) return rc_t;
    if (count > 0) HIP_TRY(launch_pent_acc(q, grid, ctx.stream));
    fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)count, grid, 256);
    return end_launch(ctx, FIN_HALF_SIGNED, 0, h_out, 1, st);
  }
  RectLdsParams lp{};
  lp.idx0 = g->rect_idx->idx0;
  const int64_t lcount = lds_maps ? lds_params_from_plan(lp, ctx, gv, g->rect_lds->plan, g->rect_lds->ranges) : 0;
  if (int rc_t = start_timer(ctx)) return rc_t;
  // (workgroups per CU: what its LDS -- the map + 1.5 KB of scratch per wave -- lets run together)
  const int lds_wgs = std::max(1, (int)((160 * 1024) / (kRectLdsWords * 4 + kRectLdsWaves * 1536 + 1024)));
  if (lcount > 0) HIP_TRY(launch_rect_lds(lp, (int)std::min<long long>((long long)g->cu_count * lds_wgs, (long long)lcount), ctx.stream));
  setup_trace("rect: lds kernel enqueued");
  if (count > 0) HIP_TRY(launch_rect_acc(p, grid, ctx.stream));
  setup_trace("rect: acc kernel enqueued");
  fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)(count + lcount), grid, 256);
  return end_launch(ctx, FIN_COPY, 0, h_out, 1, st);
}

// per-entry triangle tables t / tlt (edge_tab_kernel), once per graph; every rank builds the whole tables: they are inputs of
// every centre of the house / pentagon map kernels
static int ensure_edge_tables(gm_graph *g, const GraphView &gv) {
  return g->house_tables.ensure(g->mu, [&](HouseTables &ht) {
    OtherSetupScope scope(g);
    const size_t ne1 = (size_t)std::max<long long>(g->ne, 1);
    DevBuf<unsigned> t, tlt;
    HIP_TRY(t.alloc(ne1, true));  // (handed to the handle below)
    HIP_TRY(tlt.alloc(ne1, true));
    if (g->ne > 0) {
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemset(g->d_counters, 0, kCounterBlockBytes));
      HIP_TRY(launch_edge_tab(gv, t.p, tlt.p, queue_word64(g, QW64_MAIN), g->cu_count * 8, 0));
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemset(g->d_counters, 0, kCounterBlockBytes));  // (the table kernel used the dequeue head)
    }
    ht.t.take(t);  // (only after the build kernel has succeeded; the buffers free themselves on the error paths)
    ht.tlt.take(tlt);
    return kOnceBuilt;
  });
}

// house by wedge accumulation (edge_tab_kernel + house_acc_kernel + house_lds_kernel in gm_mine.hip); tune[6] & GM_T6_GLOBAL_MAPS: every end in
// the global maps, round 5's form
static int run_house_acc(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  const GraphView gv = graph_view(g);
  rc = ensure_edge_tables(g, gv);
  if (rc) return rc;
  const bool lds_maps = !(la->tune[6] & GM_T6_GLOBAL_MAPS);
  rc = lds_maps ? ensure_house_plan(g, gv) : build_centre_tasks(g, [&](unsigned long long *d_work) { return launch_house_work(gv, d_work, 0); }, "house_work_kernel", g->house_tasks);
  if (rc) return rc;
  HouseAccParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.t = g->house_tables->t;
  p.tlt = g->house_tables->tlt;
  p.tasks = g->house_tasks->tasks;
  if (lds_maps) acc_params_from_plan(p, g->house_lds->plan);
  const int64_t count = take_range(ctx, (int64_t)(lds_maps ? g->house_lds->plan.n_acc_tasks : g->house_tasks->n), p);
  p.counters = g->d_counters;
  p.queue = queue_word64(g, QW64_MAIN);
  size_t need = 0;
  const int grid = map_grid(g, count, p, 8, 3, lds_maps ? 4 : 8, g->maps.house_acc_bytes, &need);
  if (need > g->maps.house_acc_bytes) {
    g->maps.house_acc_bytes = 0;
    HIP_TRY(g->maps.house_acc.alloc(need));
    HIP_TRY(hipMemset(g->maps.house_acc, 0, need));  // every launch leaves the maps zeroed again
    HIP_TRY(g->maps.house_touched.alloc(need / 2));  // one int list per map
    g->maps.house_acc_bytes = need;
  }
  p.acc = g->maps.house_acc;
  p.touched = g->maps.house_touched;
  HouseLdsParams lp{};
  lp.t = g->house_tables->t;
  const int64_t lcount = lds_maps ? lds_params_from_plan(lp, ctx, gv, g->house_lds->plan, g->house_lds->ranges) : 0;
  if (int rc_t = start_timer(ctx)) return rc_t;
  if (lcount > 0) HIP_TRY(launch_house_lds(lp, (int)std::min<long long>((long long)g->cu_count, (long long)lcount), ctx.stream));
  if (count > 0) HIP_TRY(launch_house_acc(p, grid, ctx.stream));
  fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)(count + lcount), grid, 256);
  return end_launch(ctx, FIN_COPY, 0, h_out, 1, st);
}

// house, flattened over (v0, v1, v3) tasks (house_flat_kernel in gm_mine.hip)
static int run_house_flat(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  const GraphView gv = graph_view(g);
  rc = g->house_blocks.ensure(g->mu, [&](HouseBlocks &hb) {  // once per graph: blocks per entry on the device, prefix on the host
    OtherSetupScope scope(g);
    const size_t ne = (size_t)g->ne;
    DevOwn<unsigned> d_nblk;
    HIP_TRY(d_nblk.alloc(sizeof(unsigned) * std::max<size_t>(ne, 1)));
    std::vector<unsigned> nblk(std::max<size_t>(ne, 1));
    hipError_t e = ne ? launch_house_blocks(gv, d_nblk, 0) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(nblk.data(), d_nblk, sizeof(unsigned) * ne, hipMemcpyDeviceToHost);
    d_nblk.reset();
    if (e != hipSuccess) return hip_fail(e, "house block table", __FILE__, __LINE__);
    std::vector<unsigned long long> pre(ne + 1);
    unsigned long long acc = 0;
    for (size_t i = 0; i < ne; ++i) { pre[i] = acc; acc += nblk[i]; }
    pre[ne] = acc;
    hb.n = acc;
    HIP_TRY(hb.prefix.alloc(sizeof(unsigned long long) * (ne + 1)));
    HIP_TRY(hipMemcpy(hb.prefix, pre.data(), sizeof(unsigned long long) * (ne + 1), hipMemcpyHostToDevice));
    return kOnceBuilt;
  });
  if (rc) return rc;
  HouseParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.entry_prefix = g->house_blocks->prefix;
  p.nblocks = g->house_blocks->n;
  p.group = la->chunk > 0 ? la->chunk : 8;
  p.no_bits = (la->tune[6] & GM_T6_HOUSE_NO_BITMAP) ? 1 : 0;
  const long long ngroups = (long long)((p.nblocks + (unsigned long long)p.group - 1) / (unsigned long long)p.group);
  const int64_t count = take_range(ctx, ngroups, p);
  p.counters = g->d_counters;
  p.queue = queue_word64(g, QW64_MAIN);
  const int grid = grid_for((count + 3) / 4, g->cu_count, 8);
  if (int rc_t = start_timer(ctx)) return rc_t;
  if (count > 0 && g->ne > 0) HIP_TRY(launch_house_flat(p, grid, ctx.stream));
  fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)count, grid, 256);
  return end_launch(ctx, FIN_COPY, 0, h_out, 1, st);
}

// rectangle / house / pentagon: one wave per symmetry-broken edge (gm_sgl.hip)
static int run_sgl_nested(int pat, const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  SglParams p;
  memset(&p, 0, sizeof p);
  p.g = graph_view(g);
  p.chunk = la->chunk > 0 ? la->chunk : 64;
  const long long nchunks = (g->ne + p.chunk - 1) / p.chunk;
  const int64_t count = take_range(ctx, nchunks, p);
  p.counters = g->d_counters;
  p.queue = queue_word(g, QW_MAIN);
  p.max_deg = std::max(g->max_deg, 1);
  const int grid = grid_for((count + 3) / 4, g->cu_count, 8);
  if (pat == SGL_HOUSE || pat == SGL_DIAMOND) {  // per-wave list for the materialised S = N(v0) ^ N(v1)
    const size_t need = (size_t)grid * 4 * (size_t)p.max_deg * sizeof(int);
    rc = ensure_scratch(g, need);
    if (rc) return rc;
    p.scratch = reinterpret_cast<int *>(g->scratch.p.get());
  }
  if (int rc_t = start_timer(ctx)) return rc_t;
  if (count > 0) HIP_TRY(launch_sgl_nested(pat, p, grid, ctx.stream));
  fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)count, grid, 256);
  return end_launch(ctx, FIN_COPY, 0, h_out, 1, st);
}

// diamond on one GPU: the edge supports of the oriented copy (cached on the handle; on its topological view where lists are long)
static int run_diamond_supports(const gm_graph *sym, const gm_launch *la, uint64_t *total, gm_stats *st) {
  gm_graph *g = const_cast<gm_graph *>(sym);
  if (!sym) return GM_ERR_INVALID;
  if (la && la->world > 1) return GM_ERR_UNSUPPORTED;
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  gm_graph *dag = g->dag_cache, *run_on = nullptr;
  int rc = topo_view(dag, la, &run_on);
  if (rc) return rc;
  rc = run_pattern({PAT_SUPPORT, 3}, run_on, la, total, 1, st);
  if (rc) return rc;
  record_ran_on_dag(g, run_on);
  return GM_OK;
}

// ---- diamond on several ranks: ONE shared pass over the triangles (the one-GPU algorithm at every N) --------------------------------------
// Every rank runs its share of the triangle pass into its own zeroed support array (one uint32 per entry of the oriented copy, padded so
// that every rank gets the same number of entries), the arrays are summed by ONE reduce-scatter over xGMI (ncclReduceScatter, ncclUint32,
// ncclSum: rank r receives the entries [r n / world, (r + 1) n / world)), every rank takes sum C(t, 2) of its slice, and the 64-bit
// counts meet in the usual all-reduce.  The reference has no multi-GPU diamond at all (src/sgl/multigpu.cu:117 is commented out).
int diamond_run_on(const gm_graph *sym, const gm_launch *la, gm_graph **run_on) {
  gm_graph *g = const_cast<gm_graph *>(sym);
  if (!sym) return GM_ERR_INVALID;
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  gm_graph *dag = g->dag_cache;
  return topo_view(dag, la, run_on);  // (rows beyond the 2048-entry stage: their out-edges through sup_long_kernel)
}
extern "C" int gm_diamond_support_size(const gm_graph *sym, int world, int64_t *n_entries) {
  if (!sym || !n_entries || world < 1) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  const int rc = diamond_run_on(sym, nullptr, &run_on);
  if (rc) return rc;
  *n_entries = diamond_support_entries(run_on->ne, world);
  return GM_OK;
}
// tooling (the byte model of bench.py, tests): what the most recent one-GPU diamond of this handle did with its streamed edges
extern "C" int gm_diamond_support_info(const gm_graph *sym, int64_t info[4]) {
  if (!sym || !info) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  const int rc = diamond_run_on(sym, nullptr, &run_on);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(run_on->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long at = 0;
  HIP_TRY(hipMemcpy(&at, run_on->d_counters + 2, sizeof at, hipMemcpyDeviceToHost));
  info[0] = run_on->sup_masks.built() ? (int64_t)run_on->sup_masks->words : 0;  // 64-bit words of the match-mask arena (0: no masks)
  info[1] = (int64_t)at;                                                  // increments issued as global atomics from the waves' queues
  info[2] = run_on->sup_masks.built() ? (int64_t)run_on->sup_masks->n_far_rows : 0;
  info[3] = (int64_t)sup_mask_min_tail(run_on);
  return GM_OK;
}
// tooling: the hub corner whose supports the one-GPU diamond of this handle takes on the matrix cores (after a first diamond)
extern "C" int gm_sup_core_info(const gm_graph *sym, int64_t info[4]) {
  if (!sym || !info) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  const int rc = diamond_run_on(sym, nullptr, &run_on);
  if (rc) return rc;
  const bool on = run_on->tasklists->skip_from < run_on->nv;
  const long long nb = on ? run_on->tasklists->core_h >> 8 : 0;
  info[0] = on ? run_on->tasklists->core_h : 0;  // vertices of the corner (0: every edge's support comes from the triangle pass)
  info[1] = 0;
  if (on) {
    int e0 = 0;
    HIP_TRY(hipSetDevice(run_on->device));
    HIP_TRY(hipMemcpy(&e0, run_on->d_rp + run_on->tasklists->skip_from, sizeof(int), hipMemcpyDeviceToHost));
    info[1] = run_on->ne - (long long)e0;  // DAG entries inside it
  }
  info[2] = nb * (nb + 1) / 2;           // pairs of 256-row blocks of the product
  info[3] = on ? (run_on->tasklists->core_h >> 9) : 0;  // 512-column chunks of a row
  return GM_OK;
}
// tooling (tests): the plan the rectangle / the house of this handle built for its LDS maps (after a first gm_sgl of that pattern with the
// maps in LDS), on the copy that call ran on: the handle the most recent call was recorded on where it holds the plan, else the handle itself
// (the house; the rectangle under GM_T6_AS_NUMBERED), else its copy numbered ascending in degree.  Read-only: nothing is built here.
//   out[0] ranges n   [1] cut   [2] {v, k} LDS tasks   [3] {v, -1} LDS tasks   [4] front acc tasks (n_cut)   [5] whole-workgroup acc tasks
//   [6] four-to-a-task acc tasks   [7] whole-workgroup tasks among the front;   the rectangle: [8 .. 8 + n] rb[0 .. n], then lb[0 .. n)
extern "C" int gm_map_plan_info(const gm_graph *sym, const char *pattern, int64_t *out, int n) {
  if (!sym || !pattern || !out) return GM_ERR_INVALID;
  const bool is_rect = strcmp(pattern, "rectangle") == 0;
  if (!is_rect && strcmp(pattern, "house") != 0) return GM_ERR_INVALID;
  auto has = [&](const gm_graph *g) { return g && (is_rect ? g->rect_lds.built() : g->house_lds.built()); };
  const gm_graph *on = has(sym->ring_alias) ? sym->ring_alias : has(sym) ? sym : has(sym->relabel_cache[0]) ? sym->relabel_cache[0] : nullptr;
  if (!on) return GM_ERR_INVALID;  // (no such call yet)
  const CentrePlan &pl = is_rect ? on->rect_lds->plan : on->house_lds->plan;
  const int nr = is_rect ? on->rect_lds->ranges.n : on->house_lds->ranges.n;
  if (n < 8 + (is_rect ? 2 * nr + 1 : 0)) return GM_ERR_INVALID;
  out[0] = nr;
  out[1] = pl.cut;
  out[2] = (int64_t)pl.n_lds_range;
  out[3] = (int64_t)pl.n_lds_whole;
  out[4] = (int64_t)pl.n_cut;
  out[5] = (int64_t)pl.n_acc_heavy;
  out[6] = (int64_t)(pl.n_acc_tasks - pl.n_acc_heavy);
  out[7] = (int64_t)pl.n_front_heavy;
  if (is_rect) {
    for (int k = 0; k <= nr; ++k) out[8 + k] = on->rect_lds->ranges.rb[k];
    for (int k = 0; k < nr; ++k) out[9 + nr + k] = on->rect_lds->ranges.lb[k];
  }
  return GM_OK;
}
extern "C" int gm_diamond_support_partial(const gm_graph *sym, const gm_launch *la, uint32_t *d_support, int64_t n_entries, gm_stats *st) {
  if (!d_support) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  int rc = diamond_run_on(sym, la, &run_on);
  if (rc) return rc;
  const int world = (la && la->world > 1) ? la->world : 1;
  // (at least gm_diamond_support_size; the ranks' slices are cut from THAT size -- size / world entries each -- whatever the buffer holds beyond it)
  if (n_entries < diamond_support_entries(run_on->ne, world)) return GM_ERR_INVALID;
  uint64_t dummy = 0;
  rc = run_pattern({PAT_SUPPORT_PART, 3, -1, 0, d_support}, run_on, la, (la && la->d_counts) ? nullptr : &dummy, 1, st);
  if (rc) return rc;
  record_ran_on_dag(sym, run_on);
  return GM_OK;
}
extern "C" int gm_diamond_support_finish(const gm_graph *sym, const gm_launch *la, const uint32_t *d_support, int64_t count, uint64_t *total, gm_stats *st) {
  if (!d_support || count < 0) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  int rc = diamond_run_on(sym, la, &run_on);
  if (rc) return rc;
  LaunchCtx ctx;
  rc = begin_launch(run_on, la, total, ctx);
  if (rc) return rc;
  if (int rc_t = start_timer(ctx)) return rc_t;
  HIP_TRY(launch_sup_pairs(d_support, 0, (long long)count, run_on->d_counters, run_on->cu_count, ctx.stream));
  fill_stats(st, (uint64_t)count, 0, 0, 256);
  rc = end_launch(ctx, FIN_COPY, 0, total, 1, st);
  if (rc) return rc;
  record_ran_on_dag(sym, run_on);
  return GM_OK;
}

static int sgl4_kind(const char *pattern) {  // 1 tailedtriangle, 2 4path, 3 3star, 0 none of them
  if (!pattern) return 0;
  return strcmp(pattern, "tailedtriangle") == 0 ? 1 : strcmp(pattern, "4path") == 0 ? 2 : strcmp(pattern, "3star") == 0 ? 3 : 0;
}

// A rank's share of the four per-edge sums behind tailedtriangle / 4path / 3star (see gm_sgl): plain sums over its tasks, so the shares
// add up; with la->d_counts they are left in that device buffer, ordered on la->stream (raw may be NULL then).
extern "C" int gm_sgl4_partial(const gm_graph *sym, const gm_launch *la, uint64_t raw[4], gm_stats *st) {
  if (!sym || (!raw && !(la && la->d_counts))) return GM_ERR_INVALID;
  if (int rc0 = reject_big(sym)) return rc0;
  const int rc = run_pattern({PAT_MOTIF4E, 4, FIN_RAW4}, sym, la, raw, 4, st);
  if (rc) return rc;
  record_ran_on(sym, sym);  // (ring_extra stays as start_timer left it)
  return GM_OK;
}

extern "C" int gm_sgl4_finish(const char *pattern, const uint64_t raw[4], uint64_t *total) {
  const int kind = sgl4_kind(pattern);
  if (!kind || !raw || !total) return GM_ERR_INVALID;
  *total = kind == 1 ? raw[2] / 2 + raw[3] : kind == 2 ? raw[1] + raw[2] + raw[3] : (raw[0] + 2 * raw[2] + 2 * raw[3]) / 6;
  return GM_OK;
}

// ---- the six 5-vertex patterns of src/sgl/omp_base.cc:29-45 as closed forms of eleven raw sums (DESIGN.md "SgL, 5-vertex closed forms") ----
enum Sgl5Raw : int { R5_T = 0, R5_D, R5_W, R5_A, R5_B, R5_H, R5_S, R5_P, R5_K4, R5_R, R5_Q };
static_assert(R5_Q + 1 == GM_SGL5_NRAW, "the order of the raw sums is ABI");
// the raw sums a pattern needs as a bit mask (0: not one of the six); "all": every sum
static unsigned sgl5_needs(const char *pattern) {
  if (!pattern) return 0u;
  auto b = [](int i) { return 1u << i; };
  if (strcmp(pattern, "hourglass") == 0) return b(R5_H) | b(R5_D);
  if (strcmp(pattern, "taileddiamond2") == 0) return b(R5_W);
  if (strcmp(pattern, "taileddiamond") == 0) return b(R5_A) | b(R5_K4);
  if (strcmp(pattern, "semihouse") == 0) return b(R5_B) | b(R5_K4);
  if (strcmp(pattern, "closedhouse") == 0) return b(R5_Q);
  if (strcmp(pattern, "5path") == 0) return b(R5_P) | b(R5_S) | b(R5_T) | b(R5_R);
  return 0u;
}

extern "C" int gm_sgl5_finish(const char *pattern, const uint64_t raw[GM_SGL5_NRAW], uint64_t *total) {
  if (!sgl5_needs(pattern) || !raw || !total) return GM_ERR_INVALID;
  if (strcmp(pattern, "hourglass") == 0) *total = raw[R5_H] - 2ull * raw[R5_D];
  else if (strcmp(pattern, "taileddiamond2") == 0) *total = raw[R5_W];
  else if (strcmp(pattern, "taileddiamond") == 0) *total = raw[R5_A] - 12ull * raw[R5_K4];
  else if (strcmp(pattern, "semihouse") == 0) *total = raw[R5_B] - 12ull * raw[R5_K4];
  else if (strcmp(pattern, "closedhouse") == 0) *total = raw[R5_Q];
  else *total = raw[R5_P] - 2ull * raw[R5_S] + 9ull * raw[R5_T] - 4ull * raw[R5_R];
  return GM_OK;
}

// the per-handle arrays of the weighted pass on the DAG it runs on; the symmetric degrees are built once
static int ensure_w5_buffers(gm_graph *g) {
  HIP_TRY(hipSetDevice(g->device));
  const size_t ne = (size_t)std::max<long long>(g->ne, 1), nv = (size_t)std::max(g->nv, 1);
  if (const int rc = g->w5deg.ensure(g->mu, [&](SymDegrees &sd) {
        HIP_TRY(sd.deg.alloc(sizeof(int) * nv));
        HIP_TRY(launch_wtri_degrees(g->nv, g->ne, g->d_rp, g->d_col, sd.deg, g->cu_count, 0));
        HIP_TRY(hipDeviceSynchronize());
        return kOnceBuilt;
      })) return rc;
  std::lock_guard<std::mutex> lk(g->mu);
  if (g->w5.out) return GM_OK;
  if (!g->w5.sup) HIP_TRY(g->w5.sup.alloc(sizeof(unsigned) * (size_t)diamond_support_entries(g->ne, 1)));
  if (!g->w5.ed) HIP_TRY(g->w5.ed.alloc(sizeof(unsigned) * ne));
  if (!g->w5.tv2) HIP_TRY(g->w5.tv2.alloc(sizeof(unsigned long long) * nv));
  HIP_TRY(g->w5.out.alloc(64));
  return GM_OK;
}

// one kernel of the symmetric graph that leaves ONE sum in counters[0] (P, Q): a launch of its own on the handle
template <class Launch>
static int run_sym_sum(const gm_graph *sym, const gm_launch *la, uint64_t *out, SubLaunches &sub, Launch launch) {
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, la, out, ctx)) return rc;
  if (int rc = start_timer(ctx)) return rc;
  if (int rc = launch(ctx)) return rc;
  return sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_COPY, 0, out, 1, s); });
}

// the raw sums of the bit mask `needs` (gm_sgl5_raw: those of a pattern; gm_sgl6_raw: D, B, K4, or T for the arrays of the pass alone)
static int sgl5_raw_needs(const gm_graph *sym, unsigned needs, const gm_launch *la, uint64_t raw[GM_SGL5_NRAW], gm_stats *st) {
  if (!sym || !raw || !needs) return GM_ERR_INVALID;
  for (int i = 0; i < GM_SGL5_NRAW; ++i) raw[i] = 0;
  if (int rc0 = reject_big(sym)) return rc0;
  // the divisions and halvings need the sums of the whole graph, and the total is put together on the host: one rank, synchronous
  if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  auto need = [&](int i) { return (needs >> i & 1u) != 0; };
  SubLaunches sub;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  if (sym->ne == 0) return GM_OK;
  if (need(R5_T) || need(R5_D) || need(R5_W) || need(R5_A) || need(R5_B) || need(R5_H) || need(R5_S)) {
    // the supports of every entry of the oriented copy, filled like a one-rank gm_diamond_support_partial (rows beyond the stage through
    // sup_long_kernel), into an array of the 5-vertex forms' own; then the sums over entries, triangles and vertices
    gm_graph *run_on = nullptr;
    if (int rc = diamond_run_on(sym, &l2, &run_on)) return rc;
    if (int rc = ensure_w5_buffers(run_on)) return rc;
    uint64_t dummy = 0, ab[4] = {0, 0, 0, 0};
    if (int rc = sub.run([&](gm_stats *s) { return run_pattern({PAT_SUPPORT_PART, 3, -1, 0, run_on->w5.sup}, run_on, &l2, &dummy, 1, s); })) return rc;
    PatternReq weighted{PAT_WTRI, 3, FIN_RAW4};
    weighted.wtri_tri = need(R5_A) || need(R5_B);
    weighted.wtri_vert = need(R5_H) || need(R5_S);
    if (int rc = sub.run([&](gm_stats *s) { return run_pattern(weighted, run_on, &l2, ab, 4, s); })) return rc;
    unsigned long long o[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(o, run_on->w5.out, sizeof o, hipMemcpyDeviceToHost));  // (run_pattern has synchronised the stream)
    const uint64_t v[7] = {o[0] / 3ull, o[1], o[2], ab[0], ab[1], o[3], o[4]};
    const int at[7] = {R5_T, R5_D, R5_W, R5_A, R5_B, R5_H, R5_S};
    for (int i = 0; i < 7; ++i)
      if (need(at[i])) raw[at[i]] = v[i];
  }
  if (need(R5_K4)) {
    if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;
    if (int rc = sub.run([&](gm_stats *s) { return gm_clique(g->dag_cache, 4, &l2, &raw[R5_K4], s); })) return rc;
  }
  if (need(R5_R)) {
    if (int rc = sub.run([&](gm_stats *s) { return gm_sgl(sym, "rectangle", &l2, &raw[R5_R], s); })) return rc;
  }
  if (need(R5_P)) {
    if (int rc = run_sym_sum(sym, &l2, &raw[R5_P], sub, [&](LaunchCtx &c) {
          HIP_TRY(launch_path5(g->nv, g->d_rp, g->d_col, g->d_counters, g->cu_count, c.stream));
          return (int)GM_OK;
        })) return rc;
  }
  if (need(R5_Q)) {
    const int grid = chouse_grid(g->ne, g->cu_count);
    if (int rc = ensure_scratch(g, sizeof(int) * (size_t)grid * 4 * (size_t)std::max(g->max_deg, 1))) return rc;
    if (int rc = run_sym_sum(sym, &l2, &raw[R5_Q], sub, [&](LaunchCtx &c) {
          ChouseParams cp;
          memset(&cp, 0, sizeof cp);
          cp.nv = g->nv; cp.ne = g->ne; cp.rp = g->d_rp; cp.col = g->d_col;
          cp.scratch = reinterpret_cast<int *>(g->scratch.p.get()); cp.max_deg = std::max(g->max_deg, 1); cp.out = g->d_counters;
          HIP_TRY(launch_chouse(cp, grid, c.stream));
          return (int)GM_OK;
        })) return rc;
  }
  record_ran_on(g, g, true);
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

extern "C" int gm_sgl5_raw(const gm_graph *sym, const char *pattern, const gm_launch *la, uint64_t raw[GM_SGL5_NRAW], gm_stats *st) {
  if (!sym || !pattern || !raw) return GM_ERR_INVALID;
  return sgl5_raw_needs(sym, strcmp(pattern, "all") == 0 ? (1u << GM_SGL5_NRAW) - 1u : sgl5_needs(pattern), la, raw, st);
}
// the same by bit mask (bit i: raw[i]), as gm_sgl6_raw takes its sums: A or B of a dense graph without its 4-cliques
extern "C" int gm_sgl5_raw_need(const gm_graph *sym, uint32_t need, const gm_launch *la, uint64_t raw[GM_SGL5_NRAW], gm_stats *st) {
  if (!sym || !raw || !need || (need >> GM_SGL5_NRAW)) return GM_ERR_INVALID;
  return sgl5_raw_needs(sym, need, la, raw, st);
}

extern "C" int gm_sgl(const gm_graph *sym, const char *pattern, const gm_launch *la, uint64_t *total, gm_stats *st) {
  if (!pattern) return GM_ERR_INVALID;
  if (strcmp(pattern, "diamond") == 0) {
    // tune[6] & GM_T6_SGL_NESTED: the LISTING (nested) form of the reference, src/sgl/gpu_kernels/diamond_nested.cuh:4-31 -- materialise
    // S, count_smaller per member -- as a second implementation; the default counts C(|S|,2) per edge (diamond_count.cuh:15-17)
    if (la && (la->tune[6] & GM_T6_SGL_NESTED)) return run_sgl_nested(SGL_DIAMOND, sym, la, total, st);
    // One GPU: |N(v0) ^ N(v1)| of EVERY edge from one pass over the triangles of the DAG (edge supports, gm_sup.hip), then sum C(t, 2).
    // Several ranks, DAG rows beyond the 2048-entry stage, or one of the A/B switches of the per-edge kernels (tune[6] & GM_T6_PER_EDGE: that
    // path on request): one intersection of the two symmetric lists per edge (gm_hrow.hip, gm_chunk.h).
    {
      const int t6 = la ? la->tune[6] : 0;
      const bool big = sym && sym->d_rp64;  // (>= 2^31 entries: only the supports of the oriented copy can run; on one GPU)
      const bool per_edge = ((t6 & (GM_T6_PER_EDGE | GM_T6_NO_CLASSES | GM_T6_FORCE_CLASSES | GM_T6_CLASSES_SORTED_COPY | GM_T6_GIANT_SPLIT | GM_T6_HROW_MUL32)) || (la && la->world > 1) ||
                             (la && la->tune[5] == 1) || gm_opt("GM_DIAMOND_PER_EDGE") || !sym) && !big;
      if (!per_edge) {
        const int rc = run_diamond_supports(sym, la, total, st);
        if (rc != GM_ERR_UNSUPPORTED) return rc;
        if (big) return reject_big(sym);
      }
    }
    return run_pattern({PAT_DIAMOND, 4}, sym, la, total, 1, st);
  }
  // rectangle / house / pentagon run on a copy of the graph renumbered by degree (get_relabeled; tune[6] & GM_T6_AS_NUMBERED: on the
  // graph as given). tune[6] & GM_T6_SGL_NESTED: the wave-per-edge loop nests; & GM_T6_SGL_FLAT: rectangle as wedges + flat intersections,
  // house without the LDS S-bitmap (A/B, tests).
  const bool is_rect = strcmp(pattern, "rectangle") == 0, is_house = strcmp(pattern, "house") == 0, is_pent = strcmp(pattern, "pentagon") == 0;
  if (is_rect || is_house || is_pent) {
    if (!sym) return GM_ERR_INVALID;
    if (int rc0 = reject_big(sym)) return rc0;
    const int t6 = la ? la->tune[6] : 0;
    const gm_graph *run_on = sym;
    const bool wedge_form = (is_pent || is_rect) && (t6 & GM_T6_SGL_FLAT);  // anchored wedges: hubs first; 2-path / (v0,v1,v3) forms: hubs last
    // house: by wedge accumulation (default; its 2-path count does not depend on the numbering, so no renumbered copy), or
    // the flattened (v0, v1, v3) form (GM_T6_SGL_FLAT; GM_T6_HOUSE_NO_BITMAP: without the LDS S-bitmap). The packed map holds 24-bit counts and
    // 40-bit weighted sums: rows of 2^20 entries or more take the flattened form.
    const bool house_acc = is_house && !(t6 & (GM_T6_SGL_NESTED | GM_T6_SGL_FLAT | GM_T6_HOUSE_NO_BITMAP)) && sym->max_deg < (1 << 20);
    if (!(t6 & GM_T6_AS_NUMBERED) && !(t6 & GM_T6_SGL_NESTED) && !house_acc) {
      gm_graph *r = nullptr;
      int rc = get_relabeled(const_cast<gm_graph *>(sym), wedge_form ? 1 : 0, &r);
      if (rc) return rc;
      run_on = r;
    }
    int rc;
    if (t6 & GM_T6_SGL_NESTED) rc = run_sgl_nested(is_rect ? SGL_RECTANGLE : is_house ? SGL_HOUSE : SGL_PENTAGON, run_on, la, total, st);
    else if (house_acc) rc = run_house_acc(run_on, la, total, st);
    else if (is_house) rc = run_house_flat(run_on, la, total, st);
    else if (is_pent && (t6 & GM_T6_SGL_FLAT)) rc = run_rect_flat(run_on, la, total, st, true);
    else if (is_pent) rc = run_rect_acc(run_on, la, total, st, true);
    else if (t6 & GM_T6_SGL_FLAT) rc = run_rect_flat(run_on, la, total, st);
    else rc = run_rect_acc(run_on, la, total, st);
    record_ran_on(sym, run_on);  // (whatever rc)
    return rc;
  }
  // The other 4-vertex patterns of src/sgl/omp_base.cc:21-31 (round 6) need no enumeration of their own: with tri = |N(u) ^ N(v)|,
  // su = d(u) - tri - 1, sv = d(v) - tri - 1 per undirected edge -- the four per-edge sums of the formula 4-motif (PAT_MOTIF4E,
  // src/motif/cpu_kernels/automine_formula.h:33-41: raw0 = sum su (su - 1) + sv (sv - 1), raw1 = sum su sv, raw2 = sum tri (su + sv),
  // raw3 = sum tri (tri - 1)) --
  //   tailedtriangle (tailedtriangle.h:1-12) = sum_v t(v) (d(v) - 2) = 1/2 sum_e tri (d(u) + d(v) - 4)         = raw2 / 2 + raw3
  //   4path          (4path.h:1-14)          = sum_e (d(u) - 1)(d(v) - 1) - 3 T  (T = 1/3 sum_e tri)            = raw1 + raw2 + raw3
  //   3star          (3star.h:1-13)          = sum_v C(d(v), 3) = 1/6 sum_e [(d(u)-1)(d(u)-2) + (d(v)-1)(d(v)-2)] = (raw0 + 2 raw2 + 2 raw3) / 6
  // (the reference's symmetry breaking makes each of them the plain edge-induced count; checked against sgl_omp_base on the seven golden
  // graphs).  The divisions need the sums of the whole graph: a rank's share goes through gm_sgl4_partial.
  if (sgl4_kind(pattern)) {
    if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;  // several ranks: gm_sgl4_partial + all-reduce + gm_sgl4_finish
    uint64_t raw[4] = {0, 0, 0, 0};
    const int rc = gm_sgl4_partial(sym, la, raw, st);
    return rc ? rc : gm_sgl4_finish(pattern, raw, total);
  }
  // The six 5-vertex patterns beyond house / pentagon (5path, semihouse, closedhouse, hourglass, taileddiamond, taileddiamond2): closed
  // forms of eleven raw sums over edge supports, triangles and degrees (gm_sgl5_raw / gm_sgl5_finish, gm_wtri.hip).  One rank, and the total
  // is put together on the host: world > 1 or d_counts -> GM_ERR_UNSUPPORTED.
  if (sgl5_needs(pattern)) {
    if (total) *total = 0;
    if (!total) return (la && la->d_counts) ? GM_ERR_UNSUPPORTED : GM_ERR_INVALID;
    uint64_t raw[GM_SGL5_NRAW];
    const int rc = gm_sgl5_raw(sym, pattern, la, raw, st);
    return rc ? rc : gm_sgl5_finish(pattern, raw, total);
  }
  if (total) *total = 0;  // "Not implemented", total_num = 0 (src/sgl/omp_base.cc:51-53): 6path, dumbbell
  return GM_ERR_UNSUPPORTED;
}

// ---- 6path and dumbbell (src/sgl/omp_base.cc:46-50) as closed forms of nine raw sums (DESIGN.md "SgL, 6-vertex closed forms") ---------------
//   6path = X - Y - 2 Z + 12 R + 4 D - 5 C5,   dumbbell = M - B + 6 K4
// behind entry points of their own: gm_sgl above keeps answering GM_ERR_UNSUPPORTED for the two names (tests/test_gpu_sgl5.py pins that);
// routing it here is a later one-line change.
enum Sgl6Raw : int { R6_X = 0, R6_Y, R6_Z, R6_R, R6_D, R6_C5, R6_M, R6_B, R6_K4 };
static_assert(R6_K4 + 1 == GM_SGL6_NRAW, "the order of the raw sums is ABI");
static unsigned sgl6_needs(const char *pattern) {
  if (!pattern) return 0u;
  auto b = [](int i) { return 1u << i; };
  if (strcmp(pattern, "6path") == 0) return b(R6_X) | b(R6_Y) | b(R6_Z) | b(R6_R) | b(R6_D) | b(R6_C5);
  if (strcmp(pattern, "dumbbell") == 0) return b(R6_M) | b(R6_B) | b(R6_K4);
  return 0u;
}

extern "C" int gm_sgl6_need(const char *pattern, uint32_t *mask) {
  if (!pattern || !mask) return GM_ERR_INVALID;
  *mask = strcmp(pattern, "all") == 0 ? (1u << GM_SGL6_NRAW) - 1u : sgl6_needs(pattern);
  return *mask ? GM_OK : GM_ERR_INVALID;
}

extern "C" int gm_sgl6_finish(const char *pattern, const uint64_t raw[GM_SGL6_NRAW], uint64_t *total) {
  if (!sgl6_needs(pattern) || !raw || !total) return GM_ERR_INVALID;
  if (strcmp(pattern, "6path") == 0) *total = raw[R6_X] - raw[R6_Y] - 2ull * raw[R6_Z] + 12ull * raw[R6_R] + 4ull * raw[R6_D] - 5ull * raw[R6_C5];
  else *total = raw[R6_M] - raw[R6_B] + 6ull * raw[R6_K4];
  return GM_OK;
}

// Z and R (out[0], out[1]) by wrect_kernel on the copy numbered ascending in degree (tune[6] & GM_T6_AS_NUMBERED: on the graph as given).  The plan
// is built once per graph that runs it: GM_WRECT_RANGE (ids per LDS range, default and limit kWrectRange) is read then.
static int run_wrect(const gm_graph *sym, const gm_launch *la_in, uint64_t out[2], gm_stats *st) {
  gm_graph *self = const_cast<gm_graph *>(sym);
  const gm_graph *run_on = sym;
  if (!(la_in && (la_in->tune[6] & GM_T6_AS_NUMBERED))) {
    gm_graph *r = nullptr;
    if (int rc = get_relabeled(self, 0, &r)) return rc;
    run_on = r;
  }
  uint64_t v[4] = {0, 0, 0, 0};
  LaunchCtx ctx;
  if (int rc = begin_launch(run_on, la_in, v, ctx)) return rc;
  gm_graph *g = ctx.g;
  const GraphView gv = graph_view(g);
  if (int rc = ensure_idx0(g, gv)) return rc;
  if (const int rc = g->wrect.ensure(g->mu, [&](WrectPlan &wp) {  // (two first calls on one handle: one builds, the other waits)
    OtherSetupScope scope(g);
    const size_t nv = (size_t)g->nv;
    int range = kWrectRange;
    if (const char *e = gm_opt("GM_WRECT_RANGE")) range = std::max(16, std::min(kWrectRange, std::atoi(e)));
    const long long nranges = std::max<long long>(1, ((long long)g->nv + range - 1) / range);
    wp.range = range;
    wp.grp = (int)((nranges + 63) / 64);
    HIP_TRY(wp.mask.alloc(sizeof(unsigned long long) * std::max<size_t>(nv, 1)));
    HIP_TRY(launch_wrect_mask(g->nv, g->d_rp, g->d_col, range, wp.grp, wp.mask, g->cu_count, 0));
    std::vector<int> idx0h(std::max<size_t>(nv, 1));
    if (nv) HIP_TRY(hipMemcpy(idx0h.data(), g->rect_idx->idx0, sizeof(int) * nv, hipMemcpyDeviceToHost));
    const std::vector<int2> tasks = wrect_tasks(idx0h.data(), nv, range, kWrectThreads);  // (the hubs' per-range tasks first)
    wp.n_tasks = tasks.size();
    HIP_TRY(wp.tasks.alloc(sizeof(int2) * std::max<size_t>(tasks.size(), 1)));
    if (!tasks.empty()) HIP_TRY(hipMemcpy(wp.tasks, tasks.data(), sizeof(int2) * tasks.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return kOnceBuilt;
  })) return rc;
  WrectParams p;
  memset(&p, 0, sizeof p);
  p.rp = g->d_rp; p.col = g->d_col; p.idx0 = g->rect_idx->idx0;
  p.rmask = g->wrect->mask; p.range = g->wrect->range; p.grp = g->wrect->grp;
  p.tasks = g->wrect->tasks; p.count = g->wrect->n_tasks;
  p.queue = queue_word64(g, QW64_MAIN);
  p.counters = g->d_counters;
  if (int rc = start_timer(ctx)) return rc;
  const int grid = grid_for((long long)p.count, g->cu_count, wrect_per_cu());
  if (p.count > 0) HIP_TRY(launch_wrect(p, grid, ctx.stream));
  fill_stats(st, (uint64_t)g->ne, (uint64_t)p.count, grid, kWrectThreads);
  const int rc = end_launch(ctx, FIN_RAW4, 0, v, 4, st);
  out[0] = v[0];
  out[1] = v[1];
  record_ran_on(sym, run_on);  // (whatever rc)
  return rc;
}

extern "C" int gm_sgl6_raw(const gm_graph *sym, uint32_t need, const gm_launch *la, uint64_t raw[GM_SGL6_NRAW], gm_stats *st) {
  if (!sym || !raw || !need || (need >> GM_SGL6_NRAW)) return GM_ERR_INVALID;
  for (int i = 0; i < GM_SGL6_NRAW; ++i) raw[i] = 0;
  if (int rc0 = reject_big(sym)) return rc0;
  if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;  // (the closed forms are applied on the host: one rank, synchronous)
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  auto want = [&](int i) { return (need >> i & 1u) != 0; };
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  HIP_TRY(hipSetDevice(g->device));
  if (int rc = require_sorted_rows(g)) return rc;  // (as in every solver, before any of the sub-launches builds a table)
  if (sym->ne == 0) return GM_OK;
  SubLaunches sub;
  const bool entry_sums = want(R6_X) || want(R6_Y) || want(R6_M);
  if (entry_sums || want(R6_D) || want(R6_B) || want(R6_K4)) {
    // D, B and K4 are sums of the 5-vertex forms; X, M and Y read the arrays their pass leaves on the DAG it ran on -- the supports of the
    // entries, 2 T_v, the symmetric degrees -- so the pass runs for them too (T asks for nothing but the pass itself)
    unsigned n5 = (want(R6_D) ? 1u << R5_D : 0u) | (want(R6_B) ? 1u << R5_B : 0u) | (want(R6_K4) ? 1u << R5_K4 : 0u);
    if (entry_sums && !(n5 & ((1u << R5_D) | (1u << R5_B)))) n5 |= 1u << R5_T;
    uint64_t raw5[GM_SGL5_NRAW];
    if (int rc = sub.run([&](gm_stats *s) { return sgl5_raw_needs(sym, n5, &l2, raw5, s); })) return rc;
    raw[R6_D] = want(R6_D) ? raw5[R5_D] : 0;
    raw[R6_B] = want(R6_B) ? raw5[R5_B] : 0;
    raw[R6_K4] = want(R6_K4) ? raw5[R5_K4] : 0;
  }
  if (entry_sums) {
    gm_graph *run_on = nullptr;
    if (int rc = diamond_run_on(sym, &l2, &run_on)) return rc;  // (the handle the pass above ran on)
    if (!run_on->w5.sup || !run_on->w5.tv2 || !run_on->w5deg->deg) return GM_ERR_INVALID;
    {
      std::lock_guard<std::mutex> lk(run_on->mu);
      if (!run_on->w5.s6e1) HIP_TRY(run_on->w5.s6e1.alloc(sizeof(unsigned) * (size_t)std::max(run_on->nv, 1)));
    }
    uint64_t v[4] = {0, 0, 0, 0};
    LaunchCtx ctx;
    if (int rc = begin_launch(run_on, &l2, v, ctx)) return rc;
    HIP_TRY(hipMemsetAsync(run_on->w5.s6e1, 0, sizeof(unsigned) * (size_t)std::max(run_on->nv, 1), ctx.stream));
    if (int rc = start_timer(ctx)) return rc;
    Sgl6EntryParams ep;
    memset(&ep, 0, sizeof ep);
    ep.nv = run_on->nv; ep.ne = run_on->ne; ep.rp = run_on->d_rp; ep.col = run_on->d_col;
    ep.sup = run_on->w5.sup; ep.deg = run_on->w5deg->deg; ep.tv2 = run_on->w5.tv2; ep.e1 = run_on->w5.s6e1; ep.out = run_on->d_counters;
    HIP_TRY(launch_sgl6_sums(ep, run_on->cu_count, ctx.stream));
    if (int rc = sub.run([&](gm_stats *s) { return end_launch(ctx, FIN_RAW4, 0, v, 4, s); })) return rc;
    raw[R6_X] = want(R6_X) ? v[0] : 0;
    raw[R6_M] = want(R6_M) ? v[1] : 0;
    raw[R6_Y] = want(R6_Y) ? v[2] : 0;
  }
  if (want(R6_Z)) {  // (the kernel of Z counts R on the way: the rectangle path is only asked when Z is not)
    uint64_t zr[2] = {0, 0};
    if (int rc = sub.run([&](gm_stats *s) { return run_wrect(sym, &l2, zr, s); })) return rc;
    raw[R6_Z] = zr[0];
    raw[R6_R] = want(R6_R) ? zr[1] : 0;
  } else if (want(R6_R)) {
    if (int rc = sub.run([&](gm_stats *s) { return gm_sgl(sym, "rectangle", &l2, &raw[R6_R], s); })) return rc;
  }
  if (want(R6_C5)) {
    if (int rc = sub.run([&](gm_stats *s) { return gm_sgl(sym, "pentagon", &l2, &raw[R6_C5], s); })) return rc;
  }
  record_ran_on(g, g, true);
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  if (st) st->kernel_ms = sub.ms;
  return GM_OK;
}

extern "C" int gm_sgl6(const gm_graph *sym, const char *pattern, const gm_launch *la, uint64_t *total, gm_stats *st) {
  if (total) *total = 0;
  const unsigned need = sgl6_needs(pattern);
  if (!sym || !total || !need) return GM_ERR_INVALID;
  uint64_t raw[GM_SGL6_NRAW];
  const int rc = gm_sgl6_raw(sym, need, la, raw, st);
  return rc ? rc : gm_sgl6_finish(pattern, raw, total);
}
