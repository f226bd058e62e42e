// gm_launch.hip -- the launch layer behind the solvers of the C ABI (its interface: gm_launch.h): launch prologue / epilogue, run_pattern (TC, edge
// supports, diamond, 3-motif, k-clique, the per-edge sums of 4-motif) as a driver over plan_pattern / fill_mine_params / prepare_scratch / launch_*,
// gm_kernel_times, the DAG estimates, gm_tc / gm_clique / gm_motif*, and every kernel of the layer (gm_solve_sgl.hip, gm_solve_local.hip: host code only).
// Reference launch logic: src/triangle/gpu_base.cu:36-45, src/sgl/gpu_base.cu:37-75, src/clique/gpu_base.cu:28-50, src/motif/gpu_base.cu:42-75.
#include "gm_launch.h"

using namespace gm;

// ------------------------------------------------------------------------------------------------
// solvers
// ------------------------------------------------------------------------------------------------
// counters -> counts, the same arithmetic on both sides (finalize_kernel on the device, end_launch on the host); returns how many it wrote
__host__ __device__ static inline int finalize_math(int mode, unsigned long long base, const unsigned long long *c, unsigned long long *out) {
  if (mode == FIN_MOTIF3) {
    out[0] = c[2] - c[0];  // wedges = sum_e idx(e) - sum_e |A' ^ B|   (automine_base.h:13)
    out[1] = c[1];         // triangles                                  (automine_base.h:18)
  } else if (mode == FIN_MOTIF3_FORMULA) {
    out[0] = base - 3ull * c[0];  // wedges = sum_v C(d,2) - 3T  (src/motif/omp_formula.cc:39-40); base only on rank 0
    out[1] = c[0];
  } else if (mode == FIN_RAW4) {
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
  } else if (mode == FIN_HALF_SIGNED) {
    out[0] = (unsigned long long)((long long)c[0] >> 1);  // an even two's-complement sum (pent_acc_kernel): rank partials add up mod 2^64
  } else {
    out[0] = c[0];
  }
  return mode == FIN_RAW4 ? 4 : (mode == FIN_MOTIF3 || mode == FIN_MOTIF3_FORMULA) ? 2 : 1;
}

__global__ void finalize_kernel(int mode, unsigned long long base, const unsigned long long *__restrict__ c,
                                unsigned long long *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  finalize_math(mode, base, c, out);
}

// a big handle (ne >= 2^31, 64-bit offsets): the mining kernels index the graph they walk with 32 bits
int reject_big(const gm_graph *g) {
  if (!g || !g->d_rp64) return GM_OK;
  g_last_error = "this solver walks the graph it is given with a 32-bit task index; " + std::to_string(g->ne) +
                 " entries: orient it (gm_graph_orient) for TC / k-clique, gm_motif k = 3 counts through the formula solver";
  return GM_ERR_TOO_LARGE;
}

// One 64-bit sum over the arrays of a handle (the reductions over the offsets below, the triangle sample): 8 bytes on the device, zeroed,
// `launch(d_sum)` adds into them (skipped when there is nothing to sum), copied back
template <class Launch>
static int reduce_to_u64(const gm_graph *g, bool nonempty, const char *what, unsigned long long *sum, Launch launch) {
  HIP_TRY(hipSetDevice(g->device));
  DevOwn<unsigned long long> d_s;
  HIP_TRY(d_s.alloc(8));
  hipError_t e = hipMemset(d_s, 0, 8);
  if (e == hipSuccess && nonempty) launch(d_s.get());
  if (e == hipSuccess) e = hipMemcpy(sum, d_s, 8, hipMemcpyDeviceToHost);
  return e == hipSuccess ? GM_OK : hip_fail(e, what, __FILE__, __LINE__);
}
static dim3 rows_grid(const gm_graph *g) { return dim3((unsigned)std::min<long long>(((long long)g->nv + 255) / 256, 2048)); }  // 256 rows per workgroup

// sum of the lengths of the rows beyond kStageCapBig entries (the task edges of the giant-row kernel), once per graph
__global__ __launch_bounds__(256) void giant_edges_kernel(int nv, const int *__restrict__ rp, unsigned long long *__restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s = 0;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const int d = rp[v + 1] - rp[v];
    if (d > kStageCapBig) s += (unsigned long long)d;
  }
  s = gm::wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}
static int giant_task_edges(gm_graph *g, unsigned long long *out) {
  const int rc = g->facts.giant_edges.ensure(g->mu, [&](unsigned long long &s) {
    return reduce_to_u64(g, g->nv > 0, "giant_edges_kernel", &s, [&](unsigned long long *d_s) { hipLaunchKernelGGL(giant_edges_kernel, rows_grid(g), dim3(256), 0, 0, g->nv, g->d_rp, d_s); });
  });
  *out = *g->facts.giant_edges;
  return rc;
}

// ---- common launch prologue / epilogue of every mining entry point (LaunchCtx, the dequeue words: gm_launch.h) ----------------------
// every solver relies on ascending rows (checked once per handle; the reference sorts on request: adj_sorted = 0)
int require_sorted_rows(gm_graph *g) {
  bool sorted = false;
  if (int rc = graph_rows_sorted(g, &sorted)) return rc;
  if (!sorted) g_last_error = "the neighbour lists of this graph are not strictly ascending: call gm_graph_sort_neighbors first (Graph::sort_neighbors, adj_sorted = 0)";
  return sorted ? GM_OK : GM_ERR_INVALID;
}

// validates the arguments, selects the device, zeroes the 64-byte counter block on the launch stream
int begin_launch(const gm_graph *cg, const gm_launch *la, const uint64_t *h_out, LaunchCtx &c) {
  if (!cg) return GM_ERR_INVALID;
  if (int rc = reject_big(cg)) return rc;
  c.g = const_cast<gm_graph *>(cg);
  c.la = launch_or_default(la);
  c.world = c.la.world > 1 ? c.la.world : 1;
  c.rank = c.la.rank;
  if (c.rank < 0 || c.rank >= c.world) return GM_ERR_INVALID;
  if (!h_out && !c.la.d_counts) return GM_ERR_INVALID;
  HIP_TRY(hipSetDevice(c.g->device));
  if (int rc = require_sorted_rows(c.g)) return rc;
  c.stream = (hipStream_t)c.la.stream;
  HIP_TRY(hipMemsetAsync(c.g->d_counters, 0, kCounterBlockBytes, c.stream));
  return GM_OK;
}

int start_timer(LaunchCtx &c) {
  c.g->ring_alias = nullptr;
  c.g->ring_extra[0] = c.g->ring_extra[1] = nullptr;
  c.evp = c.g->ev[c.g->ev_launches % gm_graph::kEvRing];
  c.g->ev_corner[c.g->ev_launches % gm_graph::kEvRing] = false;
  c.g->ev_launches++;
  HIP_TRY(hipEventRecord(c.evp[0], c.stream));
  return GM_OK;
}

// stops the timer, publishes the counters: to d_counts (device, asynchronous) and / or to h_out (synchronises)
int end_launch(LaunchCtx &c, int fin_mode, unsigned long long fin_base, uint64_t *h_out, int nout, gm_stats *st) {
  HIP_TRY(hipEventRecord(c.evp[1], c.stream));
  if (c.la.d_counts) {
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(64), 0, c.stream, fin_mode, fin_base, c.g->d_counters,
                       (unsigned long long *)c.la.d_counts);
    HIP_TRY(hipGetLastError());
    if (!h_out) return GM_OK;  // asynchronous: the caller owns the synchronisation
  }
  unsigned long long v[4], o[4];
  HIP_TRY(hipMemcpyAsync(v, c.g->d_counters, sizeof v, hipMemcpyDeviceToHost, c.stream));
  HIP_TRY(hipStreamSynchronize(c.stream));
  if (st) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c.evp[0], c.evp[1]));
    st->kernel_ms = ms;
  }
  const int n = finalize_math(fin_mode, fin_base, v, o);
  const int lim = n == 1 ? 1 : nout;  // (a single count is written whatever nout says; the lists are clipped to the caller's buffer)
  for (int i = 0; i < n && i < lim; ++i) h_out[i] = o[i];
  return GM_OK;
}

// ---- run_pattern: plan -> kernel parameters -> scratch -> launches --------------------------------------------------------------------
// What a launch of run_pattern decided (plan_pattern) and the tables it runs on.
struct PatternPlan {
  Pattern pat = PAT_TC;        // (the edge supports run as PAT_TC: the triangle pass of the task lists with another match handler)
  bool support = false, sup_part = false, wtri = false, clique = false, sym_pat = false;
  bool use_tct = false, split_stage = false, tct_long = false, use_kst = false, sup_masks = false, tc_core = false, sup_core = false;
  bool use_wide = false, use_classes = false, use_range = false;
  int target = 0, tct_stage = 0, corner_from = 0x7fffffff, cls_lo = 0;
  unsigned long long part_cap = 0;
  ChunkTable *tab = nullptr;       // the main table
  ChunkTable *tab_big = nullptr;   // task lists: the hosts with rows of 1025 .. 2048 entries (split_stage)
  ChunkTable *tab_long = nullptr;  // TC: the rows beyond the 2048-entry stage
  ChunkTable *tab_cls[4] = {nullptr, nullptr, nullptr, nullptr};  // [0] = tab, [1 .. 3] the workgroup classes
  CliquePlan *plan = nullptr;      // 4-clique, re-hosted
};

// One call of run_pattern: what its stages hand to each other.
struct PatternRun {
  PatternReq rq;                    // what the caller asked for
  LaunchCtx ctx;
  PatternPlan pl;
  MineParams p;                     // the main table's launch; the other tables' launches start from a copy
  int per_cu = 1, grid = 1;         // the main table's workgroups (gm_stats.grid)
  long long want = 0;               // ... and its dequeues
  unsigned long long my_edges = 0;  // task edges of this rank's shares (gm_stats.tasks)
  uint64_t chunks_total = 0;        // chunks of this rank's shares (gm_stats.chunks)
  bool joined[3] = {false, false, false};  // class kernels on a side stream that the launch stream has yet to wait for
#ifdef GM_DEBUG_CHUNKS
  DevOwn<unsigned long long> debug_ticks;  // what p.chunk_ticks points at
#endif
};

// which path the launch takes and the chunk tables it needs (pl.pat / support / sup_part are set by the caller)
static int plan_pattern(const LaunchCtx &c, PatternPlan &pl) {
  gm_graph *g = c.g;
  const gm_launch *la = &c.la;
  const int world = c.world, rank = c.rank;
  // tune[0] = chunk target override, tune[1] = grab, tune[2] = cost_x_step, tune[3] = cost_y_step,
  // tune[4] = blocks per CU override, tune[5] = force "search in HBM" (no LDS staging) when 1
  // default chunk size: as large as the LDS stage allows (fewer dequeues, better staging reuse) while every rank still
  // gets >= ~2 chunks per resident workgroup for the dynamic dequeue to balance (matters for strong scaling at N = 8)
  // (round 3: 4 chunks per resident workgroup for a rank of a larger job -- with ~2 the heaviest-first dequeue of a 1/8 share of the
  // LiveJournal stand-in ended 50 % above its mean, TC 1.01 ms per rank against 0.66 ideal; one rank keeps the round-2 rule)
  pl.target = kDefaultChunk;
  long long min_chunks = (world > 1 ? 4LL : 2LL) * g->cu_count * 7;
  if (const char *e = gm_sweep_env("GM_MIN_CHUNKS_PER_CU")) min_chunks = (long long)std::max(1, atoi(e)) * g->cu_count;  // (sweeps)
  while (pl.target > 128 && g->ne / ((long long)world * pl.target) < min_chunks) pl.target >>= 1;
  if (la->chunk > 0) pl.target = la->chunk;
  if (la->tune[0] > 0) pl.target = la->tune[0];
  pl.target = std::max(64, std::min(pl.target, kStageCap));
  pl.clique = pl.pat == PAT_CLIQUE4 || pl.pat == PAT_CLIQUEK;
  // tune[6] & GM_T6_EAGER_PARTS (tests): cut every chunk above 4096 estimated entries into parts
  // chunk costs are estimated keys (DAG patterns: d(u) + d(v) per edge; symmetric patterns: streamed keys, bitmap probes
  // weighted kProbeCost); parts bound the longest task of a launch
  // TC: the shorter list of every edge is streamed against the longer one (gm_tch.hip) when every DAG row fits the LDS stage
  // (tune[6] & GM_T6_TC_CHUNKED: A/B switch, the chunked kernel that streams N+(v) of every out-edge).  Its chunks host the tasks of
  // their vertices -- a hub hosts 10^5 in-edges -- so their cost is counted from the task lists and heavy chunks are cut into
  // parts of 1 M keys / world (>= 128 K): one-GPU simulation of an 8-rank share of R-MAT-22, parts of 8 M / 512 K / 128 K / 32 K keys:
  // 5.36 / 1.18 / 0.99 / 1.15 ms per rank (one GPU: 6.50 / 6.54 / 6.73 / 8.09 ms), profiles/r02/ab_tct_part_cap.log
  pl.use_tct = pl.pat == PAT_TC && !(la->tune[6] & GM_T6_TC_CHUNKED) && la->tune[5] != 1 && g->ne > 0;
  // The 2048-entry stage costs occupancy (four instead of six workgroups per CU, R-MAT-22 on it: 3.04 vs 2.57 ms), and only the few hosts with
  // rows of 1025 .. 2048 entries need it: a graph that has such rows runs TWO tables -- hosts with rows <= 1024 on the 1024-entry kernel,
  // the others on the 2048-entry one (own dequeue word).  GM_TCT_STAGE_BIG: the 2048-entry stage for every host (A/B).
  const bool stage_big_all = gm_sweep_env("GM_TCT_STAGE_BIG") != nullptr;
  pl.split_stage = pl.use_tct && g->max_deg > kStageCap && !stage_big_all && !gm_sweep_env("GM_TCT_NO_SPLIT_STAGE");
  pl.tct_stage = ((g->max_deg <= kStageCap && !stage_big_all) || pl.split_stage) ? kStageCap : kTctStageMax;
  // (rows beyond the 2048-entry stage host nothing: their out-edges are the tasks of the chunked kernel, on a table of those rows only)
  pl.tct_long = pl.use_tct && g->max_deg > kTctStageMax;
  const unsigned long long tct_part = pl.use_tct ? task_part_cap(g, world) : 0ull;
  pl.part_cap = (la->tune[6] & GM_T6_EAGER_PARTS) ? 4096ull : (stage_cap_of(pl.pat) != kStageCapWide
       ? (pl.use_tct ? tct_part : kPartCostCap)
       // a rank's share is 1/world of the launch: so is the tolerable tail (3-motif's bounded lists make its estimates
       // pessimistic already: measured, 1/8 share 84.8 ms unscaled vs 91.2 ms scaled; diamond 5.2 vs 4.2 ms)
       : (pl.pat == PAT_MOTIF3 ? kPartCostCapSym : std::max<unsigned long long>(kPartCostCapSym / (unsigned long long)world, 256ull << 10)));
  // 4-clique: vertices whose matrix exceeds the 8 KB budget go through the two-phase path (gm_mine.h)
  // (tune[6] & GM_T6_CLIQUE4_MINING: A/B switch, everything stays in the mining kernel with its arena path)
  pl.use_wide = pl.pat == PAT_CLIQUE4 && !(la->tune[6] & GM_T6_CLIQUE4_MINING);
  // symmetric-graph patterns: the rows of more than kClassRowMin entries go to the workgroup classes (gm_hrow.hip: hashed sets in LDS)
  pl.sym_pat = stage_cap_of(pl.pat) == kStageCapWide;
  // (tune[6] & GM_T6_NO_CLASSES: A/B switch, every row through the general kernel -- SPLIT chunks and dense HBM bitmaps for the long ones)
  pl.use_classes = pl.sym_pat && !(la->tune[6] & GM_T6_NO_CLASSES) && !(la->tune[5] == 1);
  // They are separate launches: one whose share of chunks cannot fill the chip runs on a side stream (below), and with that the
  // classes win or tie wherever there are long rows (profiles/r02/ab_class_threshold.log, general path vs classes, ms: diamond R-MAT-16
  // 1.68 vs 0.76, R-MAT-18 2.64 vs 2.03, power law 3.94 vs 3.68, R-MAT-22 27.9 vs 16.6, R-MAT-23 255 vs 107; 3-motif R-MAT-16 1.43 vs 0.75,
  // R-MAT-20 6.4 vs 5.7, power law 4.07 vs 4.10, R-MAT-24 458 vs 172). A graph without such rows skips their (empty) tables.
  // tune[6] & GM_T6_FORCE_CLASSES forces them on.
  if (pl.use_classes && !(la->tune[6] & GM_T6_FORCE_CLASSES)) pl.use_classes = g->max_deg > kClassRowMin;
  if (pl.support && (!pl.use_tct || (world > 1 && !pl.sup_part))) return GM_ERR_UNSUPPORTED;  // (the caller takes the per-edge kernels)
  if (pl.support && pl.tct_long) {  // the out-edges of the rows beyond the stage: sup_long_kernel, below
    if (const int rc_l = ensure_long_rows(g)) return rc_l;
  }
  // the triangle count reads the key stream + the lists of the longer tasks (ensure_keystream); the edge supports, the kernels without the
  // stream (tune[6] & GM_T6_NO_KEYSTREAM) and the handles that cannot have one read the full task lists
  if (pl.use_tct) {
    // The edge supports take the stream only where matches are RARE: a match of a streamed key costs them two gathers (the entries beside
    // the stream) and two global atomics, where a task of the lists costs one atomic per match and one per task.  Flat / power-law LJ-size
    // 1.06 / 1.55 -> 0.70 / 1.32 ms, but R-MAT-22 8.50 -> 10.95 and R-MAT-24 102 -> 115: the switch is the one that decides the renumbering
    // (sum d+^2 / |E+| below kSupStreamMaxMeanRow: short lists) -- and few triangles per edge, which short lists do not imply: on a graph
    // with LiveJournal's size AND triangle density (planted communities, 6.7 triangles per DAG entry; round 6) the stream's two atomics per
    // match made the diamond 13.4 ms where the task lists take 2.8.  The density is estimated from a sample of the entries
    // (ensure_tri_per_edge): the stream below 0.5 triangles per entry (power law: 0.1, flat: 0).  GM_SUP_STREAM=0 / 1 forces it.
    bool sup_stream = false;
    if (pl.support && !pl.wtri && !(la->tune[6] & GM_T6_NO_KEYSTREAM)) {  // (the weighted pass reads the full task lists)
      if (const char *e = gm_opt("GM_SUP_STREAM")) sup_stream = atoi(e) != 0;
      else sup_stream = ensure_mean_sq_deg(g) == GM_OK && *g->facts.mean_sq_deg < (double)kSupStreamMaxMeanRow && ensure_tri_per_edge(g) == GM_OK &&
                        *g->facts.tri_per_edge < 0.5;
    }
    if ((sup_stream || !pl.support) && !(la->tune[6] & GM_T6_NO_KEYSTREAM)) {
      if (const int rc_k = ensure_keystream(g, pl.support, &pl.use_kst, !pl.support && !pl.tct_long)) return rc_k;  // (the triangle count: the hub corner may stay out, gm_ctc.hip)
    }
    if (!pl.use_kst) {
      if (const int rc_t = ensure_tasklists(g)) return rc_t;
    }
  }
  if (pl.support && !pl.sup_part && !pl.wtri && !g->diamond.sup) HIP_TRY(g->diamond.sup.alloc(sizeof(unsigned) * (size_t)std::max<long long>(g->ne, 1)));
  // match masks instead of one atomic per streamed edge (gm_sup.hip): one GPU, the task lists, a topologically numbered DAG
  // (tune[6] & GM_T6_SUP_ATOMICS: A/B switch, every streamed edge by an atomic)
  if (pl.support && !pl.sup_part && !pl.wtri && world == 1 && pl.use_tct && !pl.use_kst && !(la->tune[6] & GM_T6_SUP_ATOMICS)) {
    if (const int rc_m = ensure_sup_masks(g)) return rc_m;
    pl.sup_masks = g->sup_masks.built();
  }
  setup_trace("run_pattern: task lists");
  // the hosts with rows of 1025 .. 2048 entries, on the 2048-entry kernel -- when a rank's share of them can fill the chip about twice: the two
  // launches follow each other on the stream, and the second waits for the first one's last chunk.  R-MAT-24 has 8.5 K such chunks with a
  // third of all keys: split / one table, ms per rank at world 1 / 2 / 4 / 8: TC 32.3 / 16.1 / 9.26 / 5.20 against 36.2 / 18.2 / 9.30 / 4.82,
  // edge supports - / 51.0 / 26.0 / 16.7 against - / 60.5 / 30.4 / 15.5 (profiles/r04/ab_split_stage.txt).  GM_TCT_SPLIT_ALWAYS: at every world.
  if (pl.split_stage) {
    RowFilter rb;
    rb.tct = (pl.use_kst && !pl.support && g->kst->skip_from < g->nv) ? 2 : 1;  // (2: priced from the stream without the hub corner, gm_tables.hip)
    rb.only_lo = kStageCap;
    rb.only_hi = kTctStageMax;
    if (const int rc_b = get_table(g, pl.target, true, 0, pl.part_cap, kTctStageMax, &pl.tab_big, rb, kBitmapMinDeg)) return rc_b;
    if ((long long)pl.tab_big->n / world < 2ll * g->cu_count * 4 && !gm_opt("GM_TCT_SPLIT_ALWAYS")) {
      pl.tab_big = nullptr;
      pl.split_stage = false;
      pl.tct_stage = kTctStageMax;
    }
  }
  // the triangles of the hub corner on the matrix cores (gm_ctc.hip): this handle's key stream holds no task of the corner's rows
  pl.corner_from = pl.use_kst ? g->kst->skip_from : (pl.use_tct ? g->tasklists->skip_from : 0x7fffffff);  // the rows the stream / the task lists in use leave out
  pl.tc_core = pl.use_tct && !pl.support && pl.corner_from < g->nv;
  pl.sup_core = pl.support && !pl.wtri && !pl.use_kst && pl.corner_from < g->nv;  // (the weighted pass walks the corner's out-edges itself)
  if (pl.sup_core) {
    if (const int rc_c = ensure_sup_corner(g)) return rc_c;
  }
  RowFilter rf;
  rf.tct = pl.use_tct ? ((pl.tc_core && pl.use_kst) ? 2 : 1) : 0;
  if (pl.tct_long) { rf.skip_lo = kTctStageMax; rf.skip_hi = 0x7fffffff; }
  if (pl.split_stage) { rf.skip_lo = kStageCap; rf.skip_hi = 0x7fffffff; }  // (this table: the hosts whose rows fit the 1024-entry stage)
  // 4-clique: the first level is re-hosted (gm_cbuild.hip) for every vertex whose row fits its stage -- the narrow chunk table and
  // the wide list live in the CliquePlan; what is left for THIS table are the rows beyond kCbMaxDeg (mine_kernel's arena path)
  if (pl.use_wide) rf.only_lo = kCbMaxDeg;
  // Rows of 1025..3072 entries fit the general kernel's stage, but their partner lists (mean 600 keys on R-MAT-24) are cheaper
  // against a hashed set than against the filter + bisection of a multi-row chunk: measured (profiles/r02/ab_hrow_class_lower_bound.log,
  // ms, lower bound 3072 / 2048 / 1024 / 512 / 256) diamond R-MAT-24 262 / 240 / 239 / 238 / 237, R-MAT-22 21.1 / 21.0 / 17.5 / 17.6 / 17.5,
  // 3-motif R-MAT-24 185 / 172 / 172 / 171 / 171.
  pl.cls_lo = kClassRowMin;
  if (const char *e = gm_sweep_env("GM_CLS_LO")) pl.cls_lo = std::max(64, atoi(e));  // (sweeps)
  // giant rows (> kStageCapBig entries): hashed sets of row pieces (giant_kernel, gm_hrow.hip) instead of SPLIT chunks probing
  // dense bitmaps in HBM (tune[6] & GM_T6_GIANT_SPLIT: A/B switch, they stay SPLIT chunks of the general kernel)
  pl.use_range = pl.use_classes && !(la->tune[6] & GM_T6_GIANT_SPLIT) && hrow_fits(g->nv, 2);  // (its pieces are class-2 sets: nv <= 2^27)
  if (pl.use_classes) { rf.skip_lo = pl.cls_lo; rf.skip_hi = pl.use_range ? 0x7fffffff : kStageCapBig; }
  if (int rc = get_table(g, pl.target, !pl.clique, pl.clique ? kBitWords : 0, pl.part_cap, pl.use_tct ? pl.tct_stage : stage_cap_of(pl.pat), &pl.tab, rf, pl.use_classes ? kStageCapBig : kBitmapMinDeg)) return rc;
  if (pl.tct_long && !pl.support) {
    RowFilter rl;
    rl.only_lo = kTctStageMax;
    if (int rc = get_table(g, pl.target, true, 0, kPartCostCap, kStageCap, &pl.tab_long, rl, kBitmapMinDeg)) return rc;
  }
  pl.tab_cls[0] = pl.tab;
  if (pl.use_classes) {
    RowFilter r1, r2;
    r1.only_lo = pl.cls_lo; r1.only_hi = kStageCapMid;
    r2.only_lo = kStageCapMid; r2.only_hi = kStageCapBig;
    // Parts of the one-row chunks: coarse. Measured on MI355X (profiles/r02/ab_sym_classes.log, diamond / 3-motif R-MAT-24, ms):
    // whole rows (largest chunk 6e7 estimated keys) 636 / 370; parts of 512 K keys 1277 / 765 (16-wave workgroups with ~10
    // batches per part); 512 K keys with >= 64 batches per part and 4-edge batches 743 / 462 -- every batch pays a few
    // dependent global round trips (descriptors, the bounded prefix of 3-motif) before it streams, so small batches and
    // small parts lose more than the shorter tail wins (8 M keys 368 / 634, 32 M keys 363 / 627). Parts of 32 M keys only trim the
    // few heaviest rows. Side streams for the class kernels: 396 / 667 (GM_CLASSES_STREAMS, off).
    // (hashed sets: a part costs one table build, ~10 us. A rank's share is 1/world of the launch and so is the tolerable tail -- one-GPU
    // simulation of 8 rank shares, parts of 32 M / 8 M / 2 M keys: 3-motif R-MAT-24 28.2 / 25.8 / 26.5 ms per rank, diamond R-MAT-22 8.3 / 6.4 / 5.4;
    // on one GPU the same parts cost 171 / 173 / 181 and 17.5 / 18.3 / 18.4 ms: profiles/r02/ab_class_part_cap.log)
    unsigned long long cls_cap = (la->tune[6] & GM_T6_EAGER_PARTS) ? 4096ull
                                 : std::max<unsigned long long>(pl.part_cap, std::max<unsigned long long>((32ull << 20) / (unsigned long long)std::max(world, 1), 2ull << 20));
    if (const char *e = gm_sweep_env("GM_CLS_CAP_MKEYS")) cls_cap = (unsigned long long)std::max(1, atoi(e)) << 20;  // (sweeps)
    if (const char *e = gm_sweep_env("GM_CLS_CAP_KKEYS")) cls_cap = (unsigned long long)std::max(16, atoi(e)) << 10;
    // (target 1: every row is a chunk of its own -- the class kernels take one-row chunks -- also below the general kernel's chunk target)
    if (int rc = get_table(g, 1, false, 0, cls_cap, kStageCapMid, &pl.tab_cls[1], r1, 0x7fffffff)) return rc;
    if (int rc = get_table(g, 1, false, 0, cls_cap, kStageCapBig, &pl.tab_cls[2], r2, 0x7fffffff)) return rc;
    if (pl.use_range) {  // pieces of <= kGiantEdges task edges, never cut into parts (part_cap 0: giant_kernel ignores part / nparts)
      RowFilter r3;
      r3.only_lo = kStageCapBig;
      // A chunk is the unit of the dequeue and costs its whole row's set builds (~20 us per piece of 24576 entries): as large as
      // kGiantEdges where there are many, smaller where the giant rows of the graph (or of a rank's share) would otherwise be a
      // handful of chunks -- the LiveJournal stand-in has ~40 chunks of 8192 edges, 3.9 ms each: the whole launch of a 1/8 share
      // waited for ONE of them (1.9 ms ideal). Aim at 4 chunks per resident workgroup and rank.
      int gtarget = kGiantEdges;
      {
        unsigned long long ge = 0;
        if (int rc = giant_task_edges(g, &ge)) return rc;
        const unsigned long long per = ge / ((unsigned long long)g->cu_count * (unsigned long long)giant_per_cu() * 4ull * (unsigned long long)world);
        gtarget = (int)std::max<unsigned long long>(512, std::min<unsigned long long>((unsigned long long)kGiantEdges, per));
        gtarget = (gtarget + 63) & ~63;
        if (const char *e = gm_sweep_env("GM_GIANT_TARGET")) gtarget = std::max(64, std::min(atoi(e), kGiantEdges));  // (sweeps)
      }
      if (int rc = get_table(g, gtarget, true, 0, 0ull, kStageCapBig, &pl.tab_cls[3], r3, 0x7fffffff)) return rc;
    }
  }
  if (pl.use_wide) {
    if (int rc = get_clique_plan(g, rank, world, la->policy, pl.target, pl.part_cap, &pl.plan)) return rc;
  }
  return GM_OK;
}

// this rank's share of a table: chunk ids first + i*step of the dequeue order (or a contiguous / vertex range); its task edges go to r.my_edges
static int take_share(PatternRun &r, ChunkTable *tb, MineParams &q) {
  gm_graph *g = r.ctx.g;
  const gm_launch *la = &r.ctx.la;
  const PatternPlan &pl = r.pl;
  const int world = r.ctx.world, rank = r.ctx.rank;
  q.chunks = tb->d;
  q.chunk_slot = tb->d_slot;
  q.bitmaps = tb->d_bitmaps;
  q.bitmap_words = tb->bitmap_words;
  q.row_slot = tb->d_row_slot;
  const long long n = (long long)tb->n;
  long long first = 0, step = 1, count = 0;
  // dequeue order (tune[6] & GM_T6_CHUNK_ID_ORDER: plain chunk-id order; & GM_T6_SWAP_ORDERS: swap the two orders -- ablation only)
  // measured on R-MAT (one rank): the cliques want the full cost order (4-clique 220.6 -> 208.6 ms, 5-clique 796 -> 589 ms),
  // the symmetric-graph patterns the locality-preserving heavy-first order at every world size, TC heavy-first for one
  // rank and the full order for shares
  const bool clique_pat = pl.pat == PAT_CLIQUE4 || pl.pat == PAT_CLIQUEK;
  const int which = (((world > 1 && !pl.sym_pat) || clique_pat) ? 1 : 0) ^ ((la->tune[6] & GM_T6_SWAP_ORDERS) ? 1 : 0);
  const bool lpt = la->policy == GM_PART_ROUND_ROBIN && tb->d_order[which] && !(la->tune[6] & GM_T6_CHUNK_ID_ORDER);
  q.order = lpt ? tb->d_order[which] : nullptr;
  if (world > 1 && la->policy != GM_PART_VERTEX && tb->d_edges) {
    // a rank of a larger job: its records as a list of their own -- every part of a chunk with the same rank (ShareOrder, gm_host.h)
    const ShareOrder *so = nullptr;
    if (int rcs = get_share_order(g, tb, world, rank, la->policy, lpt ? which : -1, &so)) return rcs;
    q.first = 0;
    q.step = 1;
    q.count = (int)so->n;
    q.order = so->d;
    r.my_edges += so->edges;
    return GM_OK;
  }
  if (la->policy == GM_PART_VERTEX) {  // contiguous chunk range whose first vertex lies in this rank's vertex range
    if (int rcv = table_host_views(g, tb)) return rcv;
    chunk_range_of_vertex_share(tb, g->nv, rank, world, &first, &count);
  } else {
    gm_partition((int64_t)n, rank, world, la->policy, (int64_t *)&first, (int64_t *)&step, (int64_t *)&count);
  }
  q.first = (int)first;
  q.step = (int)step;
  q.count = (int)count;
  // task edges of the share (gm_stats): the whole table's total came with the table; a share reads the per-chunk host views
  if (first == 0 && step == 1 && count == n) { r.my_edges += tb->total_edges; return GM_OK; }
  if (int rcv = table_host_views(g, tb)) return rcv;
  if (step == 1) r.my_edges += tb->edge_prefix[first + count] - tb->edge_prefix[first];  // (any order: the same set)
  else for (long long j = first; j < n; j += step) {
    const size_t c = lpt ? (size_t)tb->order[which][(size_t)j] : (size_t)j;
    r.my_edges += tb->edge_prefix[c + 1] - tb->edge_prefix[c];
  }
  return GM_OK;
}

// the kernel parameters of the main table's launch: the graph and its task lists, this rank's share, the tuning words
static int fill_mine_params(PatternRun &r, int k) {
  gm_graph *g = r.ctx.g;
  const gm_launch *la = &r.ctx.la;
  const PatternPlan &pl = r.pl;
  MineParams &p = r.p;
  memset(&p, 0, sizeof p);
  p.g = graph_view(g);
  if (int rc = ensure_edesc(g)) return rc;  // (the kernels read them unconditionally; -DGM_EDESC=0 builds gather rp[v] instead, for A/B runs)
  p.g.edesc = *g->edesc;
  if (pl.use_tct) {
    const TaskLists &tl = *g->tasklists;
    const KeyStream &ks = *g->kst;
    p.g.trp = tl.trp;
    p.g.tdesc = tl.tdesc;
    p.g.tedge = pl.support ? tl.tedge.get() : nullptr;
    if (pl.sup_masks) {
      p.g.tmoff = g->sup_masks->tmoff;
      p.smask = g->sup_masks->smask;
    }
    // the triangle count streams the short lists from their task-major copies (gm_host.h TaskLists::colk; tune[6] & GM_T6_NO_KEYSTREAM: from their rows);
    // the edge supports need the entries of the streamed keys in col[] itself
    if (pl.use_kst && pl.support) {  // ... with the entries the supports need beside them (the second set when the stream was built without)
      const KeyEntries &k2 = *g->kst_entries;
      p.g.kst = k2.kst2 ? k2.kst2 : ks.kst;
      p.g.kst_rp = ks.rp;
      p.g.kst_et = k2.kst_et ? k2.kst_et : ks.kst_et;
      p.g.trp = ks.trpl;
      p.g.tdesc = k2.tdescl2 ? k2.tdescl2 : ks.tdescl;
      p.g.tedge = k2.tedgel ? k2.tedgel : ks.tedgel;
    } else if (pl.use_kst) {  // short lists as one tagged key stream, the longer ones as tasks
      p.g.kst = ks.kst;
      p.g.kst_rp = ks.rp;
      p.g.trp = ks.trpl;
      p.g.tdesc = ks.tdescl;
    } else if (!pl.support && tl.colk && tl.tdesck && !(la->tune[6] & GM_T6_NO_KEYSTREAM)) {
      p.g.col = tl.colk;
      p.g.col_entries = (long long)g->ne + (long long)tl.n_copy_keys;  // (the descriptors of the copies point behind ne)
      p.g.tdesc = tl.tdesck;
    }
  }
  if (int rc = take_share(r, pl.tab, p)) return rc;
  p.grab = la->tune[1] > 0 ? la->tune[1] : 1;
  // the task-list kernels take TWO chunks per dequeue where a resident workgroup has many to take (one device atomic + one workgroup
  // barrier less per chunk: flat LJ-size TC 0.605 -> 0.427 ms, power law 0.77 -> 0.71, R-MAT-22 2.57 -> 2.48; four: 0.423 / 0.71 / 3.37 --
  // the heavy chunks at the head of the queue then pair up, profiles/r04/ab_tc_grab.txt)
  // (not the edge supports: their launch time is the atomics', and a rank's share loses -- diamond R-MAT-22 at 2 / 4 ranks 6.06 / 4.79 ms with two
  // chunks per dequeue against 4.44 / 3.13 with one)
  if (la->tune[1] <= 0 && pl.use_tct && !pl.support && p.count >= 8ll * (long long)g->cu_count * (long long)(pl.tct_stage <= kStageCap ? 6 : 4)) p.grab = 2;
  // direction rule: X if b*(xb + xs*lg a) <= a*(yb + ys*lg b); tune[2] = xs+1, tune[3] = ys+1, tune[7] = xb*16 + yb
  p.cost_x_step = la->tune[2] > 0 ? la->tune[2] - 1 : 1;
  p.cost_y_step = la->tune[3] > 0 ? la->tune[3] - 1 : 6;
  p.cost_x_base = (la->tune[7] & 255) > 0 ? ((la->tune[7] >> 4) & 15) : 2;
  p.cost_y_base = (la->tune[7] & 255) > 0 ? (la->tune[7] & 15) : 2;
  p.cost_y_bitmap = la->tune[7] >> 8;  // 0 = price pass Y as a bisection even when row v has a bitmap
  p.k = k;
  p.flags = (la->tune[5] == 1) ? 1 : 0;
  p.flags |= (la->tune[6] & GM_T6_KERNEL_FLAGS_MASK) << 1;  // debug/ablation: bit1 skip clique phase 2, bit2 skip bit-matrix writes (counts wrong)
  if (la->tune[6] & GM_T6_HROW_MUL32) p.flags |= 1 << 23;  // hashed-row classes: the 32-bit multiply of id spaces beyond 2^24 (tests)
  if (la->tune[6] & GM_T6_HSET_FALLBACK) p.flags |= 1 << 22;  // hashed-row classes: every lookup through the global-memory fallback (tests)
  if (la->tune[6] & GM_T6_KCLIQUE_ANY_WIDTH) p.flags |= 1 << 20;  // k >= 5: the any-width pair count instead of the tile walk (tests)
  p.counters = g->d_counters;
  p.queue = queue_word(g, QW_MAIN);
  return GM_OK;
}

// what the launches may allocate, before the timer starts: the main table's grid and the cliques' arena, the giant-row scratch, the side streams
// of the 4-clique A/B switch
static int prepare_scratch(PatternRun &r, int k) {
  gm_graph *g = r.ctx.g;
  const gm_launch *la = &r.ctx.la;
  const PatternPlan &pl = r.pl;
  MineParams &p = r.p;
  const size_t lds = mine_lds_bytes(pl.pat);
  r.per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds));
  if (la->tune[4] > 0) r.per_cu = la->tune[4];
  r.want = ((long long)p.count + (long long)p.grab - 1) / (long long)p.grab;
  r.grid = grid_for(r.want, g->cu_count, r.per_cu);
  if (pl.clique && pl.tab->max_bit_words > 0) {
    // one arena slot per workgroup; k >= 5 doubles it (second half: compacted sub-matrices, cliquek_count_sub)
    // k >= 5: k - 2 slots of max_bit_words + 4096 words (the vertex's matrix + one compacted sub-matrix per deeper level; the
    // margin covers the padding of compacted rows to 64 columns)
    const unsigned long long region = pl.tab->max_bit_words + 4096ull;
    const int plist = (g->max_deg + 64) & ~63;  // (rows beyond 4096 columns keep their position lists here: cliquek_count_sub_any)
    const unsigned long long slot_words = (pl.pat == PAT_CLIQUEK) ? (unsigned long long)(k - 2) * (region + (unsigned long long)plist) : pl.tab->max_bit_words;
    p.scratch_region = region;
    p.scratch_plist = plist;
    {  // a slot per workgroup: with very long rows fewer workgroups, so that the arena stays within half of the free memory
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      const unsigned long long budget = (unsigned long long)(free_b + g->scratch.bytes) / 2ull;
      const unsigned long long fit = budget / std::max<unsigned long long>(slot_words * sizeof(unsigned), 1ull);
      if (fit == 0) {
        g_last_error = "k-clique: the bit-matrix of the longest DAG row (" + std::to_string(g->max_deg) + " entries) does not fit the device memory";
        return GM_ERR_TOO_LARGE;
      }
      if ((unsigned long long)r.grid > fit) r.grid = (int)fit;
    }
    const size_t need = (size_t)slot_words * sizeof(unsigned) * (size_t)r.grid;
    if (int rc = ensure_scratch(g, need)) return rc;
    p.scratch = g->scratch.p;
    p.scratch_words = slot_words;
  }
  // (a side stream is a hardware queue: ~17 ms each to create -- GM_SETUP_TRACE, the first 4-clique call spent 35 ms here for a variant that is off)
  if (pl.use_wide && pl.plan && pl.plan->core_base >= 0 && gm_sweep_env("GM_CLIQUE_SIDE_STREAM")) {  // (4-clique A/B: the gathered build beside the streamed one, below)
    for (int i = 0; i < 2; ++i) {
      if (!g->aux_stream[i]) {
        HIP_TRY(hipStreamCreateWithFlags(&g->aux_stream[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&g->aux_done[i], hipEventDisableTiming));
      }
    }
  }
  if (pl.use_classes) {
    // what the class launches may allocate, before the timer starts: the giant-row kernel's scratch -- per workgroup, where the pieces of
    // the row cut the partner lists of its chunk, kGiantEdges ints per piece (giant_bounds).  (The side streams are created by the first
    // launch that sends a class to one -- a class whose chunks cannot fill the chip: small graphs, shares of a rank -- and that launch's
    // time then includes it; creating all three up front cost every first call ~50 ms.)
    if (pl.tab_cls[3] && pl.tab_cls[3]->n > 0) {
      if (int rc = ensure_scratch(g, (size_t)giant_scratch_words(g->max_deg) * sizeof(unsigned) * (size_t)g->cu_count * (size_t)giant_per_cu())) return rc;
    }
  }
  return GM_OK;
}

#ifdef GM_DEBUG_CHUNKS
// diagnostics: wall_clock64 ticks per dequeue position of the main table, dumped after the launch
static int debug_chunks_begin(PatternRun &r) {
  ChunkTable *tab = r.pl.tab;
  HIP_TRY(r.debug_ticks.alloc(sizeof(unsigned long long) * std::max<size_t>(tab->n, 1)));
  HIP_TRY(hipMemset(r.debug_ticks, 0, sizeof(unsigned long long) * std::max<size_t>(tab->n, 1)));
  r.p.chunk_ticks = r.debug_ticks;
  return GM_OK;
}
static int debug_chunks_dump(PatternRun &run) {
  gm_graph *g = run.ctx.g;
  hipStream_t stream = run.ctx.stream;
  ChunkTable *tab = run.pl.tab;
  const MineParams &p = run.p;
  const Pattern pat = run.pl.pat;
  unsigned long long *d_ticks = p.chunk_ticks;
  HIP_TRY(hipStreamSynchronize(stream));
  std::vector<unsigned long long> ticks(tab->n);
  HIP_TRY(hipMemcpy(ticks.data(), d_ticks, sizeof(unsigned long long) * tab->n, hipMemcpyDeviceToHost));
  run.debug_ticks.reset();
  std::vector<ChunkRec> recs(tab->n);
  HIP_TRY(hipMemcpy(recs.data(), tab->d, sizeof(ChunkRec) * tab->n, hipMemcpyDeviceToHost));
  if (int rcv = table_host_views(g, tab)) return rcv;
  const std::vector<int> *h_rp_p = nullptr;
  if (int rcv = host_rp(g, &h_rp_p)) return rcv;
  const std::vector<int> &h_rp = *h_rp_p;
  std::vector<size_t> idx(tab->n);
  for (size_t i = 0; i < tab->n; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return ticks[a] > ticks[b]; });
  unsigned long long tot = 0;
  for (auto t : ticks) tot += t;
  if (const char *dump = gm_sweep_env("GM_CHUNK_DUMP")) {
    static int dump_no = 0;
    const std::string name = std::string(dump) + "." + std::to_string(dump_no++) + ".pat" + std::to_string((int)pat);
    FILE *f = fopen(name.c_str(), "w");
    if (f) {
      fprintf(f, "pos,cid,rows,entries,rowlen,whole,part,nparts,cost,us\n");
      for (size_t pos = 0; pos < tab->n; ++pos) {
        const size_t cid = p.order ? (size_t)(p.order == tab->d_order[0] ? tab->order[0][pos] : tab->order[1][pos]) : pos;
        const ChunkRec &r = recs[cid];
        const bool whole = r.e_begin == h_rp[r.u_begin] && r.e_end == h_rp[r.u_end];
        fprintf(f, "%zu,%zu,%d,%d,%d,%d,%d,%d,%llu,%.1f\n", pos, cid, r.u_end - r.u_begin, r.e_end - r.e_begin,
                h_rp[r.u_begin + 1] - h_rp[r.u_begin], (int)whole, r.part, r.nparts, tab->cost[cid], ticks[pos] / 100.0);
      }
      fclose(f);
    }
  }
  fprintf(stderr, "[chunks] n=%zu total ticks %llu (100 MHz): mean %.1f us\n", tab->n, tot, tot / 100.0 / std::max<size_t>(tab->n, 1));
  for (size_t k = 0; k < std::min<size_t>(12, tab->n); ++k) {
    const size_t pos = idx[k];
    const size_t cid = p.order ? (size_t)(p.order == tab->d_order[0] ? tab->order[0][pos] : tab->order[1][pos]) : pos;
    const ChunkRec &r = recs[cid];
    fprintf(stderr, "[chunks] #%zu pos %zu: %.1f us  rows [%d,%d) entries [%d,%d) n=%d part %d/%d rowlen %d\n", k, pos, ticks[pos] / 100.0,
            r.u_begin, r.u_end, r.e_begin, r.e_end, r.e_end - r.e_begin, r.part, r.nparts, h_rp[r.u_begin + 1] - h_rp[r.u_begin]);
  }
  return GM_OK;
}
#endif

// 4-clique, re-hosted: per arena round, (1) cbuild_kernel over the round's host chunks builds every row of every owner's matrix,
// (2) clique_small_kernel counts the matrices of the narrow chunks, the big-LDS classes X / L / S those of the wide vertices
static int launch_clique4_rounds(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  const gm_launch *la = &r.ctx.la;
  hipStream_t stream = r.ctx.stream;
  CliquePlan *plan = r.pl.plan;
  const MineParams &p = r.p;
  {  // task edges of the share: the entries of its narrow chunks + the rows of its wide vertices
    ChunkTable *tn = plan->tabN;
    if (plan->n_count == (long long)tn->n) {
      r.my_edges += tn->total_edges;
    } else {
      if (int rc = table_host_views(g, tn)) return rc;
    }
    for (long long i = 0; i < plan->n_count && plan->n_count != (long long)tn->n; ++i) {
      const long long pos = plan->n_first + i * plan->n_step;
      const size_t c = plan->d_order ? (size_t)tn->order[plan->order_which][(size_t)pos] : (size_t)pos;
      r.my_edges += tn->edge_prefix[c + 1] - tn->edge_prefix[c];
    }
    r.my_edges += plan->wide_edges;
  }
  HIP_TRY(hipMemsetAsync(g->arena.queue, 0, 65536, stream));
  setup_trace("launch: clique prologue");
  const bool prof = gm_sweep_env("GM_WIDE_PROFILE") != nullptr;
  int qword = 0;
  for (const auto &rd : plan->rounds) {
    if (qword + 9 > 16384) return GM_ERR_TOO_LARGE;  // (more than ~3000 arena rounds)
    bool gather_joined = false;
    // the rows of the wide vertices whose first endpoint lies in the hub core: gathered (gm_cgather.hip) -- by blocks of core rows resident in
    // LDS where the plan lists the round's (vertex, block) units (round 6), row by row from the bitmap otherwise (tune[6] & GM_T6_CLIQUE4_ROW_GATHER: on request)
    const bool blocked = plan->core_base >= 0 && rd.w1 > rd.w0 && rd.d_gunits != nullptr && rd.n_gitems > 0 && !(la->tune[6] & GM_T6_CLIQUE4_ROW_GATHER);
    if (blocked) {
      CGatherBParams cb;
      memset(&cb, 0, sizeof cb);
      cb.mat = g->arena.mat;
      cb.tri = g->core_blocks->tri;
      cb.rowbase = g->core_blocks->rowbase;
      cb.blk = g->core_blocks->blk;
      cb.tab = rd.d_gtab;
      cb.units = rd.d_gunits;
      cb.items = rd.d_gitems;
      cb.delta = g->core->base & 31;
      cb.count = (int)rd.n_gitems;
      cb.queue = g->arena.queue + qword++;
      const int ggrid = grid_for(cb.count, g->cu_count, cgatherb_per_cu());
      HIP_TRY(launch_cgatherb(cb, ggrid, stream));
      setup_trace("launch: core gather (blocked)");
    } else if (plan->core_base >= 0 && rd.w1 > rd.w0) {
      CGatherParams cg;
      memset(&cg, 0, sizeof cg);
      cg.rp = g->d_rp;
      cg.col = g->d_col;
      cg.verts = plan->d_verts;
      cg.base = plan->d_slot_base;
      cg.mat = g->arena.mat;
      cg.core = g->core->bits;
      cg.core_base = g->core->base;
      cg.core_words = (g->core->h + 31) / 32;
      cg.core_bytes = (unsigned long long)g->core->h * (unsigned long long)cg.core_words * 4ull;
      cg.first_slot = (int)rd.w0;
      cg.count = (int)(rd.w1 - rd.w0);
      cg.queue = g->arena.queue + qword++;
      const int ggrid = grid_for(cg.count, g->cu_count, cgather_per_cu());
      // (GM_CLIQUE_SIDE_STREAM=1: on a side stream beside the streamed build and the counts of the narrow vertices -- they touch other rows
      // of the arena.  Measured and not taken: the gathers want all 32 waves of a CU -- 4 / 3 / 2 / 1 workgroups per CU beside the streamed
      // build: 29.2 / 29.5 / 33.8 / 53.4 ms against 27.7 one after the other, profiles/r04/ab_clique4_side_stream.txt)
      const bool side = gm_sweep_env("GM_CLIQUE_SIDE_STREAM") != nullptr;
      hipStream_t gs = side ? g->aux_stream[0] : stream;
      if (side) {
        HIP_TRY(hipEventRecord(g->aux_done[1], stream));  // after the queue words were zeroed / the previous round's counts read the arena
        HIP_TRY(hipStreamWaitEvent(gs, g->aux_done[1], 0));
      }
      HIP_TRY(launch_cgather(cg, ggrid, gs));
      setup_trace("launch: core gather");
      if (side) {
        HIP_TRY(hipEventRecord(g->aux_done[0], gs));
        gather_joined = true;
      }
    }
    if (rd.n_tasks > 0) {
      CBuildParams pw;
      memset(&pw, 0, sizeof pw);
      pw.g = p.g;
      pw.chunks = rd.host_tab.d;
      pw.order = rd.host_tab.d_order[1];  // heaviest host chunks first
      // (a chunk of hosts without a task of this rank's owners has cost 0 and sits at the end of the cost order: not dequeued at all --
      // a rank of eight found its 7 M tasks in 97.5 K chunks, most of them empty for it)
      pw.count = (int)std::min(rd.host_tab.n, rd.host_tab.n_with_cost);
      pw.trp = rd.d_trp;
      pw.tasks = rd.d_tasks;
      pw.queue = g->arena.queue + qword++;
      pw.mat = g->arena.mat;
      pw.flags = p.flags;
      const int bgrid = grid_for(pw.count, g->cu_count, cbuild_per_cu(plan->stage));
      if (pw.count > 0) HIP_TRY(launch_cbuild(pw, plan->stage, bgrid, stream));
      setup_trace("launch: streamed build");
      r.chunks_total += (uint64_t)pw.count;
    }
    if (rd.n_count > 0) {
      CliqueSmallParams cs;
      memset(&cs, 0, sizeof cs);
      cs.rp = g->d_rp;
      cs.chunks = plan->tabN->d;
      cs.order = plan->d_order;
      cs.first = (int)(plan->n_first + rd.n_pos0 * plan->n_step);
      cs.step = (int)plan->n_step;
      cs.count = (int)rd.n_count;
      cs.base = rd.d_base;
      cs.mat = g->arena.mat;
      cs.queue = g->arena.queue + qword++;
      cs.counters = g->d_counters;
      cs.topo = plan->topo ? 1 : 0;
      const int sgrid = grid_for(cs.count, g->cu_count, 8);
      HIP_TRY(launch_clique_small(cs, sgrid, stream));
      setup_trace("launch: narrow counts");
      r.chunks_total += (uint64_t)rd.n_count;
    }
    if (gather_joined) HIP_TRY(hipStreamWaitEvent(stream, g->aux_done[0], 0));  // the wide vertices' rows are complete
    // pair counts of the wide vertices on the matrix cores (gm_cmma.hip)
    for (int cls = 2; cls >= 0; --cls) {  // the column blocks and the one-per-CU workgroups before the small ones
      CliqueCountParams c;
      memset(&c, 0, sizeof c);
      c.rp = g->d_rp;
      c.verts = plan->d_verts;
      c.base = plan->d_slot_base;
      c.mat = g->arena.mat;
      c.slots = plan->d_mcls_slots + rd.mcls_begin[cls];
      c.qrec = plan->d_mcls_rec + rd.mcls_begin[cls];
      c.count = (int)(rd.mcls_begin[cls + 1] - rd.mcls_begin[cls]);
      c.queue = g->arena.queue + qword++;
      c.counters = g->d_counters;
      c.topo = plan->topo ? 1 : 0;
      if (c.count == 0) continue;
      const int per_cu_c = (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / clique_mma_lds_bytes(cls), (size_t)(2048 / clique_mma_threads(cls))));
      const int cgrid = grid_for((long long)c.count * (cls == 2 ? 8 : 1), g->cu_count, per_cu_c);
      HIP_TRY(launch_clique_mma(cls, c, cgrid, stream));
      setup_trace("launch: matrix-core counts");
    }
  }
  if (prof) {
    HIP_TRY(hipStreamSynchronize(stream));
    size_t nt = 0, nh = 0;
    for (const auto &rd : plan->rounds) { nt += rd.n_tasks; nh += rd.host_tab.n; }
    fprintf(stderr, "[clique plan] %zu wide vertices, %lld narrow chunks, %zu tasks in %zu host chunks, %zu round(s), arena %.1f MB, stage %d, %s numbering\n",
            plan->verts.size(), plan->n_count, nt, nh, plan->rounds.size(), g->arena.mat_bytes / 1048576.0, plan->stage, plan->topo ? "topological" : "arbitrary");
  }
  return GM_OK;
}

// the workgroup classes of the symmetric-graph patterns: class 3 (giant rows), then 2, then 1, each on its own dequeue word
static int launch_classes(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  const gm_launch *la = &r.ctx.la;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  const MineParams &p = r.p;
  // A class kernel whose share of chunks cannot fill the chip on its own (small graphs, 1/8 shares) runs on a side stream, so
  // that the kernels launched after it fill the idle CUs; one that can fill it stays on the launch's stream -- there every
  // kernel has the chip to itself (side streams at R-MAT-24 size: diamond 667 vs 636 ms, the 148 KB workgroups of class 2 wait
  // for whole CUs to drain). GM_CLASSES_STREAMS=0 / 1 forces one or the other.
  const char *streams_env = gm_sweep_env("GM_CLASSES_STREAMS");
  auto side_stream = [&](int cls, long long count, long long full_grid, hipStream_t *ws) -> int {
    *ws = stream;
    const bool side = streams_env ? atoi(streams_env) != 0 : count < full_grid;
    if (!side) return GM_OK;
    if (!g->aux_stream[cls - 1]) {
      HIP_TRY(hipStreamCreateWithFlags(&g->aux_stream[cls - 1], hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&g->aux_done[cls - 1], hipEventDisableTiming));
    }
    *ws = g->aux_stream[cls - 1];
    HIP_TRY(hipStreamWaitEvent(*ws, r.ctx.evp[0], 0));  // after the counters were zeroed and the timer started
    return GM_OK;
  };
  auto side_done = [&](int cls, hipStream_t ws) -> int {
    if (ws == stream) return GM_OK;
    HIP_TRY(hipEventRecord(g->aux_done[cls - 1], ws));
    r.joined[cls - 1] = true;
    return GM_OK;
  };
  for (int cls = 3; cls >= 1; --cls) {
    if (!pl.tab_cls[cls]) continue;
    MineParams q = p;
    if (int rc = take_share(r, pl.tab_cls[cls], q)) return rc;
    q.queue = queue_word(g, QW_CLASS1 + (cls - 1));  // its own dequeue word inside the zeroed 64-byte block
    if (q.count == 0) continue;
    r.chunks_total += (uint64_t)q.count;
    // the row as a hashed set in LDS (gm_hrow.hip) unless the ids are too wide for its 14-bit remainders
    // (tune[6] & GM_T6_CLASSES_SORTED_COPY: A/B switch, the sorted LDS copy + bit filter + bisection of gm_mine_wide.hip)
    const bool giant = cls == 3;
    const bool hrow = !giant && !(la->tune[6] & GM_T6_CLASSES_SORTED_COPY) && p.g.edesc != nullptr && hrow_fits(g->nv, cls);
    const int per_cu_w = giant ? giant_per_cu() : hrow ? hrow_per_cu(cls) : (int)std::max<size_t>(1, (160 * 1024) / mine_wide_lds_bytes(cls));
    const int wgrid = grid_for(q.count, g->cu_count, per_cu_w);
    if (giant) {
      q.scratch = g->scratch.p;  // (allocated before the timer started)
      q.scratch_words = giant_scratch_words(g->max_deg);
    }
    hipStream_t ws;
    if (int rc = side_stream(cls, q.count, (long long)g->cu_count * per_cu_w, &ws)) return rc;
    if (giant) HIP_TRY(launch_giant(pl.pat, q, wgrid, ws));
    else if (hrow) HIP_TRY(launch_hrow(pl.pat, cls, q, wgrid, ws));
    else HIP_TRY(launch_mine_wide(pl.pat, cls, q, wgrid, ws));
    if (int rc = side_done(cls, ws)) return rc;
  }
  return GM_OK;
}

// The tables of the task-list kernels, one after the other on the launch stream.  support: the edge supports' kernel (launch_sup / sup_per_cu,
// gm_sup.hip) instead of the triangle count's (launch_tch / tch_per_cu, gm_tch.hip).
enum TaskKernel : int { TK_TC = 0, TK_SUPPORT = 1, TK_WTRI = 2, TK_CREDIT = 3 };
static int launch_task_tables(PatternRun &r, int kind) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  const MineParams &p = r.p;
  const WtriParams wp = {g->w5.sup, g->w5.ed, g->w5deg->deg};
  const CreditParams crp = {r.rq.credit_sup, r.rq.credit_w};
  auto launch = [&](const MineParams &q, int stage, long long dequeues) {
    if (kind == TK_CREDIT) return launch_credit(q, crp, stage, grid_for(dequeues, g->cu_count, credit_per_cu(stage)), stream);
    const int grid = grid_for(dequeues, g->cu_count, kind == TK_WTRI ? wtri_per_cu(stage) : kind == TK_SUPPORT ? sup_per_cu(stage) : tch_per_cu(stage));
    return kind == TK_WTRI ? launch_wtri(q, wp, stage, grid, stream) : kind == TK_SUPPORT ? launch_sup(q, stage, grid, stream) : launch_tch(q, stage, grid, stream);
  };
  if (pl.tab_big) {  // the hosts with rows of 1025 .. 2048 entries first (the heaviest tasks), on the 2048-entry kernel
    MineParams q = p;
    if (int rc = take_share(r, pl.tab_big, q)) return rc;
    q.grab = 1;
    q.queue = queue_word(g, QW_STAGE_BIG);
    r.chunks_total += (uint64_t)q.count;
    if (q.count > 0) HIP_TRY(launch(q, kTctStageMax, q.count));
  }
  if (p.count > 0) HIP_TRY(launch(p, pl.tct_stage, r.want));
  return GM_OK;
}

// The hub corner of a launch on the matrix cores (gm_ctc.hip), bracketed by evp[2] / evp[3] (gm_corner_times); a rank takes every world-th
// block.  support: the supports of the corner's edges (launch_core_sup) instead of its triangles (launch_core_tc).
static int launch_corner(PatternRun &r, CoreTcParams cp, bool support) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  cp.first = r.ctx.rank;
  cp.step = r.ctx.world;
  cp.queue = queue_word(g, QW_CORNER);  // (its own dequeue word inside the zeroed 64-byte block)
  cp.counters = g->d_counters;
  HIP_TRY(hipEventRecord(r.ctx.evp[2], stream));
  HIP_TRY(support ? launch_core_sup(cp, g->cu_count, stream) : launch_core_tc(cp, g->cu_count, stream));
  HIP_TRY(hipEventRecord(r.ctx.evp[3], stream));
  g->ev_corner[(g->ev_launches - 1) % gm_graph::kEvRing] = true;
  return GM_OK;
}

// TC through the task lists: the long-row table, the big-stage table, the main table, the hub corner
static int launch_tc(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  const MineParams &p = r.p;
  if (pl.tab_long) {  // TC: the out-edges of the rows beyond the stage, through the chunked kernel (own dequeue word)
    MineParams q = p;
    if (int rc = take_share(r, pl.tab_long, q)) return rc;
    q.g.trp = nullptr;
    q.g.tdesc = nullptr;
    q.queue = queue_word(g, QW_TC_LONG);
    if (q.count > 0) {
      r.chunks_total += (uint64_t)q.count;
      const long long wq = ((long long)q.count + (long long)q.grab - 1) / (long long)q.grab;
      HIP_TRY(launch_mine(pl.pat, q, grid_for(wq, g->cu_count, r.per_cu), stream));
    }
  }
  if (int rc = launch_task_tables(r, TK_TC)) return rc;
  if (pl.tc_core) {  // the out-edges of the hub corner: one masked bit-matrix product; a rank takes every world-th block
    CoreTcParams cp;
    memset(&cp, 0, sizeof cp);
    cp.core = g->core->bits;
    cp.row_words = (g->core->h + 31) / 32;
    // (a stream built with a choice of block pairs, tc_pairs_setup: the region they lie in and the list of their pieces)
    const bool pairs = pl.use_kst && g->kst->pair_region > 0;
    const int from = pairs ? g->kst->pair_from : pl.corner_from;
    cp.row0 = from - g->core->base;
    cp.word0 = cp.row0 >> 5;
    cp.h = g->nv - from;
    cp.ntasks = 0;
    if (pairs) {
      cp.tasks = g->kst->pair_tasks;
      cp.n_list = g->kst->n_pair_tasks;
    }
    if (int rc = launch_corner(r, cp, false)) return rc;
    // (gm_stats.tasks: a table's task edges are its rows' entries -- the corner's rows are chunks of the table like any other)
  }
  return GM_OK;
}

// edge supports: zero the supports, three increments per triangle, then sum C(t, 2): all inside the timed region
static int launch_supports(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  const int world = r.ctx.world, rank = r.ctx.rank;
  unsigned *sup = pl.sup_part ? r.rq.sup_out : g->diamond.sup;
  HIP_TRY(hipMemsetAsync(sup, 0, sizeof(unsigned) * (size_t)(pl.sup_part ? diamond_support_entries(g->ne, world) : g->ne), stream));
  r.p.scratch = sup;
  if (int rc = launch_task_tables(r, TK_SUPPORT)) return rc;
  if (pl.tct_long && g->long_rows->n > 0) {
    SupLongParams sl;
    memset(&sl, 0, sizeof sl);
    sl.rp = g->d_rp;
    sl.col = g->d_col;
    sl.rows = g->long_rows->rows;
    sl.prefix = g->long_rows->prefix;
    sl.nrows = g->long_rows->n;
    sl.total = g->long_rows->edges;
    sl.sup = sup;
    sl.topo = tails_trimmed(g) ? 1 : 0;
    sl.rank = rank;
    sl.world = world;
    HIP_TRY(launch_sup_long(sl, g->cu_count, stream));
    r.my_edges += (unsigned long long)((g->long_rows->edges - rank + world - 1) / world);
  }
  if (pl.sup_core) {  // the supports of the hub corner's edges: (A A)_ij on the matrix cores (gm_ctc.hip); a rank takes every world-th block
    CoreTcParams cp;
    memset(&cp, 0, sizeof cp);
    cp.core = g->sup_corner->csym;
    cp.h = g->tasklists->core_h;
    cp.row_words = cp.h / 32;
    cp.rp = g->d_rp;
    cp.base = pl.corner_from;
    cp.first_pos = g->sup_corner->cfirst;
    cp.sup = sup;
    if (int rc = launch_corner(r, cp, true)) return rc;
  }
  if (pl.sup_masks) {  // the masks of the in-edge tasks, summed by column into the supports of their rows
    SupColsParams sc;
    memset(&sc, 0, sizeof sc);
    sc.nv = g->nv;
    sc.ne = g->ne;
    sc.lmin = sup_mask_min_tail(g);
    sc.rp = g->d_rp;
    sc.emoff = g->sup_masks->emoff;
    sc.smask = g->sup_masks->smask;
    sc.sup = sup;
    sc.far_rows = g->sup_masks->far_rows;
    sc.n_far_rows = g->sup_masks->n_far_rows;
    HIP_TRY(launch_sup_cols(sc, g->cu_count, stream));
  }
  if (!pl.sup_part) HIP_TRY(launch_sup_pairs(sup, 0, g->ne, g->d_counters, g->cu_count, stream));
  return GM_OK;
}

// The 5-vertex closed forms on the DAG (gm_wtri.hip; gm_sgl5_raw filled g->w5.sup and says what it wants, rq.wtri_*): the per-entry sums and the
// scatter into 2 T_v, the support-weighted second pass over the triangles (A, B -> counters[0], [1]) -- the task tables, then the out-edges
// no task list holds: the rows beyond the stage or the rows of the hub corner -- and the per-vertex sums.  All inside the timed region.
static int launch_weighted(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  HIP_TRY(hipMemsetAsync(g->w5.out, 0, 64, stream));
  HIP_TRY(hipMemsetAsync(g->w5.tv2, 0, sizeof(unsigned long long) * (size_t)std::max(g->nv, 1), stream));
  WtriEntryParams ep;
  memset(&ep, 0, sizeof ep);
  ep.nv = g->nv; ep.ne = g->ne; ep.rp = g->d_rp; ep.col = g->d_col; ep.sup = g->w5.sup; ep.deg = g->w5deg->deg;
  ep.ed = g->w5.ed; ep.tv2 = g->w5.tv2; ep.out = g->w5.out;
  HIP_TRY(launch_wtri_entries(ep, g->cu_count, stream));
  if (r.rq.wtri_tri) {
    if (int rc = launch_task_tables(r, TK_WTRI)) return rc;
    const WtriParams wp = {g->w5.sup, g->w5.ed, g->w5deg->deg};
    WtriEdgeParams we;
    memset(&we, 0, sizeof we);
    we.rp = g->d_rp; we.col = g->d_col; we.nv = g->nv; we.ne = g->ne;
    we.topo = tails_trimmed(g) ? 1 : 0;
    we.counters = g->d_counters;
    if (pl.tct_long && g->long_rows->n > 0) {
      we.rows = g->long_rows->rows; we.prefix = g->long_rows->prefix; we.nrows = g->long_rows->n; we.total = g->long_rows->edges;
      HIP_TRY(launch_wtri_edges(we, wp, g->cu_count, stream));
    } else if (pl.corner_from < g->nv) {
      we.v0 = pl.corner_from; we.total = g->ne;
      HIP_TRY(launch_wtri_edges(we, wp, g->cu_count, stream));
    }
  }
  if (r.rq.wtri_vert) HIP_TRY(launch_wtri_vertices(g->nv, g->w5.tv2, g->w5deg->deg, g->w5.out, g->cu_count, stream));
  return GM_OK;
}

// The diamond-rim credits of gm_motif_local (gm_orbit_local.hip): the weighted pass's walk -- the task tables, then the out-edges no task
// list holds -- adding into rq.credit_w from the supports rq.credit_sup.  All inside the timed region, the zeroing included.
static int launch_credits(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  HIP_TRY(hipMemsetAsync(r.rq.credit_w, 0, sizeof(unsigned long long) * (size_t)std::max<long long>(g->ne, 1), stream));
  if (int rc = launch_task_tables(r, TK_CREDIT)) return rc;
  const CreditParams crp = {r.rq.credit_sup, r.rq.credit_w};
  WtriEdgeParams we;
  memset(&we, 0, sizeof we);
  we.rp = g->d_rp; we.col = g->d_col; we.nv = g->nv; we.ne = g->ne;
  we.topo = tails_trimmed(g) ? 1 : 0;
  if (pl.tct_long && g->long_rows->n > 0) {
    we.rows = g->long_rows->rows; we.prefix = g->long_rows->prefix; we.nrows = g->long_rows->n; we.total = g->long_rows->edges;
    HIP_TRY(launch_credit_edges(we, crp, g->cu_count, stream));
  } else if (pl.corner_from < g->nv) {
    we.v0 = pl.corner_from; we.total = g->ne;
    HIP_TRY(launch_credit_edges(we, crp, g->cu_count, stream));
  }
  return GM_OK;
}

int run_pattern(const PatternReq &rq, const gm_graph *cg, const gm_launch *la, uint64_t *h_out, int nout, gm_stats *st) {
  PatternRun r;
  r.rq = rq;
  PatternPlan &pl = r.pl;
  int fin_mode = rq.fin_mode;
  // edge supports + sum C(t, 2) (gm_sup.hip): the triangle pass of the task lists with another match handler -- everything up to the
  // launch is the triangle count's
  // (PAT_SUPPORT_PART: the share of a rank -- any world -- of the supports only, added into the caller's zeroed buffer: the ranks' arrays
  // are summed by a reduce-scatter and gm_diamond_support_finish takes sum C(t, 2) of a slice)
  pl.sup_part = rq.pat == PAT_SUPPORT_PART;
  const bool credit = rq.pat == PAT_ORBIT;  // (the rim credits of gm_motif_local: planned exactly as the weighted pass, gm_orbit_local.hip)
  if (credit && (!rq.credit_sup || !rq.credit_w)) return GM_ERR_INVALID;
  pl.wtri = rq.pat == PAT_WTRI || credit;  // (the weighted pass of the 5-vertex closed forms: the same tables and task lists, gm_wtri.hip)
  pl.support = rq.pat == PAT_SUPPORT || pl.sup_part || pl.wtri;
  if (pl.sup_part && !rq.sup_out) return GM_ERR_INVALID;
  pl.pat = pl.support ? PAT_TC : rq.pat;
  if (fin_mode < 0) fin_mode = (pl.pat == PAT_MOTIF3) ? FIN_MOTIF3 : FIN_COPY;
  if (int rc = begin_launch(cg, la, h_out, r.ctx)) return rc;
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  setup_trace("run_pattern: begin_launch");
  if (int rc = plan_pattern(r.ctx, pl)) return rc;
  setup_trace("run_pattern: tables / plan");
  if (int rc = fill_mine_params(r, rq.k)) return rc;
  if (int rc = prepare_scratch(r, rq.k)) return rc;
#ifdef GM_DEBUG_CHUNKS
  if (int rc = debug_chunks_begin(r)) return rc;
#endif
  if (int rc = start_timer(r.ctx)) return rc;
  r.chunks_total = (uint64_t)r.p.count;
  if (pl.use_wide && pl.plan)
    if (int rc = launch_clique4_rounds(r)) return rc;
  if (pl.use_classes)
    if (int rc = launch_classes(r)) return rc;
  int rc = GM_OK;
  if (credit) rc = launch_credits(r);
  else if (pl.wtri) rc = launch_weighted(r);
  else if (pl.support) rc = launch_supports(r);
  else if (pl.use_tct) rc = launch_tc(r);
  else if (r.p.count > 0) HIP_TRY(launch_mine(pl.pat, r.p, r.grid, stream));
  if (rc) return rc;
#ifdef GM_DEBUG_CHUNKS
  if (int rc_d = debug_chunks_dump(r)) return rc_d;
#endif
  for (int i = 0; i < 3; ++i)
    if (r.joined[i]) HIP_TRY(hipStreamWaitEvent(stream, g->aux_done[i], 0));  // the launch ends when all three kernels have
  fill_stats(st, (pl.pat == PAT_DIAMOND || pl.pat == PAT_MOTIF4E) ? r.my_edges / 2 : r.my_edges, r.chunks_total, r.grid,
             kWavesPerBlock * GM_WAVE);
  return end_launch(r.ctx, fin_mode, rq.fin_base, h_out, nout, st);
}

extern "C" int gm_kernel_times(const gm_graph *g, int n, double *ms_out, int *n_out) {
  if (!g || !ms_out || !n_out || n < 0) return GM_ERR_INVALID;
  while (g->ring_alias) g = g->ring_alias;  // (a derived handle may itself run on a renumbered copy)
  const unsigned long long have = std::min<unsigned long long>(g->ev_launches, gm_graph::kEvRing);
  const int m = (int)std::min<unsigned long long>((unsigned long long)n, have);
  HIP_TRY(hipSetDevice(g->device));
  for (int i = 0; i < m; ++i) {  // oldest of the last m launches first
    const unsigned long long idx = (g->ev_launches - (unsigned long long)m + (unsigned long long)i) % gm_graph::kEvRing;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev[idx][0], g->ev[idx][1]));
    ms_out[i] = ms;
    // 4-motif: one call = the per-edge kernel on this handle + the rectangle kernel on the renumbered copy + the 4-clique kernel on the
    // cached DAG; the launches of the same recency on those handles belong to the same call
    for (const gm_graph *x : g->ring_extra) {
      const unsigned long long back = (unsigned long long)(m - i);
      while (x && x->ring_alias) x = x->ring_alias;
      if (!x || x->ev_launches < back) continue;
      const unsigned long long xi = (x->ev_launches - back) % gm_graph::kEvRing;
      float xms = 0.f;
      HIP_TRY(hipEventElapsedTime(&xms, x->ev[xi][0], x->ev[xi][1]));
      ms_out[i] += xms;
    }
  }
  *n_out = m;
  return GM_OK;
}

// the part of gm_kernel_times' durations that the hub-corner kernel of a launch took (gm_ctc.hip; 0 for a launch without one): the
// streamed kernels' time is the difference -- what bench.py prices against the HBM roofline
extern "C" int gm_corner_times(const gm_graph *g, int n, double *ms_out, int *n_out) {
  if (!g || !ms_out || !n_out || n < 0) return GM_ERR_INVALID;
  while (g->ring_alias) g = g->ring_alias;
  const unsigned long long have = std::min<unsigned long long>(g->ev_launches, gm_graph::kEvRing);
  const int m = (int)std::min<unsigned long long>((unsigned long long)n, have);
  HIP_TRY(hipSetDevice(g->device));
  for (int i = 0; i < m; ++i) {
    const unsigned long long idx = (g->ev_launches - (unsigned long long)m + (unsigned long long)i) % gm_graph::kEvRing;
    float ms = 0.f;
    if (g->ev_corner[idx]) HIP_TRY(hipEventElapsedTime(&ms, g->ev[idx][2], g->ev[idx][3]));
    ms_out[i] = ms;
  }
  *n_out = m;
  return GM_OK;
}

// The DAG kernels that profit from a TOPOLOGICAL numbering (every edge from a smaller to a larger id: an in-edge task streams only the
// part of N+(u) beyond v, the k-clique matrices are strictly upper triangular) run on the cached renumbered copy of a DAG that is not
// numbered that way (get_relabeled mode 2). tune[6] & GM_T6_AS_NUMBERED: on the graph as numbered, like the SgL patterns.
// Only where lists are long: the trimmed streams and the triangular counts save work per KEY, the renumbering concentrates the hubs
// in a few host chunks -- measured (profiles/r03/ab_topo_view.txt, TC ms as numbered / renumbered, whole lists / renumbered, trimmed):
// R-MAT-22 6.45 / 6.26 / 5.28, LiveJournal-size flat degrees (5.5 keys per task) 0.88 / 0.85 / 0.86, power law with LiveJournal's
// maximum degree (5.5 keys per task) 1.14 / 1.88 / 1.59. The switch is the mean length of the row a DAG entry sits in, sum d+^2 / |E+|
// (R-MAT-22: 157, R-MAT-22 ef 28: 322, R-MAT-24: 367; the power-law graph: 11.6, flat: 10.5): >= kTopoMinMeanRow -> renumbered. GM_TOPO_MIN_ROW overrides (0: always).
// Round 6: kTopoMinMeanRow = 0 -- with the kernels of rounds 4 - 5 the renumbered copy wins on those two graphs as well (gm_mine.h).
__global__ __launch_bounds__(256) void sum_sq_deg_kernel(int nv, const int *__restrict__ rp, unsigned long long *__restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s = 0;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const unsigned long long d = (unsigned long long)(rp[v + 1] - rp[v]);
    s += d * d;
  }
  s = gm::wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

// sum d^2 / ne of a handle's rows = the mean length of the row an entry sits in (cached)
int ensure_mean_sq_deg(gm_graph *self) {
  return self->facts.mean_sq_deg.ensure(self->mu, [&](double &mean) {
    unsigned long long s2 = 0;
    if (int rc = reduce_to_u64(self, self->nv > 0, "sum_sq_deg_kernel", &s2, [&](unsigned long long *d_s) { hipLaunchKernelGGL(sum_sq_deg_kernel, rows_grid(self), dim3(256), 0, 0, self->nv, self->d_rp, d_s); })) return rc;
    mean = self->ne > 0 ? (double)s2 / (double)self->ne : 0.0;
    return kOnceBuilt;
  });
}

// Triangles per DAG entry, ESTIMATED: every stride-th entry (u -> v), |N+(u) ^ N+(v)| by a merge of the two sorted rows (at most 512 steps:
// the estimate is asked for on short-row graphs), averaged.  The edge supports choose between the key stream and the task lists by it.
__global__ __launch_bounds__(256) void tri_sample_kernel(int nv, long long ne, const int *__restrict__ rp, const int *__restrict__ col, long long stride,
                                                         int nsamples, unsigned long long *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long c = 0;
  if (i < nsamples) {
    const long long e = (long long)i * stride;
    if (e < ne) {
      int lo = 0, hi = nv - 1;  // the row of entry e
      while (lo < hi) {
        const int mid = (int)(((long long)lo + hi + 1) >> 1);
        if ((long long)rp[mid] <= e) lo = mid; else hi = mid - 1;
      }
      const int v = col[e];
      int a = rp[lo], ae = rp[lo + 1], b = rp[v], be = rp[v + 1];
      for (int step = 0; step < 512 && a < ae && b < be; ++step) {
        const int x = col[a], y = col[b];
        c += x == y ? 1ull : 0ull;
        a += x <= y ? 1 : 0;
        b += y <= x ? 1 : 0;
      }
    }
  }
  c = gm::wave_sum_u64(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

int ensure_tri_per_edge(gm_graph *self) {
  return self->facts.tri_per_edge.ensure(self->mu, [&](double &tri) {
    const int nsamples = (int)std::min<long long>(1 << 16, std::max<long long>(self->ne, 1));
    const long long stride = std::max<long long>(1, self->ne / nsamples);
    unsigned long long s = 0;
    if (int rc = reduce_to_u64(self, self->ne > 0, "tri_sample_kernel", &s, [&](unsigned long long *d_s) {
          hipLaunchKernelGGL(tri_sample_kernel, dim3((unsigned)((nsamples + 255) / 256)), dim3(256), 0, 0, self->nv, (long long)self->ne, self->d_rp, self->d_col, stride,
                             nsamples, d_s);
        })) return rc;
    tri = (double)s / (double)nsamples;
    return kOnceBuilt;
  });
}

// Heavy chunks of the task-list kernels (a hub hosts 10^5 in-edges) are cut into PARTS that share the chunk's batches -- and every part
// hashes the chunk's rows again (~10 us).  A part bounds the tail of a rank's launch, so its size follows the rank's share: the
// launch streams about ne * (sum d+^2 / ne) / 2 keys, a part takes 1/3000 of a rank's share of them, between 128 K and 4 M keys.
// One-GPU simulation of 8 rank shares, TC, parts of 64 K / 128 K / 256 K / 512 K / 1 M keys: R-MAT-24 9.08 / 7.14 / 6.11 / 5.68 / 5.54 ms per
// rank (ideal 5.25), R-MAT-22 0.63 / 0.56 / 0.55 / 0.55 / 0.78; one GPU, 256 K / 512 K / 1 M / 2 M / 4 M: R-MAT-22 3.14 / 3.09 / 3.07 / 3.06 / 3.04 ms,
// R-MAT-24 47.2 / 43.7 / 41.9 / 41.2 / 40.9 (profiles/r03/ab_share_scaling.txt).
unsigned long long task_part_cap(gm_graph *g, int world) {
  if (const char *e = gm_sweep_env("GM_TCT_PART_KKEYS")) return (unsigned long long)std::max(4, atoi(e)) << 10;  // (sweeps)
  double keys = 0.0;
  if (ensure_mean_sq_deg(g) == GM_OK) keys = (double)g->ne * *g->facts.mean_sq_deg * 0.5;
  const double cap = keys / (3000.0 * (double)std::max(world, 1));
  return (unsigned long long)std::min(std::max(cap, (double)(128 << 10)), (double)(4 << 20));
}

int topo_view(const gm_graph *dag, const gm_launch *la, gm_graph **run_on) {
  gm_graph *self = const_cast<gm_graph *>(dag);
  if (!self) return GM_ERR_INVALID;
  if (int rc = reject_big(self)) return rc;
  *run_on = self;
  if (la && (la->tune[6] & GM_T6_AS_NUMBERED)) return GM_OK;
  bool topo = false;
  int rc = graph_is_topological(self, &topo);
  if (rc || topo) return rc;
  rc = ensure_mean_sq_deg(self);
  if (rc) return rc;
  double min_row = (double)kTopoMinMeanRow;
  if (const char *e = gm_opt("GM_TOPO_MIN_ROW")) min_row = atof(e);
  if (gm_sweep_env("GM_TABLE_INFO")) fprintf(stderr, "[topo view] sum d+^2 / |E+| = %.1f (switch at %.1f)\n", *self->facts.mean_sq_deg, min_row);
  if (*self->facts.mean_sq_deg < min_row) return GM_OK;  // short lists: as numbered
  return get_relabeled(self, 2, run_on);
}

int run_tc(const gm_graph *dag, const gm_launch *la, uint64_t *out, int nout, gm_stats *st, int fin_mode, unsigned long long fin_base) {
  gm_graph *run_on = nullptr;
  int rc = topo_view(dag, la, &run_on);
  if (rc) return rc;
  rc = run_pattern({PAT_TC, 3, fin_mode, fin_base}, run_on, la, out, nout, st);
  record_ran_on(dag, run_on);  // (whatever rc)
  return rc;
}

extern "C" int gm_tc(const gm_graph *dag, const gm_launch *la, uint64_t *total, gm_stats *st) { return run_tc(dag, la, total, 1, st); }
// tooling (the byte model of bench.py, tests): the hub corner the triangle count of this handle takes on the matrix cores (after a first gm_tc)
extern "C" int gm_tc_core_info(const gm_graph *dag, int64_t info[4]) {
  if (!dag || !info) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  // (a symmetric handle: the oriented copy its formula 3-motif counts the triangles of)
  const int rc = topo_view(dag->dag_cache ? dag->dag_cache : dag, nullptr, &run_on);
  if (rc) return rc;
  const bool on = run_on->kst->skip_from < run_on->nv;
  const long long nJ = on ? (run_on->kst->core_h + 63) >> 6 : 0;
  info[0] = on ? run_on->kst->core_h : 0;           // vertices of the corner (0: every edge is a task of the key stream)
  info[1] = on ? run_on->kst->core_edges : 0;       // DAG entries inside it
  info[2] = nJ * (nJ + 1) / 2;                    // 64 x 64 blocks of the masked product
  info[3] = on ? run_on->core->h : 0;              // vertices of the core bitmap the corner is a part of
  return GM_OK;
}

// ... and the block pairs of it the product takes (tc_pairs_setup, gm_tasks.hip): info[0] = rows of the region (0: no selection -- the full
// triangle of gm_tc_core_info's corner, or none), [1] = pairs taken, [2] = pairs that hold keys, [3] = DAG entries in the product,
// [4] = keys of the stream's model that left the stream, [5] = R of the rule
extern "C" int gm_tc_pairs_info(const gm_graph *dag, int64_t info[6]) {
  if (!dag || !info) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  const int rc = topo_view(dag->dag_cache ? dag->dag_cache : dag, nullptr, &run_on);
  if (rc) return rc;
  const bool on = run_on->kst->skip_from < run_on->nv && run_on->kst->pair_region > 0;
  for (int i = 0; i < 6; ++i) info[i] = on ? run_on->kst->pair_info[i] : 0;
  return GM_OK;
}

// The oriented copy of a symmetric handle (gm_graph_orient), built once under its own lock: two solvers called on the same handle from two
// threads -- the formula 3-motif and the one-GPU diamond share it -- must not both orient and leak a handle.  A graph of
// >= 2^31 entries too: its oriented copy must fit the 32-bit task index, gm_graph_orient checks.
int ensure_dag_cache(gm_graph *g) {
  std::lock_guard<std::mutex> lk(g->dag_mu);
  if (g->dag_cache) return GM_OK;
  gm_graph *dag = nullptr;
  const int rc = gm_graph_orient(g, &dag);
  if (rc) return rc;
  dag->pool_owner = g;
  g->dag_cache = dag;
  return GM_OK;
}

extern "C" int gm_clique(const gm_graph *dag, int k, const gm_launch *la, uint64_t *total, gm_stats *st) {
  if (k == 3) return run_tc(dag, la, total, 1, st);
  if (k < 3 || k > GM_MAX_CLIQUE_K) {
    if (total) *total = 0;
    return GM_ERR_INVALID;
  }
  if (k == 4 && !(la && (la->tune[6] & (GM_T6_CLIQUE4_MINING | GM_T6_AS_NUMBERED)))) {
    // the re-hosted first level and the pair counts want a TOPOLOGICAL numbering (upper-triangular matrices: gm_cbuild.hip): a DAG
    // that is not numbered that way runs on its cached renumbered copy (tune[6] & GM_T6_AS_NUMBERED: on the graph as numbered, like the SgL
    // patterns; & GM_T6_CLIQUE4_MINING: everything in the mining kernel, which does not care)
    gm_graph *run_on = nullptr;
    int rc = topo_view(dag, la, &run_on);
    if (rc) return rc;
    rc = run_pattern({PAT_CLIQUE4, k}, run_on, la, total, 1, st);
    record_ran_on(dag, run_on);  // (whatever rc)
    return rc;
  }
  return run_pattern({k == 4 ? PAT_CLIQUE4 : PAT_CLIQUEK, k}, dag, la, total, 1, st);
}

// 4-motif, formula form (src/motif/cpu_kernels/automine_formula.h:21-56 + src/motif/omp_formula.cc:41-45):
// raw[0..3] = the per-edge sums counter[0], counter[1], counter[2], counter[4] (PAT_MOTIF4E, one |N(v0)^N(v1)| per
// undirected edge), raw[4] = edge-induced 4-cycles (rectangle kernel), raw[5] = 4-cliques (clique kernel on the cached
// DAG). Every raw value is a plain sum over tasks, so per-rank partials add up; gm_motif4_finish turns the summed raw
// values into the six vertex-induced counts.
// With la->d_counts set the six raw sums are left in that DEVICE buffer (raw[0..3] by the per-edge kernel, raw[4] by the
// rectangle kernel, raw[5] by the clique kernel, all ordered on la->stream) and nothing synchronises unless `raw` is given
// too -- this is what feeds the RCCL all-reduce of motif_multigpu.
extern "C" int gm_motif4_partial(const gm_graph *sym, const gm_launch *la, uint64_t raw[6], gm_stats *st) {
  if (!sym || (!raw && !(la && la->d_counts))) return GM_ERR_INVALID;
  if (int rc0 = reject_big(sym)) return rc0;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2 = launch_or_default(la);
  uint64_t *d_out = l2.d_counts;
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  SubLaunches sub;
  int rc = sub.run([&](gm_stats *s) { return run_pattern({PAT_MOTIF4E, 4, FIN_RAW4}, sym, &l2, raw, 4, s); });
  if (rc) return rc;
  const gm_stats s1 = sub.last;
  const gm_graph *rect_handle = sym;
  {
    const gm_graph *rect_on = sym;
    if (!(l2.tune[6] & GM_T6_AS_NUMBERED)) {
      gm_graph *r = nullptr;
      rc = get_relabeled(g, (l2.tune[6] & GM_T6_SGL_FLAT) ? 1 : 0, &r);
      if (rc) return rc;
      rect_on = r;
    }
    l2.d_counts = d_out ? d_out + 4 : nullptr;
    rc = sub.run([&](gm_stats *s) {
      return (l2.tune[6] & GM_T6_SGL_FLAT) ? run_rect_flat(rect_on, &l2, raw ? &raw[4] : nullptr, s) : run_rect_acc(rect_on, &l2, raw ? &raw[4] : nullptr, s);
    });
    rect_handle = rect_on;
  }
  if (rc) return rc;
  l2.d_counts = d_out ? d_out + 5 : nullptr;
  rc = sub.run([&](gm_stats *s) { return gm_clique(g->dag_cache, 4, &l2, raw ? &raw[5] : nullptr, s); });  // (on the DAG's topological view)
  if (rc) return rc;
  if (st) {
    *st = s1;
    st->kernel_ms = sub.ms;
  }
  record_ran_on(g, g, true, (rect_handle != sym) ? rect_handle : nullptr, g->dag_cache);  // (tune[6] & GM_T6_AS_NUMBERED: the rectangle kernel ran on this handle itself)
  return GM_OK;
}

// raw sums -> the six vertex-induced counts (host fix-up of src/motif/omp_formula.cc:41-45, same arithmetic on both sides)
__host__ __device__ static inline void motif4_finish_math(const unsigned long long *raw, unsigned long long *counts) {
  const unsigned long long k4 = raw[5];
  const unsigned long long diamond = raw[3] / 2 - 6 * k4;            // total[4] = total[4]/2 - 6*total[5]
  const unsigned long long tailed = raw[2] / 2 - 2 * diamond;        // total[2] = total[2]/2 - 2*total[4]
  const unsigned long long cycle4 = raw[4] - diamond - 3 * k4;       // vertex-induced 4-cycles from the edge-induced count
  const unsigned long long path4 = raw[1] - 4 * cycle4;              // total[1] = total[1] - 4*total[3]
  const unsigned long long star3 = raw[0] / 6 - tailed / 3;          // total[0] = total[0]/6 - total[2]/3
  counts[0] = star3; counts[1] = path4; counts[2] = tailed; counts[3] = cycle4; counts[4] = diamond; counts[5] = k4;
}

__global__ void motif4_finish_kernel(unsigned long long *__restrict__ c) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned long long raw[6], out[6];
  for (int i = 0; i < 6; ++i) raw[i] = c[i];
  motif4_finish_math(raw, out);
  for (int i = 0; i < 6; ++i) c[i] = out[i];
}

extern "C" int gm_motif4_finish(const uint64_t raw[6], uint64_t counts[6]) {
  if (!raw || !counts) return GM_ERR_INVALID;
  unsigned long long r[6], c[6];
  for (int i = 0; i < 6; ++i) r[i] = raw[i];
  motif4_finish_math(r, c);
  for (int i = 0; i < 6; ++i) counts[i] = c[i];
  return GM_OK;
}

extern "C" int gm_motif(const gm_graph *sym, int k, const gm_launch *la, uint64_t *counts, int ncounts, gm_stats *st) {
  if (k == 4) {
    const bool async = la && la->d_counts;  // the asynchronous contract of every solver: counts may be NULL then
    if (ncounts < 6 || (!counts && !async)) return GM_ERR_INVALID;
    if (la && la->world > 1) return GM_ERR_UNSUPPORTED;  // multi-GPU: gm_motif4_partial + all-reduce + gm_motif4_finish
    uint64_t raw[6];
    int rc = gm_motif4_partial(sym, la, counts ? raw : nullptr, st);
    if (rc) return rc;
    if (async) {  // finish in place on the device, ordered on the launch stream
      hipLaunchKernelGGL(motif4_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)la->stream, (unsigned long long *)la->d_counts);
      HIP_TRY(hipGetLastError());
    }
    return counts ? gm_motif4_finish(raw, counts) : GM_OK;
  }
  if (k != 3) return GM_ERR_INVALID;
  if (ncounts < 2) return GM_ERR_INVALID;
  // Default: the reference's OTHER 3-motif solver (motif_omp_formula / motif_gpu_formula, src/motif/omp_formula.cc:39-46: the triangles
  // of the oriented graph, wedges = sum C(d,2) - 3T) -- the same two counts from 1/4 of the streamed keys, and the only form a graph
  // of 2^31 entries or more fits (its oriented copy has a 32-bit task index).  tune[6] & GM_T6_PER_EDGE, or one of the A/B switches of
  // the per-edge kernels: automine_3motif's enumeration (src/motif/cpu_kernels/automine_base.h:2-22), one bounded intersection of the
  // two symmetric lists per edge (gm_hrow.hip, gm_chunk.h).
  const int t6 = la ? la->tune[6] : 0;
  const bool per_edge = ((t6 & (GM_T6_PER_EDGE | GM_T6_NO_CLASSES | GM_T6_FORCE_CLASSES | GM_T6_CLASSES_SORTED_COPY | GM_T6_GIANT_SPLIT | GM_T6_HROW_MUL32)) || (la && la->tune[5] == 1) ||
                         gm_sweep_env("GM_MOTIF3_PER_EDGE")) && !(sym && sym->d_rp64);
  if (!per_edge) {
    const int rc = gm_motif_formula(sym, k, la, counts, ncounts, st);
    if (rc == GM_OK && st) st->tasks *= 2;  // (the graph's directed entries, as the enumeration reports them: two per task edge of the DAG)
    return rc;
  }
  // The enumeration's two totals do not depend on the vertex numbering, its WORK does: for an edge {lo < hi} only the common neighbours
  // below hi count, and the kernels trim the streamed list to them.  Numbered by DESCENDING degree (the cached copy the SgL wedge forms use),
  // "below hi" = "of higher degree than hi": the trimmed list is what an oriented row would be -- sum_v d+(v)^2 streamed keys instead of
  // sum_e min(d(u), d(v)) over the symmetric lists (R-MAT-24: 150 G).  GM_MOTIF3E_AS_NUMBERED / tune[6] & GM_T6_AS_NUMBERED: on the graph as given.
  const gm_graph *run_on = sym;
  if (!(t6 & GM_T6_AS_NUMBERED) && !gm_sweep_env("GM_MOTIF3E_AS_NUMBERED")) {
    gm_graph *r = nullptr;
    const int rc = get_relabeled(const_cast<gm_graph *>(sym), 1, &r);
    if (rc == GM_ERR_HIP && g_last_hip_error == (int)hipErrorOutOfMemory) {  // (the copy is an optimisation -- about the size of the graph again: without it the graph runs as numbered)
      (void)hipGetLastError();
      g_last_error.clear();
    } else if (rc) {
      return rc;
    } else {
      run_on = r;
    }
  }
  const int rc = run_pattern({PAT_MOTIF3, 3}, run_on, la, counts, ncounts, st);
  if (run_on != sym) record_ran_on(sym, run_on);  // (whatever rc; as numbered, nothing is recorded: only start_timer has cleared the alias)
  return rc;
}

// motif_omp_formula / motif_gpu_formula (src/motif/omp_formula.cc:39-46, cpu_kernels/automine_formula.h:2-19):
// enumerate only the triangles, derive the wedges: wedges = sum_v C(d(v),2) - 3*T. Here the triangles come from the
// TC kernel on the oriented graph (built once per handle and cached), so the hub rows of the symmetric graph are
// never intersected. Counts are identical to gm_motif; with world > 1 the sum_v C(d,2) term is contributed by rank 0
// and the per-rank partial wedge count is only meaningful after the all-reduce (mod 2^64 arithmetic).
template <class OffT>
__global__ __launch_bounds__(256) void sum_c2_kernel(int nv, const OffT *__restrict__ rp, unsigned long long *__restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s = 0;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const unsigned long long d = (unsigned long long)(rp[v + 1] - rp[v]);
    s += d * (d - 1) / 2;
  }
  s = gm::wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

extern "C" int gm_motif_formula(const gm_graph *sym, int k, const gm_launch *la, uint64_t *counts, int ncounts, gm_stats *st) {
  if (!sym) return GM_ERR_INVALID;
  if (k != 3) return (k == 4) ? GM_ERR_UNSUPPORTED : GM_ERR_INVALID;
  if (ncounts < 2) return GM_ERR_INVALID;
  gm_graph *g = const_cast<gm_graph *>(sym);
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  // sum_v C(d(v),2): one reduction kernel over the offsets
  if (const int rc_s = g->facts.sum_c2.ensure(g->mu, [&](unsigned long long &s2) {
        return reduce_to_u64(g, true, "sum_c2_kernel", &s2, [&](unsigned long long *acc) {
          if (g->d_rp64) hipLaunchKernelGGL((sum_c2_kernel<long long>), rows_grid(g), dim3(256), 0, 0, g->nv, (const long long *)g->d_rp64, acc);
          else hipLaunchKernelGGL((sum_c2_kernel<int>), rows_grid(g), dim3(256), 0, 0, g->nv, (const int *)g->d_rp, acc);
        });
      })) return rc_s;
  const int rank = la ? la->rank : 0;
  const int rc = run_tc(g->dag_cache, la, counts, ncounts, st, FIN_MOTIF3_FORMULA, rank == 0 ? *g->facts.sum_c2 : 0ull);
  record_ran_on(g, g->dag_cache);  // (whatever rc; run_tc has recorded the handle the oriented copy ran on)
  return rc;
}

// Tooling: the level-2 part of SURVEY.md 8(d)'s ALGORITHMIC bytes of one 4-clique launch,
//   sum_e [ 8|S1| + sum_{v2 in S1} (4(|S1| + d+(v2)) + 16) ]  =  24*sum|S1| + 4*sum|S1|^2 + 4*sum_{matches} d+(v2),
// from three sums the mining kernel itself produces (PAT_DAGSTATS). The level-1 part 4*sum_e(d+(v0)+d+(v1)) + 40|E+|
// is the TC formula (computed by the caller from the CSR arrays).
extern "C" int gm_clique4_level2_bytes(const gm_graph *dag, uint64_t *bytes) {
  if (!dag || !bytes) return GM_ERR_INVALID;
  uint64_t raw[4] = {0, 0, 0, 0};  // raw[0] = sum n^2, raw[1] = sum_{matches} d+(v2), raw[2] = sum n
  const int rc = run_pattern({PAT_DAGSTATS, 4, FIN_RAW4}, dag, nullptr, raw, 4, nullptr);
  if (rc) return rc;
  *bytes = 24ull * raw[2] + 4ull * raw[0] + 4ull * raw[1];
  return GM_OK;
}

// tooling (the byte model of bench.py): the blocked gather of the most recent whole-graph 4-clique plan of this handle
extern "C" int gm_clique4_gather_info(const gm_graph *dag, int64_t info[4]) {
  if (!dag || !info) return GM_ERR_INVALID;
  info[0] = info[1] = info[2] = info[3] = 0;
  gm_graph *g = nullptr;
  {  // (the plan belongs to the handle the count runs on: the topologically renumbered copy of a DAG that is not numbered that way)
    const int rc = topo_view(dag, nullptr, &g);
    if (rc) return rc;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  for (auto &pl : g->clique_plans) {
    if (pl.world != 1) continue;
    for (auto &rd : pl.rounds) {
      info[0] += (int64_t)rd.n_gunits;             // (vertex, block) units
      info[1] += (int64_t)rd.gather_table_bytes;   // bytes they read by construction: 16 B record + 4 B per row + their table dwords
      info[2] += (int64_t)rd.n_gitems;             // work items (each loads one block image of <= 64 KB unless it shares it with its predecessor)
    }
    info[3] = g->core_blocks->n;
    break;
  }
  return GM_OK;
}

// tooling (tests): what the whole-graph 4-clique plan of this handle holds, on the copy the count ran on -- the handle itself
// (as_numbered: a call under GM_T6_AS_NUMBERED; a DAG that is numbered topologically), else its topological copy.  Read-only: nothing is
// built here, no device pass (GM_ERR_INVALID: no such call yet).
//   out[0] topo   [1] stage   [2] core_base (-1: no core)   [3] rounds   [4] wide vertices   [5 .. 7] ... per matrix-core class 0 / 1 / 2
//   [8] build tasks (all rounds)   [9] gather units   [10] gather items   [11] chunks and [12] entries of the rows left to the mining
//   kernel's arena path (> kCbMaxDeg; the table of that launch, -1 / -1: none was built)
extern "C" int gm_clique_plan_info(const gm_graph *dag, int as_numbered, int64_t *out, int n) {
  if (!dag || !out || n < 13) return GM_ERR_INVALID;
  auto plan_of = [](gm_graph *g) -> const CliquePlan * {
    if (!g) return nullptr;
    for (auto &pl : g->clique_plans)
      if (pl.world == 1) return &pl;
    return nullptr;
  };
  gm_graph *self = const_cast<gm_graph *>(dag), *g = self;
  if (!as_numbered && self->relabel_cache[2]) g = self->relabel_cache[2];
  std::lock_guard<std::mutex> lk(g->mu);
  const CliquePlan *pl = plan_of(g);
  if (!pl) return GM_ERR_INVALID;
  for (int i = 0; i < 13; ++i) out[i] = 0;
  out[0] = pl->topo ? 1 : 0;
  out[1] = pl->stage;
  out[2] = pl->core_base;
  out[3] = (int64_t)pl->rounds.size();
  out[4] = (int64_t)pl->verts.size();
  for (const auto &rd : pl->rounds) {
    for (int c = 0; c < 3; ++c) out[5 + c] += (int64_t)(rd.mcls_begin[c + 1] - rd.mcls_begin[c]);
    out[8] += (int64_t)rd.n_tasks;
    out[9] += (int64_t)rd.n_gunits;
    out[10] += (int64_t)rd.n_gitems;
  }
  out[11] = out[12] = -1;
  for (const auto &t : g->tables)
    if (t.rf.only_lo == kCbMaxDeg && t.rf.skip_clique_wide == 0 && t.bit_words == kBitWords && t.rf.tct == 0) {
      out[11] = (int64_t)t.n;
      out[12] = (int64_t)t.total_edges;
      break;
    }
  return GM_OK;
}

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_launch_kernel() {}
void gm_touch_launch() { hipLaunchKernelGGL(gm_touch_launch_kernel, dim3(1), dim3(1), 0, 0); }
