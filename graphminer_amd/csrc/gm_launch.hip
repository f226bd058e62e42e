// gm_launch.hip -- the solvers of the C ABI: launch prologue / epilogue, the dequeue words, run_pattern (TC, edge supports, diamond, 3-motif, k-clique,
// the per-edge sums of 4-motif) as a driver over plan_pattern / fill_mine_params / prepare_scratch / launch_*, the SgL launches, gm_tc / gm_sgl / gm_sgl5_* / gm_sgl6_* / gm_clique / gm_motif*.
// Reference launch logic: src/triangle/gpu_base.cu:36-45, src/sgl/gpu_base.cu:37-75, src/clique/gpu_base.cu:28-50, src/motif/gpu_base.cu:42-75.
#include "gm_host.h"

using namespace gm;

// ------------------------------------------------------------------------------------------------
// solvers
// ------------------------------------------------------------------------------------------------
enum FinMode : int { FIN_COPY = 0, FIN_MOTIF3 = 1, FIN_MOTIF3_FORMULA = 2, FIN_RAW4 = 3, FIN_HALF_SIGNED = 4 };

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
static int reject_big(const gm_graph *g) {
  if (!g || !g->d_rp64) return GM_OK;
  g_last_error = "this solver walks the graph it is given with a 32-bit task index; " + std::to_string(g->ne) +
                 " entries: orient it (gm_graph_orient) for TC / k-clique, gm_motif k = 3 counts through the formula solver";
  return GM_ERR_TOO_LARGE;
}

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
  if (g->giant_edges == ~0ull) {
    HIP_TRY(hipSetDevice(g->device));
    DevOwn<unsigned long long> d_s;
    unsigned long long s = 0;
    HIP_TRY(d_s.alloc(8));
    hipError_t e = hipMemset(d_s, 0, 8);
    if (e == hipSuccess && g->nv > 0)
      hipLaunchKernelGGL(giant_edges_kernel, dim3((unsigned)std::min<long long>(((long long)g->nv + 255) / 256, 2048)), dim3(256), 0, 0, g->nv, g->d_rp, d_s);
    if (e == hipSuccess) e = hipMemcpy(&s, d_s, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "giant_edges_kernel", __FILE__, __LINE__);
    g->giant_edges = s;
  }
  *out = g->giant_edges;
  return GM_OK;
}

// ---- common launch prologue / epilogue of every mining entry point -----------------------------------------------
struct LaunchCtx {
  gm_graph *g = nullptr;
  gm_launch la;          // caller's launch descriptor, or the all-zero default
  int world = 1, rank = 0;
  hipStream_t stream = nullptr;
  hipEvent_t *evp = nullptr;  // event pair of this launch (ring slot)
};

// ---- the dequeue words of a launch ---------------------------------------------------------------------------------------------
// d_counters is one 64-byte block: four 64-bit accumulators, then the dequeue heads of the kernels of ONE launch -- begin_launch zeroes the
// whole block on the launch stream.  Which launches meet in one block:
//   * the symmetric-graph patterns (diamond, 3-motif, the per-edge sums of 4-motif): the main table + the workgroup classes 1 .. 3;
//   * the task-list kernels of a DAG (TC, edge supports): the main table + the long-row table (TC) + the big-stage table + the hub corner.
//     They never run classes (those want a symmetric graph), so QW_TC_LONG / QW_STAGE_BIG may share the words of classes 1 / 2;
//   * the cliques and everything else: the main table only (the 4-clique rounds have their own block, d_wide_queue);
//   * the SgL map kernels (rectangle / house / pentagon, run_rect_* / run_house_*) are launches of their own and dequeue with 64-bit heads:
//     QW64_MAIN overlays the 32-bit words 0 - 1, QW64_LDS (the LDS-map kernel beside the global-map one) the words 2 - 3.
constexpr size_t kCounterBlockBytes = 64;
enum QueueWord : int { QW_MAIN = 0, QW_CLASS1 = 1, QW_CLASS2 = 2, QW_CLASS3 = 3, QW_TC_LONG = 1, QW_STAGE_BIG = 2, QW_CORNER = 4, QW_LAST = QW_CORNER };
enum QueueWord64 : int { QW64_MAIN = 0, QW64_LDS = 1, QW64_LAST = QW64_LDS };
static_assert(QW_CLASS2 == QW_CLASS1 + 1 && QW_CLASS3 == QW_CLASS1 + 2, "class cls dequeues from word QW_CLASS1 + (cls - 1)");
static_assert(32 + (QW_LAST + 1) * sizeof(unsigned) <= kCounterBlockBytes && 32 + (QW64_LAST + 1) * sizeof(unsigned long long) <= kCounterBlockBytes,
              "every dequeue word lies behind the four accumulators, inside the block begin_launch zeroes");
static inline unsigned *queue_word(const gm_graph *g, int w) { return reinterpret_cast<unsigned *>(g->d_counters + 4) + w; }
static inline unsigned long long *queue_word64(const gm_graph *g, int w) { return reinterpret_cast<unsigned long long *>(queue_word(g, 2 * w)); }

// validates the arguments, selects the device, zeroes the 64-byte counter block on the launch stream
static int begin_launch(const gm_graph *cg, const gm_launch *la, const uint64_t *h_out, LaunchCtx &c) {
  if (!cg) return GM_ERR_INVALID;
  if (int rc = reject_big(cg)) return rc;
  c.g = const_cast<gm_graph *>(cg);
  memset(&c.la, 0, sizeof c.la);
  if (la) c.la = *la;
  c.world = c.la.world > 1 ? c.la.world : 1;
  c.rank = c.la.rank;
  if (c.rank < 0 || c.rank >= c.world) return GM_ERR_INVALID;
  if (!h_out && !c.la.d_counts) return GM_ERR_INVALID;
  HIP_TRY(hipSetDevice(c.g->device));
  {  // every solver relies on ascending rows (checked once per handle; the reference sorts on request: adj_sorted = 0)
    bool sorted = false;
    if (int rc = graph_rows_sorted(c.g, &sorted)) return rc;
    if (!sorted) {
      g_last_error = "the neighbour lists of this graph are not strictly ascending: call gm_graph_sort_neighbors first (Graph::sort_neighbors, adj_sorted = 0)";
      return GM_ERR_INVALID;
    }
  }
  c.stream = (hipStream_t)c.la.stream;
  HIP_TRY(hipMemsetAsync(c.g->d_counters, 0, kCounterBlockBytes, c.stream));
  return GM_OK;
}

static int start_timer(LaunchCtx &c) {
  c.g->ring_alias = nullptr;
  c.g->ring_extra[0] = c.g->ring_extra[1] = nullptr;
  c.evp = c.g->ev[c.g->ev_launches % gm_graph::kEvRing];
  c.g->ev_corner[c.g->ev_launches % gm_graph::kEvRing] = false;
  c.g->ev_launches++;
  HIP_TRY(hipEventRecord(c.evp[0], c.stream));
  return GM_OK;
}

// stops the timer, publishes the counters: to d_counts (device, asynchronous) and / or to h_out (synchronises)
static int end_launch(LaunchCtx &c, int fin_mode, unsigned long long fin_base, uint64_t *h_out, int nout, gm_stats *st) {
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

static void fill_stats(gm_stats *st, uint64_t tasks, uint64_t chunks, int grid, int block) {
  if (!st) return;
  st->kernel_ms = 0.0;
  st->tasks = tasks;
  st->chunks = chunks;
  st->grid = (uint32_t)grid;
  st->block = (uint32_t)block;
}

// workgroups of a launch: one per unit of work, at most per_cu on every CU, at least one
static inline int clamp_grid(long long want, long long cap) { return (int)std::max<long long>(1, std::min<long long>(want, cap)); }
static inline int grid_for(long long count, int cu_count, long long per_cu) { return clamp_grid(count, (long long)cu_count * per_cu); }

// a device buffer of a handle, grown to `need` bytes (never shrunk; the old contents are not kept)
template <class T>
static int grow_dev(DevOwn<T> &buf, size_t *bytes, size_t need) {
  if (need <= *bytes) return GM_OK;
  *bytes = 0;
  HIP_TRY(buf.alloc(need));
  *bytes = need;
  return GM_OK;
}
static int ensure_scratch(gm_graph *g, size_t need) { return grow_dev(g->d_scratch, &g->scratch_bytes, need); }

// this rank's share of n units (gm_partition) as the first / step / count of a kernel's parameters; returns the count
template <class P>
static int64_t take_range(const LaunchCtx &c, int64_t n, P &p) {
  int64_t first = 0, step = 1, count = 0;
  gm_partition(n, c.rank, c.world, c.la.policy, &first, &step, &count);
  p.first = (decltype(p.first))first;
  p.step = (decltype(p.step))step;
  p.count = (decltype(p.count))count;
  return count;
}

// the CSR of a handle as the kernels see it (the optional tables stay nullptr: whoever needs one fills it in)
static GraphView graph_view(const gm_graph *g) {
  GraphView gv;
  gv.nv = g->nv;
  gv.ne = (int)g->ne;
  gv.rp = g->d_rp;
  gv.col = g->d_col;
  return gv;
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
  pl.use_tct = pl.pat == PAT_TC && !(la->tune[6] & GM_T6_TC_CHUNKED) && la->tune[5] != 1 && g->ne > 0 && !gm_sweep_env("GM_HOST_TABLES");
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
      else sup_stream = ensure_mean_sq_deg(g) == GM_OK && g->mean_sq_deg < (double)kSupStreamMaxMeanRow && ensure_tri_per_edge(g) == GM_OK &&
                        g->tri_per_edge < 0.5;
    }
    if ((sup_stream || !pl.support) && !(la->tune[6] & GM_T6_NO_KEYSTREAM)) {
      if (const int rc_k = ensure_keystream(g, pl.support, &pl.use_kst, !pl.support && !pl.tct_long)) return rc_k;  // (the triangle count: the hub corner may stay out, gm_ctc.hip)
    }
    if (!pl.use_kst) {
      if (const int rc_t = ensure_tasklists(g, pl.support)) return rc_t;
    }
  }
  if (pl.support && !pl.sup_part && !pl.wtri && !g->d_sup) HIP_TRY(g->d_sup.alloc(sizeof(unsigned) * (size_t)std::max<long long>(g->ne, 1)));
  // match masks instead of one atomic per streamed edge (gm_sup.hip): one GPU, the task lists, a topologically numbered DAG
  // (tune[6] & GM_T6_SUP_ATOMICS: A/B switch, every streamed edge by an atomic)
  if (pl.support && !pl.sup_part && !pl.wtri && world == 1 && pl.use_tct && !pl.use_kst && !(la->tune[6] & GM_T6_SUP_ATOMICS)) {
    if (const int rc_m = ensure_sup_masks(g)) return rc_m;
    pl.sup_masks = g->smask_state == 1;
  }
  setup_trace("run_pattern: task lists");
  // the hosts with rows of 1025 .. 2048 entries, on the 2048-entry kernel -- when a rank's share of them can fill the chip about twice: the two
  // launches follow each other on the stream, and the second waits for the first one's last chunk.  R-MAT-24 has 8.5 K such chunks with a
  // third of all keys: split / one table, ms per rank at world 1 / 2 / 4 / 8: TC 32.3 / 16.1 / 9.26 / 5.20 against 36.2 / 18.2 / 9.30 / 4.82,
  // edge supports - / 51.0 / 26.0 / 16.7 against - / 60.5 / 30.4 / 15.5 (profiles/r04/ab_split_stage.txt).  GM_TCT_SPLIT_ALWAYS: at every world.
  if (pl.split_stage) {
    RowFilter rb;
    rb.tct = (pl.use_kst && !pl.support && g->kst_skip_from < g->nv) ? 2 : 1;  // (2: priced from the stream without the hub corner, gm_tables.hip)
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
  pl.corner_from = pl.use_kst ? g->kst_skip_from : (pl.use_tct ? g->tl_skip_from : 0x7fffffff);  // the rows the stream / the task lists in use leave out
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
    const long long vlo = (long long)g->nv * rank / world, vhi = (long long)g->nv * (rank + 1) / world;
    auto first_chunk_at = [&](long long v) {
      long long lo = 0, hi = n;
      while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (tb->first_vertex[(size_t)mid] < v) lo = mid + 1; else hi = mid;
      }
      return lo;
    };
    first = first_chunk_at(vlo);
    count = first_chunk_at(vhi) - first;
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
  p.g.edesc = g->d_edesc;
  if (pl.use_tct) {
    p.g.trp = g->d_trp;
    p.g.tdesc = g->d_tdesc;
    p.g.tedge = pl.support ? g->d_tedge : nullptr;
    if (pl.sup_masks) {
      p.g.tmoff = g->d_tmoff;
      p.smask = g->d_smask;
    }
    // the triangle count streams the short lists from their task-major copies (gm_host.h d_colk; tune[6] & GM_T6_NO_KEYSTREAM: from their rows);
    // the edge supports need the entries of the streamed keys in col[] itself
    if (pl.use_kst && pl.support) {  // ... with the entries the supports need beside them (the second set when the stream was built without)
      p.g.kst = g->d_kst2 ? g->d_kst2 : g->d_kst;
      p.g.kst_rp = g->d_kst_rp;
      p.g.kst_et = g->d_kst_et;
      p.g.trp = g->d_trpl;
      p.g.tdesc = g->d_tdescl2 ? g->d_tdescl2 : g->d_tdescl;
      p.g.tedge = g->d_tedgel;
    } else if (pl.use_kst) {  // short lists as one tagged key stream, the longer ones as tasks
      p.g.kst = g->d_kst;
      p.g.kst_rp = g->d_kst_rp;
      p.g.trp = g->d_trpl;
      p.g.tdesc = g->d_tdescl;
    } else if (!pl.support && g->d_colk && g->d_tdesck && !(la->tune[6] & GM_T6_NO_KEYSTREAM)) {
      p.g.col = g->d_colk;
      p.g.tdesc = g->d_tdesck;
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
      const unsigned long long budget = (unsigned long long)(free_b + g->scratch_bytes) / 2ull;
      const unsigned long long fit = budget / std::max<unsigned long long>(slot_words * sizeof(unsigned), 1ull);
      if (fit == 0) {
        g_last_error = "k-clique: the bit-matrix of the longest DAG row (" + std::to_string(g->max_deg) + " entries) does not fit the device memory";
        return GM_ERR_TOO_LARGE;
      }
      if ((unsigned long long)r.grid > fit) r.grid = (int)fit;
    }
    const size_t need = (size_t)slot_words * sizeof(unsigned) * (size_t)r.grid;
    if (int rc = ensure_scratch(g, need)) return rc;
    p.scratch = g->d_scratch;
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
        const bool whole = r.e_begin == g->h_rp[r.u_begin] && r.e_end == g->h_rp[r.u_end];
        fprintf(f, "%zu,%zu,%d,%d,%d,%d,%d,%d,%llu,%.1f\n", pos, cid, r.u_end - r.u_begin, r.e_end - r.e_begin,
                g->h_rp[r.u_begin + 1] - g->h_rp[r.u_begin], (int)whole, r.part, r.nparts, tab->cost[cid], ticks[pos] / 100.0);
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
            r.u_begin, r.u_end, r.e_begin, r.e_end, r.e_end - r.e_begin, r.part, r.nparts, g->h_rp[r.u_begin + 1] - g->h_rp[r.u_begin]);
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
  HIP_TRY(hipMemsetAsync(g->d_wide_queue, 0, 65536, stream));
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
      cb.mat = g->d_wide_mat;
      cb.tri = g->d_cg_tri;
      cb.rowbase = g->d_cg_rowbase;
      cb.blk = g->d_cg_blk;
      cb.tab = rd.d_gtab;
      cb.units = rd.d_gunits;
      cb.items = rd.d_gitems;
      cb.delta = g->core_base & 31;
      cb.count = (int)rd.n_gitems;
      cb.queue = g->d_wide_queue + qword++;
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
      cg.mat = g->d_wide_mat;
      cg.core = g->d_core;
      cg.core_base = g->core_base;
      cg.core_words = (g->core_h + 31) / 32;
      cg.core_bytes = (unsigned long long)g->core_h * (unsigned long long)cg.core_words * 4ull;
      cg.first_slot = (int)rd.w0;
      cg.count = (int)(rd.w1 - rd.w0);
      cg.queue = g->d_wide_queue + qword++;
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
      pw.queue = g->d_wide_queue + qword++;
      pw.mat = g->d_wide_mat;
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
      cs.mat = g->d_wide_mat;
      cs.queue = g->d_wide_queue + qword++;
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
      c.mat = g->d_wide_mat;
      c.slots = plan->d_mcls_slots + rd.mcls_begin[cls];
      c.qrec = plan->d_mcls_rec + rd.mcls_begin[cls];
      c.count = (int)(rd.mcls_begin[cls + 1] - rd.mcls_begin[cls]);
      c.queue = g->d_wide_queue + qword++;
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
            plan->verts.size(), plan->n_count, nt, nh, plan->rounds.size(), g->wide_mat_bytes / 1048576.0, plan->stage, plan->topo ? "topological" : "arbitrary");
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
      q.scratch = g->d_scratch;  // (allocated before the timer started)
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
enum TaskKernel : int { TK_TC = 0, TK_SUPPORT = 1, TK_WTRI = 2 };
static int launch_task_tables(PatternRun &r, int kind) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  const MineParams &p = r.p;
  const WtriParams wp = {g->d_w5sup, g->d_w5ed, g->d_w5deg};
  auto launch = [&](const MineParams &q, int stage, long long dequeues) {
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
    cp.core = g->d_core;
    cp.row_words = (g->core_h + 31) / 32;
    // (a stream built with a choice of block pairs, tc_pairs_setup: the region they lie in and the list of their pieces)
    const bool pairs = pl.use_kst && g->tc_pair_region > 0;
    const int from = pairs ? g->tc_pair_from : pl.corner_from;
    cp.row0 = from - g->core_base;
    cp.word0 = cp.row0 >> 5;
    cp.h = g->nv - from;
    cp.ntasks = 0;
    if (pairs) {
      cp.tasks = g->d_tc_pair_tasks;
      cp.n_list = g->n_tc_pair_tasks;
    }
    if (int rc = launch_corner(r, cp, false)) return rc;
    // (gm_stats.tasks: a table's task edges are its rows' entries -- the corner's rows are chunks of the table like any other)
  }
  return GM_OK;
}

// edge supports: zero the supports, three increments per triangle, then sum C(t, 2): all inside the timed region
static int launch_supports(PatternRun &r, unsigned *sup_out) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  const int world = r.ctx.world, rank = r.ctx.rank;
  unsigned *sup = pl.sup_part ? sup_out : g->d_sup;
  HIP_TRY(hipMemsetAsync(sup, 0, sizeof(unsigned) * (size_t)(pl.sup_part ? diamond_support_entries(g->ne, world) : g->ne), stream));
  r.p.scratch = sup;
  if (int rc = launch_task_tables(r, TK_SUPPORT)) return rc;
  if (pl.tct_long && g->n_long_rows > 0) {
    SupLongParams sl;
    memset(&sl, 0, sizeof sl);
    sl.rp = g->d_rp;
    sl.col = g->d_col;
    sl.rows = g->d_long_rows;
    sl.prefix = g->d_long_prefix;
    sl.nrows = g->n_long_rows;
    sl.total = g->long_edges;
    sl.sup = sup;
    sl.topo = (g->topo_state == 1 && !gm_sweep_env("GM_TC_NO_TRIM")) ? 1 : 0;
    sl.rank = rank;
    sl.world = world;
    HIP_TRY(launch_sup_long(sl, g->cu_count, stream));
    r.my_edges += (unsigned long long)((g->long_edges - rank + world - 1) / world);
  }
  if (pl.sup_core) {  // the supports of the hub corner's edges: (A A)_ij on the matrix cores (gm_ctc.hip); a rank takes every world-th block
    CoreTcParams cp;
    memset(&cp, 0, sizeof cp);
    cp.core = g->d_csym;
    cp.h = g->tl_core_h;
    cp.row_words = cp.h / 32;
    cp.rp = g->d_rp;
    cp.base = pl.corner_from;
    cp.first_pos = g->d_cfirst;
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
    sc.emoff = g->d_emoff;
    sc.smask = g->d_smask;
    sc.sup = sup;
    sc.far_rows = g->d_sup_far_rows;
    sc.n_far_rows = g->n_sup_far_rows;
    HIP_TRY(launch_sup_cols(sc, g->cu_count, stream));
  }
  if (!pl.sup_part) HIP_TRY(launch_sup_pairs(sup, 0, g->ne, g->d_counters, g->cu_count, stream));
  return GM_OK;
}

// The 5-vertex closed forms on the DAG (gm_wtri.hip; gm_sgl5_raw filled g->d_w5sup and says what it wants): the per-entry sums and the
// scatter into 2 T_v, the support-weighted second pass over the triangles (A, B -> counters[0], [1]) -- the task tables, then the out-edges
// no task list holds: the rows beyond the stage or the rows of the hub corner -- and the per-vertex sums.  All inside the timed region.
static int launch_weighted(PatternRun &r) {
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  const PatternPlan &pl = r.pl;
  HIP_TRY(hipMemsetAsync(g->d_w5out, 0, 64, stream));
  HIP_TRY(hipMemsetAsync(g->d_w5tv2, 0, sizeof(unsigned long long) * (size_t)std::max(g->nv, 1), stream));
  WtriEntryParams ep;
  memset(&ep, 0, sizeof ep);
  ep.nv = g->nv; ep.ne = g->ne; ep.rp = g->d_rp; ep.col = g->d_col; ep.sup = g->d_w5sup; ep.deg = g->d_w5deg;
  ep.ed = g->d_w5ed; ep.tv2 = g->d_w5tv2; ep.out = g->d_w5out;
  HIP_TRY(launch_wtri_entries(ep, g->cu_count, stream));
  if (g->w5_tri) {
    if (int rc = launch_task_tables(r, TK_WTRI)) return rc;
    const WtriParams wp = {g->d_w5sup, g->d_w5ed, g->d_w5deg};
    WtriEdgeParams we;
    memset(&we, 0, sizeof we);
    we.rp = g->d_rp; we.col = g->d_col; we.nv = g->nv; we.ne = g->ne;
    we.topo = (g->topo_state == 1 && !gm_sweep_env("GM_TC_NO_TRIM")) ? 1 : 0;
    we.counters = g->d_counters;
    if (pl.tct_long && g->n_long_rows > 0) {
      we.rows = g->d_long_rows; we.prefix = g->d_long_prefix; we.nrows = g->n_long_rows; we.total = g->long_edges;
      HIP_TRY(launch_wtri_edges(we, wp, g->cu_count, stream));
    } else if (pl.corner_from < g->nv) {
      we.v0 = pl.corner_from; we.total = g->ne;
      HIP_TRY(launch_wtri_edges(we, wp, g->cu_count, stream));
    }
  }
  if (g->w5_vert) HIP_TRY(launch_wtri_vertices(g->nv, g->d_w5tv2, g->d_w5deg, g->d_w5out, g->cu_count, stream));
  return GM_OK;
}

int run_pattern(Pattern pat, const gm_graph *cg, const gm_launch *la, int k, uint64_t *h_out, int nout, gm_stats *st, int fin_mode,
                unsigned long long fin_base, unsigned *sup_out) {
  PatternRun r;
  PatternPlan &pl = r.pl;
  // edge supports + sum C(t, 2) (gm_sup.hip): the triangle pass of the task lists with another match handler -- everything up to the
  // launch is the triangle count's
  // (PAT_SUPPORT_PART: the share of a rank -- any world -- of the supports only, added into the caller's zeroed buffer: the ranks' arrays
  // are summed by a reduce-scatter and gm_diamond_support_finish takes sum C(t, 2) of a slice)
  pl.sup_part = pat == PAT_SUPPORT_PART;
  pl.wtri = pat == PAT_WTRI;  // (the weighted pass of the 5-vertex closed forms: the same tables and task lists, gm_wtri.hip)
  pl.support = pat == PAT_SUPPORT || pl.sup_part || pl.wtri;
  if (pl.sup_part && !sup_out) return GM_ERR_INVALID;
  pl.pat = pl.support ? PAT_TC : pat;
  if (fin_mode < 0) fin_mode = (pl.pat == PAT_MOTIF3) ? FIN_MOTIF3 : FIN_COPY;
  if (int rc = begin_launch(cg, la, h_out, r.ctx)) return rc;
  gm_graph *g = r.ctx.g;
  hipStream_t stream = r.ctx.stream;
  setup_trace("run_pattern: begin_launch");
  if (int rc = plan_pattern(r.ctx, pl)) return rc;
  setup_trace("run_pattern: tables / plan");
  if (int rc = fill_mine_params(r, k)) return rc;
  if (int rc = prepare_scratch(r, k)) return rc;
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
  if (pl.wtri) rc = launch_weighted(r);
  else if (pl.support) rc = launch_supports(r, sup_out);
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
  return end_launch(r.ctx, fin_mode, fin_base, h_out, nout, st);
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
  if (self->mean_sq_deg < 0) {
    HIP_TRY(hipSetDevice(self->device));
    DevOwn<unsigned long long> d_s;
    unsigned long long s2 = 0;
    HIP_TRY(d_s.alloc(8));
    hipError_t e = hipMemset(d_s, 0, 8);
    if (e == hipSuccess && self->nv > 0)
      hipLaunchKernelGGL(sum_sq_deg_kernel, dim3((unsigned)std::min<long long>(((long long)self->nv + 255) / 256, 2048)), dim3(256), 0, 0, self->nv, self->d_rp, d_s);
    if (e == hipSuccess) e = hipMemcpy(&s2, d_s, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "sum_sq_deg_kernel", __FILE__, __LINE__);
    self->mean_sq_deg = self->ne > 0 ? (double)s2 / (double)self->ne : 0.0;
  }
  return GM_OK;
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
  if (self->tri_per_edge < 0) {
    HIP_TRY(hipSetDevice(self->device));
    const int nsamples = (int)std::min<long long>(1 << 16, std::max<long long>(self->ne, 1));
    const long long stride = std::max<long long>(1, self->ne / nsamples);
    DevOwn<unsigned long long> d_s;
    unsigned long long s = 0;
    HIP_TRY(d_s.alloc(8));
    hipError_t e = hipMemset(d_s, 0, 8);
    if (e == hipSuccess && self->ne > 0)
      hipLaunchKernelGGL(tri_sample_kernel, dim3((unsigned)((nsamples + 255) / 256)), dim3(256), 0, 0, self->nv, (long long)self->ne, self->d_rp, self->d_col, stride,
                         nsamples, d_s);
    if (e == hipSuccess) e = hipMemcpy(&s, d_s, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "tri_sample_kernel", __FILE__, __LINE__);
    self->tri_per_edge = (double)s / (double)nsamples;
  }
  return GM_OK;
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
  if (ensure_mean_sq_deg(g) == GM_OK) keys = (double)g->ne * g->mean_sq_deg * 0.5;
  const double cap = keys / (3000.0 * (double)std::max(world, 1));
  return (unsigned long long)std::min(std::max(cap, (double)(128 << 10)), (double)(4 << 20));
}

static int topo_view(const gm_graph *dag, const gm_launch *la, gm_graph **run_on) {
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
  if (gm_sweep_env("GM_TABLE_INFO")) fprintf(stderr, "[topo view] sum d+^2 / |E+| = %.1f (switch at %.1f)\n", self->mean_sq_deg, min_row);
  if (self->mean_sq_deg < min_row) return GM_OK;  // short lists: as numbered
  return get_relabeled(self, 2, run_on);
}

static int run_tc(const gm_graph *dag, const gm_launch *la, uint64_t *out, int nout, gm_stats *st, int fin_mode = -1, unsigned long long fin_base = 0) {
  gm_graph *run_on = nullptr;
  int rc = topo_view(dag, la, &run_on);
  if (rc) return rc;
  rc = run_pattern(PAT_TC, run_on, la, 3, out, nout, st, fin_mode, fin_base);
  const_cast<gm_graph *>(dag)->ring_alias = (run_on != dag) ? run_on : nullptr;
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
  const bool on = run_on->kst_skip_from < run_on->nv;
  const long long nJ = on ? (run_on->tc_core_h + 63) >> 6 : 0;
  info[0] = on ? run_on->tc_core_h : 0;           // vertices of the corner (0: every edge is a task of the key stream)
  info[1] = on ? run_on->tc_core_edges : 0;       // DAG entries inside it
  info[2] = nJ * (nJ + 1) / 2;                    // 64 x 64 blocks of the masked product
  info[3] = on ? run_on->core_h : 0;              // vertices of the core bitmap the corner is a part of
  return GM_OK;
}

// ... and the block pairs of it the product takes (tc_pairs_setup, gm_tables.hip): info[0] = rows of the region (0: no selection -- the full
// triangle of gm_tc_core_info's corner, or none), [1] = pairs taken, [2] = pairs that hold keys, [3] = DAG entries in the product,
// [4] = keys of the stream's model that left the stream, [5] = R of the rule
extern "C" int gm_tc_pairs_info(const gm_graph *dag, int64_t info[6]) {
  if (!dag || !info) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  const int rc = topo_view(dag->dag_cache ? dag->dag_cache : dag, nullptr, &run_on);
  if (rc) return rc;
  const bool on = run_on->kst_skip_from < run_on->nv && run_on->tc_pair_region > 0;
  for (int i = 0; i < 6; ++i) info[i] = on ? run_on->tc_pair_info[i] : 0;
  return GM_OK;
}

constexpr unsigned long long kHeavyCentre = 1ull << 15;  // 2-paths above which a centre of the map kernels gets a whole workgroup (emit_centre_tasks, gm_centre_plan.h)
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
static int build_centre_tasks(gm_graph *g, WorkLaunch work_launch, const char *what, DevOwn<int4> &d_tasks, unsigned long long *n_tasks) {
  if (d_tasks) return GM_OK;
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
  DevOwn<int4> d;
  if (int rc = upload(d, tasks)) return rc;
  *n_tasks = tasks.size();
  d_tasks = std::move(d);  // (the list is what says "built": handed over whole)
  return GM_OK;
}

// rectangle, flattened over wedges (rect_flat_kernel in gm_mine.hip)
static int ensure_idx0(gm_graph *g, const GraphView &gv) {
  if (g->d_idx0) return GM_OK;
  OtherSetupScope scope(g);
  DevOwn<int> idx0;
  HIP_TRY(idx0.alloc(sizeof(int) * (size_t)std::max(g->nv, 1)));
  HIP_TRY(launch_idx0(gv, idx0, 0));
  g->d_idx0 = std::move(idx0);
  return GM_OK;
}

static int run_rect_flat(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st, bool pentagon = false) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  const GraphView gv = graph_view(g);
  if (!g->d_wblock_prefix) {  // once per graph: idx0[v] on the device, wedge-block prefix on the host
    OtherSetupScope scope(g);
    rc = ensure_idx0(g, gv);
    if (rc) return rc;
    std::vector<int> idx0((size_t)std::max(g->nv, 1));
    HIP_TRY(hipMemcpy(idx0.data(), g->d_idx0, sizeof(int) * (size_t)g->nv, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> pre((size_t)g->nv + 1);
    unsigned long long acc = 0;
    for (int v = 0; v < g->nv; ++v) {
      pre[v] = acc;
      const unsigned long long n = (unsigned long long)idx0[v];
      acc += (n * (n - (n ? 1ull : 0ull)) / 2ull + 63ull) / 64ull;
    }
    pre[g->nv] = acc;
    g->n_wblocks = acc;
    DevOwn<unsigned long long> d_pre;
    HIP_TRY(d_pre.alloc(sizeof(unsigned long long) * ((size_t)g->nv + 1)));
    HIP_TRY(hipMemcpy(d_pre, pre.data(), sizeof(unsigned long long) * ((size_t)g->nv + 1), hipMemcpyHostToDevice));
    g->d_wblock_prefix = std::move(d_pre);
  }
  RectParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.idx0 = g->d_idx0;
  p.block_prefix = g->d_wblock_prefix;
  p.nblocks = g->n_wblocks;
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
  pl.ready = true;
  return GM_OK;
}
static int max_lds_ranges(int limit) {
  const char *e = gm_opt("GM_RECT_LDS_RANGES");
  return e ? std::max(1, std::min(limit, std::atoi(e))) : limit;
}
// rectangle: the 2-path ends in the last ranges of ids (at most kRectLdsRanges) of the centres with >= GM_RECT_LDS_MIN 2-paths are counted in
// LDS maps (rect_lds_kernel): the ranges, the row bounds, the (centre, range) tasks, rect_acc_kernel's list with those centres in front
static int ensure_rect_plan(gm_graph *g, const GraphView &gv) {
  if (g->rect_plan.ready) return GM_OK;
  OtherSetupScope scope(g);
  const size_t nv = (size_t)g->nv;
  unsigned long long lds_min = 4096;
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
  RectLdsRanges rr{};  // (whatever the numbering: tune[6] & GM_T6_AS_NUMBERED runs on the graph as given)
  rr.n = rect_lds_ranges((long long)g->nv, bmax, kRectLdsWords, max_lds_ranges(kRectLdsRanges), rr.rb, rr.lb);
  setup_trace("rect: ranges");
  CentrePlan pl;
  pl.cut = rr.rb[0];
  pl.bnd_stride = rr.n + 1;
  HIP_TRY(pl.d_bnd.alloc(sizeof(int) * (size_t)pl.bnd_stride * std::max<size_t>(nv, 1)));
  std::vector<unsigned long long> est;  // (both estimates: [0, nv) all ends, [nv, 2 nv) the ends below the cut)
  if (nv) HIP_TRY(launch_rect_bounds(gv, rr, pl.d_bnd, 0));
  if (int rc = centre_estimates(nv, 2, [&](unsigned long long *d_work) { return launch_rect_work_cut(gv, g->d_idx0, pl.d_bnd, pl.bnd_stride, d_work, 0); }, "rect_work_cut_kernel", est)) return rc;
  setup_trace("rect: bounds + work estimates");
  std::vector<int> idx0h(std::max<size_t>(nv, 1));
  if (nv) HIP_TRY(hipMemcpy(idx0h.data(), g->d_idx0, sizeof(int) * nv, hipMemcpyDeviceToHost));
  const CentreTasks tasks = plan_rect_tasks(nv, est.data(), est.data() + nv, idx0h.data(), rr.rb, rr.n, lds_min, kRectLdsWaves * GM_WAVE, kHeavyCentre);
  if (int rc = upload_centre_tasks(tasks, pl)) return rc;
  g->rect_ranges = rr, g->rect_plan = std::move(pl);
  setup_trace("rect: task lists");
  return GM_OK;
}
// house: the same with ranges of kHouseLdsIds ids (at most kHouseLdsRanges) and plan_house_tasks' policy (GM_HOUSE_WALK_MIN: its 2-paths per walk)
static int ensure_house_plan(gm_graph *g, const GraphView &gv) {
  if (g->house_plan.ready) return GM_OK;
  OtherSetupScope scope(g);
  const size_t nv = (size_t)g->nv;
  const char *lds_min_given = gm_opt("GM_RECT_LDS_MIN");
  const unsigned long long lds_min = lds_min_given ? std::strtoull(lds_min_given, nullptr, 10) : 4096;
  HouseLdsRanges rr = {0, 0, g->nv};
  rr.n = house_lds_ranges((long long)g->nv, kHouseLdsIds, max_lds_ranges(kHouseLdsRanges), &rr.cut);
  CentrePlan pl;
  pl.cut = rr.cut;
  pl.bnd_stride = rr.n + 1;
  HIP_TRY(pl.d_bnd.alloc(sizeof(int) * (size_t)pl.bnd_stride * std::max<size_t>(nv, 1)));
  std::vector<unsigned long long> est;
  if (nv) HIP_TRY(launch_house_bounds(gv, rr, pl.d_bnd, 0));
  if (int rc = centre_estimates(nv, 2, [&](unsigned long long *d_work) { return launch_house_work_cut(gv, pl.d_bnd, pl.bnd_stride, d_work, 0); }, "house_work_cut_kernel", est)) return rc;
  std::vector<int> deg(nv + 1, 0);  // (the offsets, then their differences)
  if (nv) HIP_TRY(hipMemcpy(deg.data(), g->d_rp, sizeof(int) * (nv + 1), hipMemcpyDeviceToHost));
  for (size_t v = 0; v < nv; ++v) deg[v] = deg[v + 1] - deg[v];
  unsigned long long per_walk = 200;
  if (const char *e = gm_sweep_env("GM_HOUSE_WALK_MIN")) per_walk = std::strtoull(e, nullptr, 10);
  const CentreTasks tasks = plan_house_tasks(nv, est.data(), est.data() + nv, deg.data(), rr.n, lds_min, lds_min_given != nullptr, per_walk, kRectLdsWaves * GM_WAVE, kHeavyCentre);
  if (int rc = upload_centre_tasks(tasks, pl)) return rc;
  g->house_ranges = rr, g->house_plan = std::move(pl);
  return GM_OK;
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
static int run_rect_acc(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st, bool pentagon = false) {
  LaunchCtx ctx;
  int rc = begin_launch(cg, la_in, h_out, ctx);
  if (rc) return rc;
  gm_graph *g = ctx.g;
  const gm_launch *la = &ctx.la;
  const GraphView gv = graph_view(g);
  rc = ensure_idx0(g, gv);
  if (rc) return rc;
  const bool lds_maps = !pentagon && !(la->tune[6] & GM_T6_GLOBAL_MAPS);
  if (!lds_maps) rc = build_centre_tasks(g, [&](unsigned long long *d_work) { return launch_rect_work(gv, g->d_idx0, d_work, 0); }, "rect_work_kernel", g->d_rect_tasks, &g->n_rect_tasks);
  if (rc) return rc;
  setup_trace("rect: idx0 / old tasks");
  if (lds_maps && (rc = ensure_rect_plan(g, gv))) return rc;
  RectAccParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.idx0 = g->d_idx0;
  p.tasks = g->d_rect_tasks;
  if (lds_maps) acc_params_from_plan(p, g->rect_plan);
  const int64_t count = take_range(ctx, (int64_t)(lds_maps ? g->rect_plan.n_acc_tasks : g->n_rect_tasks), p);
  p.counters = g->d_counters;
  p.queue = queue_word64(g, QW64_MAIN);
  // (with the heavy centres in LDS what is left for the global maps is light: 1 / 2 / 4 / 8 workgroups per CU measured 11.15 / 10.95 /
  // 11.1 / 11.0 ms for the rectangle of R-MAT-20 -- two, so that a first call does not allocate 2 x 32 GB of maps and lists)
  int acc_wgs_per_cu = lds_maps ? 2 : 8;
  if (const char *e = gm_sweep_env("GM_RECT_ACC_WGS")) acc_wgs_per_cu = std::max(1, std::atoi(e));
  size_t need = 0;
  const int grid = map_grid(g, count, p, 4, 4, acc_wgs_per_cu, g->rect_acc_bytes, &need);
  if (need > g->rect_acc_bytes) {
    if (int rc_a = grow_dev(g->d_rect_acc, &g->rect_acc_bytes, need)) return rc_a;
    HIP_TRY(hipMemset(g->d_rect_acc, 0, need));  // every launch leaves the maps zeroed again
  }
  p.acc = g->d_rect_acc;
  // touched-vertex lists: same shape as the maps (one int list of up to nv entries per wave)
  if (int rc_t = grow_dev(g->d_pent_touched, &g->pent_touched_bytes, need)) return rc_t;
  p.touched = g->d_pent_touched;
  setup_trace("rect: global maps");
  if (pentagon) {
    rc = ensure_edge_tables(g, gv);
    if (rc) return rc;
    PentAccParams q;
    memset(&q, 0, sizeof q);
    q.g = gv;
    q.idx0 = g->d_idx0;
    q.tlt = g->d_house_tlt;
    q.tasks = p.tasks;
    q.first = p.first;
    q.step = p.step;
    q.count = p.count;
    q.acc = p.acc;
    q.touched = g->d_pent_touched;
    q.acc_stride = p.acc_stride;
    q.queue = p.queue;
    q.counters = p.counters;
    if (int rc_t = start_timer(ctx)) return rc_t;
    if (count > 0) HIP_TRY(launch_pent_acc(q, grid, ctx.stream));
    fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)count, grid, 256);
    return end_launch(ctx, FIN_HALF_SIGNED, 0, h_out, 1, st);
  }
  RectLdsParams lp{};
  lp.idx0 = g->d_idx0;
  const int64_t lcount = lds_maps ? lds_params_from_plan(lp, ctx, gv, g->rect_plan, g->rect_ranges) : 0;
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
  if (g->d_house_t && g->d_house_tlt) return GM_OK;
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
  g->d_house_t.take(t);  // (published only after the build kernel has succeeded; the buffers free themselves on the error paths)
  g->d_house_tlt.take(tlt);
  return GM_OK;
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
  rc = lds_maps ? ensure_house_plan(g, gv) : build_centre_tasks(g, [&](unsigned long long *d_work) { return launch_house_work(gv, d_work, 0); }, "house_work_kernel", g->d_house_tasks, &g->n_house_tasks);
  if (rc) return rc;
  HouseAccParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.t = g->d_house_t;
  p.tlt = g->d_house_tlt;
  p.tasks = g->d_house_tasks;
  if (lds_maps) acc_params_from_plan(p, g->house_plan);
  const int64_t count = take_range(ctx, (int64_t)(lds_maps ? g->house_plan.n_acc_tasks : g->n_house_tasks), p);
  p.counters = g->d_counters;
  p.queue = queue_word64(g, QW64_MAIN);
  size_t need = 0;
  const int grid = map_grid(g, count, p, 8, 3, lds_maps ? 4 : 8, g->house_acc_bytes, &need);
  if (need > g->house_acc_bytes) {
    g->house_acc_bytes = 0;
    HIP_TRY(g->d_house_acc.alloc(need));
    HIP_TRY(hipMemset(g->d_house_acc, 0, need));  // every launch leaves the maps zeroed again
    HIP_TRY(g->d_house_touched.alloc(need / 2));  // one int list per map
    g->house_acc_bytes = need;
  }
  p.acc = g->d_house_acc;
  p.touched = g->d_house_touched;
  HouseLdsParams lp{};
  lp.t = g->d_house_t;
  const int64_t lcount = lds_maps ? lds_params_from_plan(lp, ctx, gv, g->house_plan, g->house_ranges) : 0;
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
  if (!g->d_house_prefix) {  // once per graph: blocks per entry on the device, prefix on the host
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
    g->n_house_blocks = acc;
    DevOwn<unsigned long long> d_pre;
    HIP_TRY(d_pre.alloc(sizeof(unsigned long long) * (ne + 1)));
    HIP_TRY(hipMemcpy(d_pre, pre.data(), sizeof(unsigned long long) * (ne + 1), hipMemcpyHostToDevice));
    g->d_house_prefix = std::move(d_pre);
  }
  HouseParams p;
  memset(&p, 0, sizeof p);
  p.g = gv;
  p.entry_prefix = g->d_house_prefix;
  p.nblocks = g->n_house_blocks;
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
    p.scratch = reinterpret_cast<int *>(g->d_scratch.get());
  }
  if (int rc_t = start_timer(ctx)) return rc_t;
  if (count > 0) HIP_TRY(launch_sgl_nested(pat, p, grid, ctx.stream));
  fill_stats(st, (uint64_t)(g->ne / 2 / ctx.world), (uint64_t)count, grid, 256);
  return end_launch(ctx, FIN_COPY, 0, h_out, 1, st);
}

// The oriented copy of a symmetric handle (gm_graph_orient), built once under its own lock: two solvers called on the same handle from two
// threads -- the formula 3-motif and the one-GPU diamond share it -- must not both orient and leak a handle.  A graph of
// >= 2^31 entries too: its oriented copy must fit the 32-bit task index, gm_graph_orient checks.
static int ensure_dag_cache(gm_graph *g) {
  std::lock_guard<std::mutex> lk(g->dag_mu);
  if (g->dag_cache) return GM_OK;
  gm_graph *dag = nullptr;
  const int rc = gm_graph_orient(g, &dag);
  if (rc) return rc;
  dag->pool_owner = g;
  g->dag_cache = dag;
  return GM_OK;
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
  rc = run_pattern(PAT_SUPPORT, run_on, la, 3, total, 1, st);
  if (rc) return rc;
  dag->ring_alias = (run_on != dag) ? run_on : nullptr;
  g->ring_alias = dag;
  g->ring_extra[0] = g->ring_extra[1] = nullptr;
  return GM_OK;
}

// ---- diamond on several ranks: ONE shared pass over the triangles (the one-GPU algorithm at every N) --------------------------------------
// Every rank runs its share of the triangle pass into its own zeroed support array (one uint32 per entry of the oriented copy, padded so
// that every rank gets the same number of entries), the arrays are summed by ONE reduce-scatter over xGMI (ncclReduceScatter, ncclUint32,
// ncclSum: rank r receives the entries [r n / world, (r + 1) n / world)), every rank takes sum C(t, 2) of its slice, and the 64-bit
// counts meet in the usual all-reduce.  The reference has no multi-GPU diamond at all (src/sgl/multigpu.cu:117 is commented out).
static int diamond_run_on(const gm_graph *sym, const gm_launch *la, gm_graph **run_on) {
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
  info[0] = run_on->smask_state == 1 ? (int64_t)run_on->smask_words : 0;  // 64-bit words of the match-mask arena (0: no masks)
  info[1] = (int64_t)at;                                                  // increments issued as global atomics from the waves' queues
  info[2] = run_on->smask_state == 1 ? (int64_t)run_on->n_sup_far_rows : 0;
  info[3] = (int64_t)sup_mask_min_tail(run_on);
  return GM_OK;
}
// tooling: the hub corner whose supports the one-GPU diamond of this handle takes on the matrix cores (after a first diamond)
extern "C" int gm_sup_core_info(const gm_graph *sym, int64_t info[4]) {
  if (!sym || !info) return GM_ERR_INVALID;
  gm_graph *run_on = nullptr;
  const int rc = diamond_run_on(sym, nullptr, &run_on);
  if (rc) return rc;
  const bool on = run_on->tl_skip_from < run_on->nv;
  const long long nb = on ? run_on->tl_core_h >> 8 : 0;
  info[0] = on ? run_on->tl_core_h : 0;  // vertices of the corner (0: every edge's support comes from the triangle pass)
  info[1] = 0;
  if (on) {
    int e0 = 0;
    HIP_TRY(hipSetDevice(run_on->device));
    HIP_TRY(hipMemcpy(&e0, run_on->d_rp + run_on->tl_skip_from, sizeof(int), hipMemcpyDeviceToHost));
    info[1] = run_on->ne - (long long)e0;  // DAG entries inside it
  }
  info[2] = nb * (nb + 1) / 2;           // pairs of 256-row blocks of the product
  info[3] = on ? (run_on->tl_core_h >> 9) : 0;  // 512-column chunks of a row
  return GM_OK;
}
extern "C" int gm_diamond_support_partial(const gm_graph *sym, const gm_launch *la, uint32_t *d_support, int64_t n_entries, gm_stats *st) {
  if (!d_support) return GM_ERR_INVALID;
  gm_graph *g = const_cast<gm_graph *>(sym), *run_on = nullptr;
  int rc = diamond_run_on(sym, la, &run_on);
  if (rc) return rc;
  const int world = (la && la->world > 1) ? la->world : 1;
  // (at least gm_diamond_support_size; the ranks' slices are cut from THAT size -- size / world entries each -- whatever the buffer holds beyond it)
  if (n_entries < diamond_support_entries(run_on->ne, world)) return GM_ERR_INVALID;
  uint64_t dummy = 0;
  rc = run_pattern(PAT_SUPPORT_PART, run_on, la, 3, (la && la->d_counts) ? nullptr : &dummy, 1, st, -1, 0, d_support);
  if (rc) return rc;
  gm_graph *dag = g->dag_cache;
  dag->ring_alias = (run_on != dag) ? run_on : nullptr;
  g->ring_alias = dag;
  g->ring_extra[0] = g->ring_extra[1] = nullptr;
  return GM_OK;
}
extern "C" int gm_diamond_support_finish(const gm_graph *sym, const gm_launch *la, const uint32_t *d_support, int64_t count, uint64_t *total, gm_stats *st) {
  if (!d_support || count < 0) return GM_ERR_INVALID;
  gm_graph *g = const_cast<gm_graph *>(sym), *run_on = nullptr;
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
  gm_graph *dag = g->dag_cache;
  dag->ring_alias = (run_on != dag) ? run_on : nullptr;
  g->ring_alias = dag;
  g->ring_extra[0] = g->ring_extra[1] = nullptr;
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
  const int rc = run_pattern(PAT_MOTIF4E, sym, la, 4, raw, 4, st, FIN_RAW4, 0);
  if (rc) return rc;
  const_cast<gm_graph *>(sym)->ring_alias = nullptr;
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
  std::lock_guard<std::mutex> lk(g->mu);
  if (g->d_w5out) return GM_OK;
  HIP_TRY(hipSetDevice(g->device));
  const size_t ne = (size_t)std::max<long long>(g->ne, 1), nv = (size_t)std::max(g->nv, 1);
  if (!g->d_w5sup) HIP_TRY(g->d_w5sup.alloc(sizeof(unsigned) * (size_t)diamond_support_entries(g->ne, 1)));
  if (!g->d_w5ed) HIP_TRY(g->d_w5ed.alloc(sizeof(unsigned) * ne));
  if (!g->d_w5tv2) HIP_TRY(g->d_w5tv2.alloc(sizeof(unsigned long long) * nv));
  if (!g->d_w5deg) {
    HIP_TRY(g->d_w5deg.alloc(sizeof(int) * nv));
    HIP_TRY(launch_wtri_degrees(g->nv, g->ne, g->d_rp, g->d_col, g->d_w5deg, g->cu_count, 0));
    HIP_TRY(hipDeviceSynchronize());
  }
  HIP_TRY(g->d_w5out.alloc(64));
  return GM_OK;
}

// one kernel of the symmetric graph that leaves ONE sum in counters[0] (P, Q): a launch of its own on the handle
template <class Launch>
static int run_sym_sum(const gm_graph *sym, const gm_launch *la, uint64_t *out, double *ms, Launch launch) {
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, la, out, ctx)) return rc;
  if (int rc = start_timer(ctx)) return rc;
  if (int rc = launch(ctx)) return rc;
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_COPY, 0, out, 1, &s)) return rc;
  *ms += s.kernel_ms;
  return GM_OK;
}

// the raw sums of the bit mask `needs` (gm_sgl5_raw: those of a pattern; gm_sgl6_raw: D, B, K4, or T for the arrays of the pass alone)
static int sgl5_raw_needs(const gm_graph *sym, unsigned needs, const gm_launch *la, uint64_t raw[GM_SGL5_NRAW], gm_stats *st) {
  if (!sym || !raw || !needs) return GM_ERR_INVALID;
  for (int i = 0; i < GM_SGL5_NRAW; ++i) raw[i] = 0;
  if (int rc0 = reject_big(sym)) return rc0;
  // the divisions and halvings need the sums of the whole graph, and the total is put together on the host: one rank, synchronous
  if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2;
  memset(&l2, 0, sizeof l2);
  if (la) l2 = *la;
  auto need = [&](int i) { return (needs >> i & 1u) != 0; };
  double ms = 0.0;
  gm_stats s;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  if (sym->ne == 0) return GM_OK;
  if (need(R5_T) || need(R5_D) || need(R5_W) || need(R5_A) || need(R5_B) || need(R5_H) || need(R5_S)) {
    // the supports of every entry of the oriented copy, filled like a one-rank gm_diamond_support_partial (rows beyond the stage through
    // sup_long_kernel), into an array of the 5-vertex forms' own; then the sums over entries, triangles and vertices
    gm_graph *run_on = nullptr;
    if (int rc = diamond_run_on(sym, &l2, &run_on)) return rc;
    if (int rc = ensure_w5_buffers(run_on)) return rc;
    uint64_t dummy = 0, ab[4] = {0, 0, 0, 0};
    memset(&s, 0, sizeof s);
    if (int rc = run_pattern(PAT_SUPPORT_PART, run_on, &l2, 3, &dummy, 1, &s, -1, 0, run_on->d_w5sup)) return rc;
    ms += s.kernel_ms;
    run_on->w5_tri = need(R5_A) || need(R5_B);
    run_on->w5_vert = need(R5_H) || need(R5_S);
    memset(&s, 0, sizeof s);
    if (int rc = run_pattern(PAT_WTRI, run_on, &l2, 3, ab, 4, &s, FIN_RAW4, 0)) return rc;
    ms += s.kernel_ms;
    unsigned long long o[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(o, run_on->d_w5out, sizeof o, hipMemcpyDeviceToHost));  // (run_pattern has synchronised the stream)
    const uint64_t v[7] = {o[0] / 3ull, o[1], o[2], ab[0], ab[1], o[3], o[4]};
    const int at[7] = {R5_T, R5_D, R5_W, R5_A, R5_B, R5_H, R5_S};
    for (int i = 0; i < 7; ++i)
      if (need(at[i])) raw[at[i]] = v[i];
  }
  if (need(R5_K4)) {
    if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;
    memset(&s, 0, sizeof s);
    if (int rc = gm_clique(g->dag_cache, 4, &l2, &raw[R5_K4], &s)) return rc;
    ms += s.kernel_ms;
  }
  if (need(R5_R)) {
    memset(&s, 0, sizeof s);
    if (int rc = gm_sgl(sym, "rectangle", &l2, &raw[R5_R], &s)) return rc;
    ms += s.kernel_ms;
  }
  if (need(R5_P)) {
    if (int rc = run_sym_sum(sym, &l2, &raw[R5_P], &ms, [&](LaunchCtx &c) {
          HIP_TRY(launch_path5(g->nv, g->d_rp, g->d_col, g->d_counters, g->cu_count, c.stream));
          return (int)GM_OK;
        })) return rc;
  }
  if (need(R5_Q)) {
    const int grid = chouse_grid(g->ne, g->cu_count);
    if (int rc = ensure_scratch(g, sizeof(int) * (size_t)grid * 4 * (size_t)std::max(g->max_deg, 1))) return rc;
    if (int rc = run_sym_sum(sym, &l2, &raw[R5_Q], &ms, [&](LaunchCtx &c) {
          ChouseParams cp;
          memset(&cp, 0, sizeof cp);
          cp.nv = g->nv; cp.ne = g->ne; cp.rp = g->d_rp; cp.col = g->d_col;
          cp.scratch = reinterpret_cast<int *>(g->d_scratch.get()); cp.max_deg = std::max(g->max_deg, 1); cp.out = g->d_counters;
          HIP_TRY(launch_chouse(cp, grid, c.stream));
          return (int)GM_OK;
        })) return rc;
  }
  g->ring_alias = nullptr;
  g->ring_extra[0] = g->ring_extra[1] = nullptr;
  if (st) st->kernel_ms = ms;
  return GM_OK;
}

extern "C" int gm_sgl5_raw(const gm_graph *sym, const char *pattern, const gm_launch *la, uint64_t raw[GM_SGL5_NRAW], gm_stats *st) {
  if (!sym || !pattern || !raw) return GM_ERR_INVALID;
  return sgl5_raw_needs(sym, strcmp(pattern, "all") == 0 ? (1u << GM_SGL5_NRAW) - 1u : sgl5_needs(pattern), la, raw, st);
}

// ---- local counts and the k-truss (gm_local.hip; DESIGN.md "Local counts and k-truss") ----------------------------------------------------
// the arrays of the symmetric handle, in the caller's entry order (peel: also the marks, the frontier list and the round counters)
static int ensure_local_buffers(gm_graph *g, bool peel, bool truss) {
  std::lock_guard<std::mutex> lk(g->mu);
  HIP_TRY(hipSetDevice(g->device));
  const size_t ne = (size_t)std::max<long long>(g->ne, 1);
  if (!g->d_lent) HIP_TRY(g->d_lent.alloc(sizeof(unsigned) * ne));
  if (peel) {
    if (!g->d_lrev) HIP_TRY(g->d_lrev.alloc(sizeof(int) * ne));
    if (!g->d_lmark) HIP_TRY(g->d_lmark.alloc(ne));
    if (!g->d_lfront) HIP_TRY(g->d_lfront.alloc(sizeof(int) * (ne / 2 + 1)));
    if (!g->d_lcnt) HIP_TRY(g->d_lcnt.alloc(64));
  }
  if (truss && !g->d_ltruss) HIP_TRY(g->d_ltruss.alloc(sizeof(unsigned) * ne));
  return GM_OK;
}

// the refusals the three calls share, in the order of the header
static int local_refusals(const gm_graph *sym, const gm_launch *la) {
  if (!sym) return GM_ERR_INVALID;
  if (int rc = reject_big(sym)) return rc;
  if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;  // (the arrays are whole-graph results, read back by the call)
  return GM_OK;
}

// The supports of every entry of the oriented copy -- one rank's PAT_SUPPORT_PART into run_on->d_lsup, every path of the triangle pass --
// and their way back: `c` is the open launch on the SYMMETRIC handle, the mapping kernel writes `out` (caller's entry order) and adds the
// sum of the supports to its counters[0].
static int local_supports(gm_graph *g, const gm_launch *l2, double *ms, gm_graph **run_on_out) {
  gm_graph *run_on = nullptr;
  if (int rc = diamond_run_on(g, l2, &run_on)) return rc;
  {
    std::lock_guard<std::mutex> lk(run_on->mu);
    if (!run_on->d_lsup) HIP_TRY(run_on->d_lsup.alloc(sizeof(unsigned) * (size_t)diamond_support_entries(run_on->ne, 1)));
  }
  uint64_t dummy = 0;
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = run_pattern(PAT_SUPPORT_PART, run_on, l2, 3, &dummy, 1, &s, -1, 0, run_on->d_lsup)) return rc;
  *ms += s.kernel_ms;
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
  mp.drp = run_on->d_rp; mp.dcol = run_on->d_col; mp.dsup = run_on->d_lsup;
  mp.topo = run_on->topo_state == 1 ? 1 : 0;
  mp.out = out; mp.sum = g->d_counters;
  HIP_TRY(launch_local_map(mp, g->cu_count, c.stream));
  return GM_OK;
}

extern "C" int gm_tc_local(const gm_graph *sym, const gm_launch *la, uint64_t *d_vertex_tri, uint32_t *d_entry_sup, uint64_t *total, gm_stats *st) {
  if (int rc = local_refusals(sym, la)) return rc;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2;
  memset(&l2, 0, sizeof l2);
  if (la) l2 = *la;
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
  double ms = 0.0;
  gm_graph *run_on = nullptr;
  if (int rc = local_supports(g, &l2, &ms, &run_on)) return rc;
  HIP_TRY(hipMemsetAsync(g->d_counters, 0, kCounterBlockBytes, ctx.stream));  // (a first call oriented the graph since begin_launch)
  if (int rc = start_timer(ctx)) return rc;
  unsigned *ent = d_entry_sup ? d_entry_sup : g->d_lent;
  if (int rc = local_map(ctx, run_on, ent)) return rc;
  if (d_vertex_tri) HIP_TRY(launch_local_vertices(g->nv, g->d_rp, ent, (unsigned long long *)d_vertex_tri, g->cu_count, ctx.stream));
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_COPY, 0, &sum, 1, &s)) return rc;
  if (total) *total = sum / 6ull;  // sum_e t(e) over both directions = 2 sum_v T_v = 6 T
  if (st) st->kernel_ms = ms + s.kernel_ms;
  return GM_OK;
}

// gm_ktruss (decompose = false) and gm_truss_decompose: the supports in the caller's order, then whole-frontier rounds.  One 8-byte word
// comes back per round: the frontier's size and the smallest support that stays alive.
static int run_truss(const gm_graph *sym, bool decompose, int k_in, const gm_launch *la, uint32_t *d_out, uint64_t *n_edges, int32_t *k_max,
                     int32_t *rounds_out, gm_stats *st) {
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2;
  memset(&l2, 0, sizeof l2);
  if (la) l2 = *la;
  if (n_edges) *n_edges = 0;
  if (k_max) *k_max = 0;
  if (rounds_out) *rounds_out = 0;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  uint64_t alive = 0;
  LaunchCtx ctx;
  if (int rc = begin_launch(sym, &l2, &alive, ctx)) return rc;
  if (sym->ne == 0) return GM_OK;
  if (int rc = ensure_local_buffers(g, true, decompose)) return rc;
  double ms = 0.0;
  gm_graph *run_on = nullptr;
  if (int rc = local_supports(g, &l2, &ms, &run_on)) return rc;
  if (int rc = start_timer(ctx)) return rc;
  hipStream_t stream = ctx.stream;
  if (int rc = local_map(ctx, run_on, g->d_lent)) return rc;
  if (!g->lrev_ready) {  // (once per handle)
    HIP_TRY(launch_local_rev(g->nv, g->ne, g->d_rp, g->d_col, g->d_lrev, g->cu_count, stream));
    g->lrev_ready = true;
  }
  HIP_TRY(launch_local_peel_init(g->ne, g->d_lrev, g->d_lmark, g->cu_count, stream));
  LocalPeelParams pp;
  memset(&pp, 0, sizeof pp);
  pp.nv = g->nv; pp.ne = g->ne; pp.rp = g->d_rp; pp.col = g->d_col; pp.rev = g->d_lrev;
  pp.sup = g->d_lent; pp.mark = g->d_lmark; pp.front = g->d_lfront; pp.cnt = g->d_lcnt;
  pp.truss = decompose ? g->d_ltruss : nullptr;
  long long k = decompose ? 3 : k_in, kmax = 0;
  int rounds = 0;
  for (;;) {
    unsigned word[2] = {0u, 0u};
    for (;;) {  // the rounds of level k: threshold k - 2
      pp.thr = (unsigned)(k - 2);
      pp.level = (unsigned)(k - 1);
      HIP_TRY(hipMemsetAsync(g->d_lcnt, 0, 8, stream));
      HIP_TRY(launch_local_mark(pp, g->cu_count, stream));
      HIP_TRY(hipMemcpyAsync(word, g->d_lcnt, sizeof word, hipMemcpyDeviceToHost, stream));
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
  gm_stats s;
  memset(&s, 0, sizeof s);
  if (int rc = end_launch(ctx, FIN_COPY, 0, &alive, 1, &s)) return rc;
  if (n_edges) *n_edges = alive;
  if (k_max) *k_max = (int32_t)kmax;  // (the last level that removed an edge)
  if (rounds_out) *rounds_out = rounds;
  if (st) st->kernel_ms = ms + s.kernel_ms;
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

// ---- triangle listing (gm_list.hip; DESIGN.md "Triangle listing") -----------------------------------------------------------------------
// On the oriented copy as numbered: it keeps the caller's ids, so a match is written as it is found.  The count stage runs once per handle
// (the batches' first slots stay on the SYMMETRIC handle); a window is one fill launch that walks only the batches it meets.
extern "C" int gm_tc_list(const gm_graph *sym, const gm_launch *la, uint64_t first, uint64_t cap, int32_t *d_tri, uint64_t *total,
                          uint64_t *n_written, gm_stats *st) {
  if (total) *total = 0;
  if (n_written) *n_written = 0;
  if (int rc = local_refusals(sym, la)) return rc;
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2;
  memset(&l2, 0, sizeof l2);
  if (la) l2 = *la;
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
  if (!g->list_ready) {  // (once per handle)
    if (dag->ne > 0) {
      const size_t nb = (size_t)((dag->ne + GM_WAVE - 1) / GM_WAVE);
      {
        std::lock_guard<std::mutex> lk(g->mu);
        if (!g->d_list_off) HIP_TRY(g->d_list_off.alloc(sizeof(unsigned long long) * (nb + 1)));
      }
      lp.off = g->d_list_off;
      HIP_TRY(list_count_scan(lp, g->cu_count, ctx.stream));
      HIP_TRY(hipMemcpyAsync(&g->list_total, g->d_list_off + nb, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx.stream));
      HIP_TRY(hipStreamSynchronize(ctx.stream));
    }
    g->list_ready = true;
  }
  const uint64_t T = g->list_total;
  const uint64_t nw = (d_tri && first < T) ? std::min<uint64_t>(cap, T - first) : 0;
  if (nw > 0) {
    lp.off = g->d_list_off; lp.first = first; lp.nw = nw; lp.tri = d_tri;
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
    return run_pattern(PAT_DIAMOND, sym, la, 4, total, 1, st);
  }
  // rectangle / house / pentagon run on a copy of the graph renumbered by degree (get_relabeled; tune[6] & GM_T6_AS_NUMBERED: on the
  // graph as given). tune[6] & GM_T6_SGL_NESTED: the wave-per-edge loop nests; & GM_T6_SGL_FLAT: rectangle as wedges + flat intersections,
  // house without the LDS S-bitmap (A/B, tests).
  const bool is_rect = strcmp(pattern, "rectangle") == 0, is_house = strcmp(pattern, "house") == 0, is_pent = strcmp(pattern, "pentagon") == 0;
  if (is_rect || is_house || is_pent) {
    if (!sym) return GM_ERR_INVALID;
    if (int rc0 = reject_big(sym)) return rc0;
    const int t6 = la ? la->tune[6] : 0;
    gm_graph *self = const_cast<gm_graph *>(sym);
    const gm_graph *run_on = sym;
    const bool wedge_form = (is_pent || is_rect) && (t6 & GM_T6_SGL_FLAT);  // anchored wedges: hubs first; 2-path / (v0,v1,v3) forms: hubs last
    // house: by wedge accumulation (default; its 2-path count does not depend on the numbering, so no renumbered copy), or
    // the flattened (v0, v1, v3) form (GM_T6_SGL_FLAT; GM_T6_HOUSE_NO_BITMAP: without the LDS S-bitmap). The packed map holds 24-bit counts and
    // 40-bit weighted sums: rows of 2^20 entries or more take the flattened form.
    const bool house_acc = is_house && !(t6 & (GM_T6_SGL_NESTED | GM_T6_SGL_FLAT | GM_T6_HOUSE_NO_BITMAP)) && sym->max_deg < (1 << 20);
    if (!(t6 & GM_T6_AS_NUMBERED) && !(t6 & GM_T6_SGL_NESTED) && !house_acc) {
      gm_graph *r = nullptr;
      int rc = get_relabeled(self, wedge_form ? 1 : 0, &r);
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
    self->ring_alias = (run_on != sym) ? const_cast<gm_graph *>(run_on) : nullptr;
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
  if (std::lock_guard<std::mutex> lk(g->mu); !g->wrect_ready) {  // (two first calls on one handle: one builds, the other waits)
    OtherSetupScope scope(g);
    const size_t nv = (size_t)g->nv;
    int range = kWrectRange;
    if (const char *e = gm_opt("GM_WRECT_RANGE")) range = std::max(16, std::min(kWrectRange, std::atoi(e)));
    const long long nranges = std::max<long long>(1, ((long long)g->nv + range - 1) / range);
    g->wrect_range = range;
    g->wrect_grp = (int)((nranges + 63) / 64);
    HIP_TRY(g->d_wrect_mask.alloc(sizeof(unsigned long long) * std::max<size_t>(nv, 1)));
    HIP_TRY(launch_wrect_mask(g->nv, g->d_rp, g->d_col, range, g->wrect_grp, g->d_wrect_mask, g->cu_count, 0));
    std::vector<int> idx0h(std::max<size_t>(nv, 1));
    if (nv) HIP_TRY(hipMemcpy(idx0h.data(), g->d_idx0, sizeof(int) * nv, hipMemcpyDeviceToHost));
    const std::vector<int2> tasks = wrect_tasks(idx0h.data(), nv, range, kWrectThreads);  // (the hubs' per-range tasks first)
    g->n_wrect_tasks = tasks.size();
    HIP_TRY(g->d_wrect_tasks.alloc(sizeof(int2) * std::max<size_t>(tasks.size(), 1)));
    if (!tasks.empty()) HIP_TRY(hipMemcpy(g->d_wrect_tasks, tasks.data(), sizeof(int2) * tasks.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    g->wrect_ready = true;
  }
  WrectParams p;
  memset(&p, 0, sizeof p);
  p.rp = g->d_rp; p.col = g->d_col; p.idx0 = g->d_idx0;
  p.rmask = g->d_wrect_mask; p.range = g->wrect_range; p.grp = g->wrect_grp;
  p.tasks = g->d_wrect_tasks; p.count = g->n_wrect_tasks;
  p.queue = queue_word64(g, QW64_MAIN);
  p.counters = g->d_counters;
  if (int rc = start_timer(ctx)) return rc;
  const int grid = grid_for((long long)p.count, g->cu_count, wrect_per_cu());
  if (p.count > 0) HIP_TRY(launch_wrect(p, grid, ctx.stream));
  fill_stats(st, (uint64_t)g->ne, (uint64_t)p.count, grid, kWrectThreads);
  const int rc = end_launch(ctx, FIN_RAW4, 0, v, 4, st);
  out[0] = v[0];
  out[1] = v[1];
  self->ring_alias = (run_on != sym) ? run_on : nullptr;
  return rc;
}

extern "C" int gm_sgl6_raw(const gm_graph *sym, uint32_t need, const gm_launch *la, uint64_t raw[GM_SGL6_NRAW], gm_stats *st) {
  if (!sym || !raw || !need || (need >> GM_SGL6_NRAW)) return GM_ERR_INVALID;
  for (int i = 0; i < GM_SGL6_NRAW; ++i) raw[i] = 0;
  if (int rc0 = reject_big(sym)) return rc0;
  if (la && (la->world > 1 || la->d_counts)) return GM_ERR_UNSUPPORTED;  // (the closed forms are applied on the host: one rank, synchronous)
  gm_graph *g = const_cast<gm_graph *>(sym);
  gm_launch l2;
  memset(&l2, 0, sizeof l2);
  if (la) l2 = *la;
  auto want = [&](int i) { return (need >> i & 1u) != 0; };
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  HIP_TRY(hipSetDevice(g->device));
  {  // unsorted rows are refused as in every solver (begin_launch's check and text, before any of the sub-launches builds a table)
    bool sorted = false;
    if (int rc = graph_rows_sorted(g, &sorted)) return rc;
    if (!sorted) {
      g_last_error = "the neighbour lists of this graph are not strictly ascending: call gm_graph_sort_neighbors first (Graph::sort_neighbors, adj_sorted = 0)";
      return GM_ERR_INVALID;
    }
  }
  if (sym->ne == 0) return GM_OK;
  double ms = 0.0;
  gm_stats s;
  const bool entry_sums = want(R6_X) || want(R6_Y) || want(R6_M);
  if (entry_sums || want(R6_D) || want(R6_B) || want(R6_K4)) {
    // D, B and K4 are sums of the 5-vertex forms; X, M and Y read the arrays their pass leaves on the DAG it ran on -- the supports of the
    // entries, 2 T_v, the symmetric degrees -- so the pass runs for them too (T asks for nothing but the pass itself)
    unsigned n5 = (want(R6_D) ? 1u << R5_D : 0u) | (want(R6_B) ? 1u << R5_B : 0u) | (want(R6_K4) ? 1u << R5_K4 : 0u);
    if (entry_sums && !(n5 & ((1u << R5_D) | (1u << R5_B)))) n5 |= 1u << R5_T;
    uint64_t raw5[GM_SGL5_NRAW];
    memset(&s, 0, sizeof s);
    if (int rc = sgl5_raw_needs(sym, n5, &l2, raw5, &s)) return rc;
    ms += s.kernel_ms;
    raw[R6_D] = want(R6_D) ? raw5[R5_D] : 0;
    raw[R6_B] = want(R6_B) ? raw5[R5_B] : 0;
    raw[R6_K4] = want(R6_K4) ? raw5[R5_K4] : 0;
  }
  if (entry_sums) {
    gm_graph *run_on = nullptr;
    if (int rc = diamond_run_on(sym, &l2, &run_on)) return rc;  // (the handle the pass above ran on)
    if (!run_on->d_w5sup || !run_on->d_w5tv2 || !run_on->d_w5deg) return GM_ERR_INVALID;
    {
      std::lock_guard<std::mutex> lk(run_on->mu);
      if (!run_on->d_s6e1) HIP_TRY(run_on->d_s6e1.alloc(sizeof(unsigned) * (size_t)std::max(run_on->nv, 1)));
    }
    uint64_t v[4] = {0, 0, 0, 0};
    LaunchCtx ctx;
    if (int rc = begin_launch(run_on, &l2, v, ctx)) return rc;
    HIP_TRY(hipMemsetAsync(run_on->d_s6e1, 0, sizeof(unsigned) * (size_t)std::max(run_on->nv, 1), ctx.stream));
    if (int rc = start_timer(ctx)) return rc;
    Sgl6EntryParams ep;
    memset(&ep, 0, sizeof ep);
    ep.nv = run_on->nv; ep.ne = run_on->ne; ep.rp = run_on->d_rp; ep.col = run_on->d_col;
    ep.sup = run_on->d_w5sup; ep.deg = run_on->d_w5deg; ep.tv2 = run_on->d_w5tv2; ep.e1 = run_on->d_s6e1; ep.out = run_on->d_counters;
    HIP_TRY(launch_sgl6_sums(ep, run_on->cu_count, ctx.stream));
    memset(&s, 0, sizeof s);
    if (int rc = end_launch(ctx, FIN_RAW4, 0, v, 4, &s)) return rc;
    ms += s.kernel_ms;
    raw[R6_X] = want(R6_X) ? v[0] : 0;
    raw[R6_M] = want(R6_M) ? v[1] : 0;
    raw[R6_Y] = want(R6_Y) ? v[2] : 0;
  }
  if (want(R6_Z)) {  // (the kernel of Z counts R on the way: the rectangle path is only asked when Z is not)
    uint64_t zr[2] = {0, 0};
    memset(&s, 0, sizeof s);
    if (int rc = run_wrect(sym, &l2, zr, &s)) return rc;
    ms += s.kernel_ms;
    raw[R6_Z] = zr[0];
    raw[R6_R] = want(R6_R) ? zr[1] : 0;
  } else if (want(R6_R)) {
    memset(&s, 0, sizeof s);
    if (int rc = gm_sgl(sym, "rectangle", &l2, &raw[R6_R], &s)) return rc;
    ms += s.kernel_ms;
  }
  if (want(R6_C5)) {
    memset(&s, 0, sizeof s);
    if (int rc = gm_sgl(sym, "pentagon", &l2, &raw[R6_C5], &s)) return rc;
    ms += s.kernel_ms;
  }
  g->ring_alias = nullptr;
  g->ring_extra[0] = g->ring_extra[1] = nullptr;
  fill_stats(st, (uint64_t)sym->ne, 0, 0, kWavesPerBlock * GM_WAVE);
  if (st) st->kernel_ms = ms;
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
    gm_graph *self = const_cast<gm_graph *>(dag), *run_on = nullptr;
    int rc = topo_view(dag, la, &run_on);
    if (rc) return rc;
    rc = run_pattern(PAT_CLIQUE4, run_on, la, k, total, 1, st);
    self->ring_alias = (run_on != self) ? run_on : nullptr;
    return rc;
  }
  return run_pattern(k == 4 ? PAT_CLIQUE4 : PAT_CLIQUEK, dag, la, k, total, 1, st);
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
  gm_launch l2;
  memset(&l2, 0, sizeof l2);
  if (la) l2 = *la;
  uint64_t *d_out = l2.d_counts;
  if (const int rc_dag = ensure_dag_cache(g)) return rc_dag;  // (the oriented copy, cached on the handle)
  gm_stats s1, s2, s3;
  memset(&s1, 0, sizeof s1); memset(&s2, 0, sizeof s2); memset(&s3, 0, sizeof s3);
  l2.d_counts = d_out;
  int rc = run_pattern(PAT_MOTIF4E, sym, &l2, 4, raw, 4, &s1, FIN_RAW4, 0);
  if (rc) return rc;
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
    rc = (l2.tune[6] & GM_T6_SGL_FLAT) ? run_rect_flat(rect_on, &l2, raw ? &raw[4] : nullptr, &s2)
                             : run_rect_acc(rect_on, &l2, raw ? &raw[4] : nullptr, &s2);
    rect_handle = rect_on;
  }
  if (rc) return rc;
  l2.d_counts = d_out ? d_out + 5 : nullptr;
  rc = gm_clique(g->dag_cache, 4, &l2, raw ? &raw[5] : nullptr, &s3);  // (on the DAG's topological view)
  if (rc) return rc;
  if (st) {
    *st = s1;
    st->kernel_ms = s1.kernel_ms + s2.kernel_ms + s3.kernel_ms;
  }
  g->ring_alias = nullptr;
  g->ring_extra[0] = (rect_handle != sym) ? rect_handle : nullptr;  // (tune[6] & GM_T6_AS_NUMBERED: the rectangle kernel ran on this handle itself)
  g->ring_extra[1] = g->dag_cache;
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
  const int rc = run_pattern(PAT_MOTIF3, run_on, la, 3, counts, ncounts, st);
  if (run_on != sym) const_cast<gm_graph *>(sym)->ring_alias = run_on;
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
  if (!g->sum_c2_valid) {  // sum_v C(d(v),2): one reduction kernel over the offsets
    DevBuf<unsigned long long> acc;
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(acc.alloc(1));
    HIP_TRY(hipMemset(acc.p, 0, 8));
    const dim3 cgrid((unsigned)std::min<long long>(((long long)g->nv + 255) / 256, 2048));
    if (g->d_rp64) hipLaunchKernelGGL((sum_c2_kernel<long long>), cgrid, dim3(256), 0, 0, g->nv, (const long long *)g->d_rp64, acc.p);
    else hipLaunchKernelGGL((sum_c2_kernel<int>), cgrid, dim3(256), 0, 0, g->nv, (const int *)g->d_rp, acc.p);
    unsigned long long s2 = 0;
    HIP_TRY(hipMemcpy(&s2, acc.p, 8, hipMemcpyDeviceToHost));
    g->sum_c2 = s2;
    g->sum_c2_valid = true;
  }
  const int rank = la ? la->rank : 0;
  const int rc = run_tc(g->dag_cache, la, counts, ncounts, st, FIN_MOTIF3_FORMULA, rank == 0 ? g->sum_c2 : 0ull);
  g->ring_alias = g->dag_cache;
  return rc;
}

// Tooling: the level-2 part of SURVEY.md 8(d)'s ALGORITHMIC bytes of one 4-clique launch,
//   sum_e [ 8|S1| + sum_{v2 in S1} (4(|S1| + d+(v2)) + 16) ]  =  24*sum|S1| + 4*sum|S1|^2 + 4*sum_{matches} d+(v2),
// from three sums the mining kernel itself produces (PAT_DAGSTATS). The level-1 part 4*sum_e(d+(v0)+d+(v1)) + 40|E+|
// is the TC formula (computed by the caller from the CSR arrays).
extern "C" int gm_clique4_level2_bytes(const gm_graph *dag, uint64_t *bytes) {
  if (!dag || !bytes) return GM_ERR_INVALID;
  uint64_t raw[4] = {0, 0, 0, 0};  // raw[0] = sum n^2, raw[1] = sum_{matches} d+(v2), raw[2] = sum n
  const int rc = run_pattern(PAT_DAGSTATS, dag, nullptr, 4, raw, 4, nullptr, FIN_RAW4, 0);
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
    info[3] = g->n_cg_blocks;
    break;
  }
  return GM_OK;
}

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_launch_kernel() {}
void gm_touch_launch() { hipLaunchKernelGGL(gm_touch_launch_kernel, dim3(1), dim3(1), 0, 0); }
