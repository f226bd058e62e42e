// gm_host.h -- host-side internals shared by the translation units behind the C ABI (include/graphminer_amd.h):
//   gm_graph.hip   handle, upload / adopt, orientation, neighbour sort, degree renumbering      (GraphGPU::init, Graph::orientation)
//   gm_tables.hip  task-chunk tables, their bitmap sets and rank shares, partitions              (Graph::init_edgelist, Scheduler)
//   gm_tasks.hip   edge descriptors, task lists, key stream, block-pair rule, support masks / corner of the triangle-count family
//   gm_clique_plan.hip  the 4-clique plan: wide vertices, core bitmap and its blocks, rounds, gather index
//   gm_launch.hip  the launch layer (interface: gm_launch.h, for the three solver units only): launch prologue / epilogue, run_pattern,
//                  gm_kernel_times, gm_tc / gm_clique / gm_motif, and every kernel of the layer
//   gm_solve_sgl.hip    the SgL family: gm_sgl, the rectangle / house / pentagon map solvers, gm_diamond_support_*, gm_sgl4 / 5 / 6   (host code only)
//   gm_solve_local.hip  gm_tc_local, gm_ktruss, gm_truss_decompose, gm_tc_list, gm_clique_local, gm_clique_list, gm_rect_local, gm_clique_kcore, gm_clique_core_decompose, gm_clique_ktruss, gm_clique_truss_decompose, gm_tri_clique4_local, gm_nucleus34, gm_nucleus34_decompose   (host code only)
//   gm_tools.hip   set-op batch, R-MAT generator, PMC / issue-rate calibration kernels, self test
// Host-side counterparts in the reference:
//   GraphGPU::init / init_edgelist          include/graph_gpu.h:69-194
//   launch sizing                            src/triangle/gpu_base.cu:36-45, src/clique/gpu_base.cu:28-50
//   Scheduler::round_robin                   src/common/scheduler.cc:34-85
//   Graph::orientation                       src/common/graph.cc:233-279
// None of that code is reused: tasks are described by a compact chunk table (16 B per ~256 edges)
// instead of per-GPU COO copies, and the multi-GPU split is index arithmetic on chunk ids.
// State of a handle (struct gm_graph, below): the graph itself; the structures built on first use, one struct each behind a Once<T>
// (gm_once.h: built under g->mu in a local, published whole, read through the Once -- one protocol for "is it there yet"); the keyed
// lists handed out under g->mu (tables, bitmap sets, clique plans); and the work buffers of the call families, which need no protocol
// because one solver call at a time runs per handle (include/graphminer_amd.h).
#pragma once
#include "../../include/graphminer_amd.h"
#include "gm_centre_plan.h"
#include "gm_devown.h"
#include "gm_mine.h"
#include "gm_once.h"
#include "gm_setops.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace gm;  // (internal header: every unit that includes it lives behind the C ABI)

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
extern thread_local std::string g_last_error;
extern thread_local int g_last_hip_error;  // the hipError_t of the most recent hip_fail of this thread (out of memory: optional structures are skipped)
int hip_fail(hipError_t e, const char *what, const char *file, int line);
#define HIP_TRY(call)                                              \
  do {                                                             \
    hipError_t _e = (call);                                        \
    if (_e != hipSuccess) return hip_fail(_e, #call, __FILE__, __LINE__); \
  } while (0)
// A step that may fail without the call failing (an optimisation that did not fit): taken before the step, drop() forgets its failure --
// the runtime's sticky error, and the text and code hip_fail recorded go back to what they were
struct HipFailureMark {
  std::string text = g_last_error;
  int code = g_last_hip_error;
  void drop() const { (void)hipGetLastError(); g_last_error = text; g_last_hip_error = code; }
};

// The temporaries of the setup paths (a table build has ~20 of them) come out of ONE device allocation per handle: a bump allocator
// that a PoolScope opens at the top of a setup function and rewinds at its end. hipMalloc / hipFree cost 0.1-0.3 ms each and hipFree
// synchronises the device: round 2 measured ~10 ms of allocation overhead per table. What does not fit the pool
// falls through to hipMalloc (and tells the pool how much to ask for next time).
struct TempPool {
  DevOwn<char> base;
  size_t cap = 0, off = 0, want = 0;  // want: bytes the open scopes would have liked (pool + fall-through allocations)
  // A handle family (a graph + its cached orientation and renumbered copies) shares the root's pool, and two threads may work on two
  // members at once under their own handle locks.  The pool belongs to ONE thread at a time: the first PoolScope claims it,
  // nested scopes of that thread share it (stack discipline), and a scope opened by another thread meanwhile gets no pool -- its
  // DevBufs fall through to hipMalloc.  No lock is held across a scope, so there is no lock order to get wrong.
  std::mutex claim_mu;
  std::thread::id owner;
  int depth = 0;
};
extern thread_local TempPool *g_temp_pool;  // the pool of the innermost open PoolScope of this thread (gm_graph.hip)

// Temporaries that do not fit the pool (the GB-sized scratch copies of orientation / renumbering / the key stream on a large graph) are
// kept in a small per-device CACHE (a budget of 16 GB and 64 blocks PER DEVICE) instead of going back to the driver: hipFree of a large buffer costs 0.2 ms on a good day and 30 ms
// per GB on a bad one (scripts/alloc_jitter.hip: p90 of hipFree(1 GB) = 30 ms, in phases), and that -- not a kernel -- was the 441 ms
// first call of config 5 the round-4 driver run recorded against the builder's 80 (reproduced in round 5: orientation 88 instead of 7.5
// ms, tables 227 instead of 28, every kernel time unchanged).  A block is handed out again to a request of at least a quarter of its size,
// after a device synchronisation; the cache is emptied when a root handle is freed (gm_graph.hip).
hipError_t big_cache_get(void **p, size_t bytes, size_t *block_bytes);  // a cached block or a fresh hipMalloc
void big_cache_put(void *p, size_t block_bytes);                         // synchronises the device; beyond the cache's budget: hipFree
void big_cache_trim();                                                   // hipFree of every cached block of the current device
constexpr size_t kBigCacheMinBytes = (size_t)4 << 20;
// EVERY device allocation of the library goes through here: hipMalloc, and when the device is out of memory the cached
// temporaries of this device go back to the driver and the request is made once more -- the cache may park up to its budget of memory
// that nothing else can reach, and a setup path must not fail (or quietly drop an optimisation) while it does.
// dev_malloc_bytes, and dev_free, the counterpart: a block of >= kBigCacheMinBytes goes to the device's cache, anything else to hipFree
// (declared in gm_devown.h, with DevOwn<T>, the owner of every persistent array)
void dev_handle_born(int device);  // (gm_graph.hip: the cache lives as long as the device has a handle)
bool dev_handle_died(int device);

template <class T>
struct DevBuf {  // RAII device array; pooled when a PoolScope is open and the pool has room
  T *p = nullptr;
  size_t n = 0;
  bool pooled = false;
  size_t block_bytes = 0;  // > 0: a block of the large-temporary cache (returned there by drop())
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { drop(); }
  void drop() {
    if (p && !pooled) {
      if (block_bytes) big_cache_put(p, block_bytes);
      else dev_free(p);
    }
    p = nullptr;
    pooled = false;
    block_bytes = 0;
  }
  // keep = true: the array outlives the scope (DevOwn::take hands it to a long-lived owner): never from the pool
  hipError_t alloc(size_t count, bool keep = false) {
    drop();
    n = count;
    const size_t bytes = (sizeof(T) * std::max<size_t>(count, 1) + 255) & ~(size_t)255;
    TempPool *pool = keep ? nullptr : g_temp_pool;
    if (pool) {
      pool->want += bytes;
      if (pool->off + bytes <= pool->cap) {
        p = reinterpret_cast<T *>(pool->base + pool->off);
        pool->off += bytes;
        pooled = true;
        return hipSuccess;
      }
    }
    if (!keep && bytes >= kBigCacheMinBytes) return big_cache_get(reinterpret_cast<void **>(&p), bytes, &block_bytes);
    return dev_malloc_bytes(reinterpret_cast<void **>(&p), bytes);
  }
  // (a pooled array cannot be handed on: alloc(..., true); a cached block can -- it is an allocation of its own, only larger than asked for)
  T *release() { T *q = pooled ? nullptr : p; p = nullptr; n = 0; pooled = false; block_bytes = 0; return q; }
};

struct ScanTemp {  // temp storage of the hipCUB calls, grown on demand
  DevBuf<char> buf;
  hipError_t reserve(size_t bytes) { return bytes <= buf.n ? hipSuccess : buf.alloc(bytes); }
};


// (dev_exclusive_sum and the other hipCUB helpers over a ScanTemp: gm_scan.h -- only the units that include hipCUB pay for them)

// estimated work (adjacency entries touched) above which a chunk is cut into parts
// Rows longer than kBitmapMinDeg get a dense vertex-id bitmap, longest first, within kBitmapBudget bytes: SPLIT chunks
// probe their own row's, pass Y probes the searched row's (one load instead of ~lg d dependent ones). A probe is a random
// 64 B line, so it only beats a bisection whose upper levels sit in cache when the row is long. Measured (diamond ms on
// R-MAT-20 / -22 / -24, 3-motif on R-MAT-24): min degree 1024: - / 117 / - / 1037;  2048: 25.8 / 94.8 / - / 1068;
// 4096: 30.6 / 94.5 / 1539 / 1057;  8192: 30.8 / 89.6 / 1528 / 1073;  16384: 44.7 / 89.8 / 1528 / 1072;
// 2048 within 256 MB (Infinity-Cache sized): 25.7 / 87.1 / 2275 / 1373;  no pass-Y bitmaps at all: - / 124 / - / 1473.
#ifndef GM_BITMAP_MIN_DEG
#define GM_BITMAP_MIN_DEG 2048
#endif
#ifndef GM_BITMAP_BUDGET_MB
#define GM_BITMAP_BUDGET_MB 8192
#endif
constexpr int kBitmapMinDeg = GM_BITMAP_MIN_DEG;
constexpr unsigned long long kBitmapBudget = (unsigned long long)GM_BITMAP_BUDGET_MB << 20;
constexpr unsigned long long kPartCostCap = 8ull << 20;     // DAG patterns: staged chunks stay whole
#ifndef GM_PART_CAP_SYM
#define GM_PART_CAP_SYM (2ull << 20)
#endif
constexpr unsigned long long kPartCostCapSym = GM_PART_CAP_SYM;  // symmetric-graph patterns (measured on R-MAT-20/22/24: 1 M best for diamond, 2 M for 3-motif)
constexpr int kDefaultChunk = 1024;  // task edges per chunk when the caller does not say

// Which rows a chunk table covers. The k-clique table leaves the wide vertices to the two-phase path; the tables of the
// symmetric-graph patterns come in three: the general one skips the rows of the big-LDS classes, each class table keeps only
// its own window of row lengths.
struct RowFilter {
  int skip_clique_wide = 0;                    // > 0: leave out the vertices with clique_is_wide(d, this many matrix words)
  int skip_lo = 0, skip_hi = 0;                // rows with skip_lo < d <= skip_hi are left out (0, 0 = none)
  int only_lo = -1, only_hi = 0x7fffffff;      // rows with only_lo < d <= only_hi are kept
  int tct = 0;                                 // 1: chunk costs from the task lists of gm_tch.hip (the tasks a chunk hosts, not its own entries)
  __host__ __device__ bool skips(int d) const {
    return (skip_clique_wide > 0 && clique_is_wide(d, skip_clique_wide)) || (d > skip_lo && d <= skip_hi) || !(d > only_lo && d <= only_hi);
  }
  bool operator==(const RowFilter &o) const {
    return skip_clique_wide == o.skip_clique_wide && skip_lo == o.skip_lo && skip_hi == o.skip_hi && only_lo == o.only_lo && only_hi == o.only_hi && tct == o.tct;
  }
};

// A rank's SHARE of a chunk table (world > 1): the records it dequeues, in dequeue order.  All PARTS of a chunk go to the same rank:
// a part is "every nparts-th batch of the chunk's task list", and the order of a host's tasks is the order in which the placement's
// atomics arrived -- different in every process.  Two ranks that split the parts of one chunk would each cut THEIR OWN order of its
// tasks, and the union would not be the chunk (round 5: bench.py --gpus 2 at full size counted 750,563,783 triangles for 750,506,260;
// the in-process rank-share tests of rounds 2 - 4 shared one handle and could not see it).
struct ShareOrder {
  int world = 1, rank = 0, policy = 0, which = -1;  // which: the dequeue order it was cut from (-1: plain record order)
  DevOwn<int> d;
  long long n = 0;
  unsigned long long edges = 0;  // task edges of the share
};

struct ChunkTable {
  int target;       // T: CSR entries per chunk
  bool allow_split; // rows longer than the staging capacity may be cut across chunks
  int bit_words;    // clique: LDS bit-matrix budget the chunks were built for (0 = unconstrained)
  unsigned long long part_cap = 0;  // estimated work above which a chunk is cut into parts; 0 = chunks are never cut (nparts == 1 everywhere)
  int stage_cap = 0;                // rows longer than this are SPLIT rows
  RowFilter rf;                     // the rows the table covers
  int bitmap_min_deg = 0;           // rows longer than this got dense bitmaps (allow_split tables)
  std::vector<unsigned long long> cost;  // estimated work per chunk (after cutting)
  DevOwn<ChunkRec> d;
  size_t n = 0;
  DevOwn<int> d_slot;                    // per chunk: hub bitmap slot or -1
  // dequeue orders of the round-robin policy: [0] chunks well above the mean cost first (heaviest first), the rest in vertex
  // order (single rank); [1] all chunks by estimated cost, descending (rank r of n owns every n-th entry)
  DevOwn<int> d_order[2];
  std::vector<int> order[2];
  // borrowed: the arrays of a BitmapSet of the graph (shared by its tables)
  unsigned *d_bitmaps = nullptr;         // n_bitmaps x bitmap_words
  int *d_row_slot = nullptr;             // per vertex: bitmap slot or -1
  size_t n_bitmaps = 0;
  unsigned long long bitmap_words = 0;
  unsigned long long max_bit_words = 0;  // largest nel*stride over chunks that exceed bit_words
  // Host views of the per-chunk scalars: what a SHARE of the table needs (a rank of a larger job: its task edges, the vertex-range policy;
  // the k-clique plan; the chunk dumps).  A device-built table keeps them on the device and table_host_views() fetches them on first use --
  // one rank never does: the first pageable device-to-host copy of a process costs ~10 ms in the runtime, which was the largest single
  // item of a first triangle count (GM_SETUP_TRACE).  total_edges / total_cost are fetched with the table (16 bytes).
  std::vector<unsigned long long> edge_prefix;  // edges owned by chunks [0,i)
  std::vector<int> first_vertex;                // u_begin of every chunk (ascending; SPLIT chunks repeat it)
  bool host_ready = false;
  unsigned long long total_edges = 0, total_cost = 0;
  size_t n_with_cost = 0;  // chunks of non-zero cost (device-built tables): they are the first n_with_cost entries of d_order[1]
  DevOwn<int> d_edges, d_firstv;  // device twins of the host views (device-built tables)
  DevOwn<unsigned long long> d_cost;
  std::list<ShareOrder> shares;  // the shares handed out so far (get_share_order)
};
int table_host_views(gm_graph *g, ChunkTable *t);  // gm_tables.hip
// GM_PART_VERTEX: the contiguous run of chunks whose first vertex lies in the vertex range of rank / world (after table_host_views)
static inline void chunk_range_of_vertex_share(const ChunkTable *tb, int nv, int rank, int world, long long *first, long long *count) {
  auto first_chunk_at = [&](long long v) {
    long long lo = 0, hi = (long long)tb->n;
    while (lo < hi) {
      const long long mid = (lo + hi) / 2;
      if (tb->first_vertex[(size_t)mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  *first = first_chunk_at((long long)nv * rank / world);
  *count = first_chunk_at((long long)nv * (rank + 1) / world) - *first;
}
// the share of rank / world under `policy` (round robin: every world-th CHUNK of the order; range: a contiguous run of chunks), cut from
// dequeue order `which` (0 / 1, or -1 = record order); needs the device twins of the per-record scalars (a device-built table)
int get_share_order(gm_graph *g, ChunkTable *t, int world, int rank, int policy, int which, const ShareOrder **out);

// k-clique (k = 4): the plan of one rank's share (gm_mine.h "level 1 re-hosted"; built by get_clique_plan, gm_clique_plan.hip).
// OWNERS are the vertices whose matrices this rank builds and counts: the vertices of its share of the narrow chunk table + its share
// of the wide list. The matrix arena is bounded (GM_WIDE_ARENA_MB): a share whose matrices need more is processed in ROUNDS; a round
// has its own owners, offsets, task lists (every DAG edge of an owner, at the endpoint that hosts it) and host-chunk table.
struct CliqueRound {
  long long n_pos0 = 0, n_count = 0;       // narrow chunks: positions [n_pos0, n_pos0 + n_count) of the rank's share of the narrow table
  size_t w0 = 0, w1 = 0;                    // wide slots [w0, w1) of the plan's vertex list
  size_t mcls_begin[4] = {0, 0, 0, 0};      // ... per class of the matrix-core count kernel (gm_cmma.hip), in d_mcls_slots
  unsigned long long words = 0;             // arena words of the round
  DevOwn<unsigned long long> d_base;        // per vertex: word offset of its matrix (nv + 1; non-owners are empty)
  DevOwn<gm::CBuildTask> d_tasks;
  size_t n_tasks = 0;
  DevOwn<int> d_trp;                        // task-list offsets per host vertex (nv + 1)
  ChunkTable host_tab;                      // chunks of host vertices (rows that fit the stage), costs from the task lists
  // the blocked gather of the wide rows (gm_cgather.hip cgatherb_kernel): the (vertex, block of core rows) units of this round's wide
  // slots sorted by block, cut into work items of about equal probe counts
  DevOwn<uint4> d_gunits;
  DevOwn<unsigned> d_gtab;                 // the column tables of the round's slots (16-bit positions, two tiles per dword)
  DevOwn<int2> d_gitems;
  size_t n_gunits = 0, n_gitems = 0;
  unsigned long long gather_table_bytes = 0;  // records + row positions + table dwords the units read by construction (tooling: gm_clique4_gather_info)
};
struct CliquePlan {
  int rank = 0, world = 1, policy = 0, target = 0, order_which = 1;
  int stage = 1024;                  // LDS stage of the build kernel: 1024, or kCbMaxDeg when a longer row hosts
  bool topo = false;                 // every DAG edge goes from a smaller to a larger id: matrices strictly upper triangular
  ChunkTable *tabN = nullptr;        // narrow chunk table (a table of the graph)
  long long n_first = 0, n_step = 1, n_count = 0;  // this rank's share of it: positions first + i * step of the dequeue order
  const int *d_order = nullptr;
  std::vector<int> verts;            // this rank's wide vertices; slot = index here (longest rows first)
  DevOwn<int> d_verts;
  DevOwn<unsigned long long> d_slot_base;  // slot -> word offset of its matrix inside its round's arena
  DevOwn<int> d_mcls_slots;
  DevOwn<int4> d_mcls_rec;           // per entry of d_mcls_slots: {d+, word offset of the matrix (low, high), 0} (gm_cmma.hip)
  int core_base = -1;                // >= 0: the rows of the wide vertices' matrices whose first endpoint is >= core_base are gathered from the
                                     // core bitmap of the graph (gm_cgather.hip); the task lists of the streamed build leave them out
  std::vector<CliqueRound> rounds;
  unsigned long long wide_edges = 0;  // task edges of the wide vertices
};

// Dense vertex-id bitmaps of the hub rows: a property of the graph (which rows: longer than min_deg and not left to a
// big-LDS class), shared by every chunk table that needs them -- tables differ per world size / tuning, the bitmaps do not
// (round 1 rebuilt up to 8 GB of them per table: ADVICE r1).
struct BitmapSet {
  int min_deg = 0;
  RowFilter rf;
  DevOwn<unsigned> d_bitmaps;
  DevOwn<int> d_row_slot;
  size_t n = 0;
  unsigned long long words = 0;
};

// The plan of a map solver whose heavy centres count in LDS maps (rectangle, house; ensure_rect_plan / ensure_house_plan, gm_solve_sgl.hip)
struct CentrePlan {             // once per graph, published whole
  DevOwn<int> d_bnd;            // nv x (n + 1) row bounds
  DevOwn<int2> d_lds_tasks;     // (centre, range) tasks of the *_lds_kernel
  DevOwn<int4> d_acc_tasks;     // the "cut" list: first n_cut tasks walk only ends below cut
  unsigned long long n_lds_tasks = 0, n_acc_tasks = 0, n_cut = 0;
  int cut = 0, bnd_stride = 0;
  // what the lists hold, for gm_map_plan_info: {v, k} / {v, -1} LDS tasks; whole-workgroup acc tasks in the front / in the whole list
  unsigned long long n_lds_range = 0, n_lds_whole = 0, n_front_heavy = 0, n_acc_heavy = 0;
};

// ------------------------------------------------------------------------------------------------
// The structures a handle builds on first use and keeps: one struct each, held by gm_graph as a Once<...> (gm_once.h).  The builder fills a
// local value under g->mu and the whole value is published at once; readers go through the Once and never see a half-built group.  Every
// comment says who builds the group and who reads it.
// ------------------------------------------------------------------------------------------------
// Task lists of the shorter-list-streams triangle count.  Built by ensure_tasklists (gm_tasks.hip); read by plan_pattern / fill_mine_params
// (gm_launch.hip), ensure_sup_corner / ensure_sup_masks, gm_sup_corner_info.
struct TaskLists {
  DevOwn<int> trp;      // row offsets (nv + 1)
  DevOwn<int2> tdesc;   // per task {rp[partner], d(partner)}
  DevOwn<int> tedge;    // the task's own DAG entry (the edge supports), always built with the lists
  // TASK-MAJOR COPIES of the short lists (a handle that cannot have the key stream; build_inline_copies): colk = col followed by the keys
  // of every list of <= GM_TC_INLINE_MAX entries in task order, tdesck = the descriptors pointing at the copies.  Consecutive tasks of a
  // host then stream consecutive lines instead of one random 64-byte line (or two) each: what bounds the triangle count on
  // LiveJournal-shaped graphs (mean list 9).  Empty when they did not fit: the kernels then stream the rows themselves
  DevOwn<int> colk;
  DevOwn<int2> tdesck;
  unsigned long long n_copy_keys = 0;  // keys of the copies
  // the hub corner the lists leave out (gm_ctc.hip): no task of a row >= skip_from; core_h = nv - skip_from vertices (0 / 0x7fffffff: none)
  int core_h = 0;
  int skip_from = 0x7fffffff;
};
// The symmetric bit matrix of the corner the task lists leave out (core_h / 32 words per row), and first[row][word] = position of the
// word's first entry inside its row.  Built by ensure_sup_corner (gm_tasks.hip); read by launch_pattern (core_tc_block_kernel<true>).
struct SupCorner {
  DevOwn<unsigned> csym;
  DevOwn<unsigned short> cfirst;
};
// MATCH MASKS of the in-edge tasks with long tails: per DAG entry / per task the offset of the task's mask in the arena (64-bit words;
// kNoMask: the task keeps its atomics), the arena itself (written and read by every launch).  Built by ensure_sup_masks (gm_tasks.hip);
// not applicable: DAG not topological, arena beyond 2^32 words, no room, GM_SUP_NO_MASKS.  Read by plan_pattern / fill_mine_params /
// launch_pattern and gm_sup_mask_info.
struct SupMasks {
  DevOwn<unsigned> emoff, tmoff;
  DevOwn<unsigned long long> smask;
  unsigned long long words = 0;
  DevOwn<int> far_rows;  // the rows with tails of more than 64 keys (masks of several words), widest ids first
  int n_far_rows = 0;
  int min_tail = 0;      // the shortest tail with a mask the offsets were laid out for (0: kSupMaskMinTail; sup_mask_min_tail)
};
// nv <= 2^24: instead of descriptors that point at copies, the copies ARE the task list of the short lists -- a key stream in host order,
// every key tagged with its host's low 8 bits (GraphView::kst), offsets per host vertex, and the longer lists as their own task lists
// (trpl / tdescl).  No descriptor, no row search, no flattening for the short lists: one coalesced load per 64 keys.
// Built by ensure_keystream (gm_tasks.hip), first set; not applicable: ids beyond 24 bits, keys beyond the 32-bit index, GM_TC_NO_KEY_STREAM.
// Read by plan_pattern / fill_mine_params / launch_pattern, gm_tc_core_info / gm_tc_pairs_info.
struct KeyStream {
  DevOwn<unsigned> kst;  // the stream itself
  DevOwn<int> rp;
  DevOwn<int> trpl;
  DevOwn<int2> tdescl;
  unsigned long long n_keys = 0;  // keys of the stream
  int n_long_tasks = 0;
  int lmax = 0;                   // the limit of a "short" list the stream was built with
  // built for the edge supports (the first caller was ensure_keystream(g, true)): per key {entry it was copied from, entry of its task's
  // own edge}, per longer list the entry of its task's own edge.  Empty otherwise: KeyEntries below
  DevOwn<int2> kst_et;
  DevOwn<int> tedgel;
  // triangle count: the out-edges of the last core_h vertices are counted on the matrix cores from the corner of the hub core (gm_ctc.hip)
  // and the stream / the longer lists hold no task of a row >= skip_from; 0 / 0x7fffffff: no such corner.  With a choice of block pairs
  // (pair_region > 0) the three keep NAMING the base corner of the density rule (gm_tc_core_info) but the stream leaves out the chosen
  // pairs' edges instead, rows >= skip_from host tasks again: read skip_from < nv only as "this stream lacks edges that the product
  // takes", never as a row bound
  int core_h = 0;
  int skip_from = 0x7fffffff;
  long long core_edges = 0;  // entries of the rows >= skip_from
  // ... chosen per PAIR of 256-row blocks (IB <= JB) of a region at the end of the core bitmap instead of as a full triangle of rows
  // (tc_pairs_setup, inside the stream's build): the stream then leaves out exactly the edges u -> v, u >= pair_from, whose bit
  // IB * nb + JB of pair_bits is set, and the product walks pair_tasks (CoreTcParams::tasks).  pair_region = 0: no selection
  int pair_region = 0, pair_from = 0x7fffffff;
  DevOwn<unsigned> pair_bits;
  DevOwn<unsigned> pair_tasks;
  int n_pair_tasks = 0;
  long long pair_info[6] = {0, 0, 0, 0, 0, 0};  // gm_tc_pairs_info
};
// The entries of a key stream that was built WITHOUT them, for the edge supports: a second set kst2 / tdescl2 (same offsets, its own order
// of arrival) with its kst_et / tedgel.  Built by ensure_keystream(g, true) (gm_tasks.hip) after the first set; fill_mine_params reads
// the second set where it exists, else the first set's own entries.
struct KeyEntries {
  DevOwn<int2> kst_et;
  DevOwn<int> tedgel;
  DevOwn<unsigned> kst2;
  DevOwn<int2> tdescl2;
};
// The rows beyond the stage of the task-list kernels (> kTctStageMax entries): ids and the prefix of their lengths.  Built by
// ensure_long_rows (gm_tasks.hip); read by launch_pattern.
struct LongRows {
  DevOwn<int> rows;
  DevOwn<long long> prefix;
  int n = 0;
  long long edges = 0;
};
// A topologically numbered DAG: dense adjacency bitmap of its LAST h vertices (the hubs, when the numbering is by degree) -- row v - base
// holds bit w - base for every edge v -> w.  The rows of the wide vertices' 4-clique matrices whose first endpoint lies in this core are
// GATHERED from it (gm_cgather.hip), the triangle count takes its corner (gm_ctc.hip).  Built by ensure_core_bitmap (gm_clique_plan.hip); not
// applicable: not topological, too small, no room, GM_CORE_H = 0.  Read by tc_core_size / tc_pairs_setup / ensure_core_tri /
// get_clique_plan, launch_clique_wide / launch_pattern, gm_tc_core_info.
struct HubCore {
  DevOwn<unsigned> bits;
  int h = 0, base = 0;
};
// ... and the same bits cut into BLOCKS of consecutive rows for the blocked gather (gm_cgather.hip cgatherb_kernel).  Built by
// ensure_core_tri (gm_clique_plan.hip); not applicable: no core bitmap, no room.  Read by build_gather_index, launch_clique_wide,
// gm_clique4_gather_info.
struct CoreBlocks {
  DevOwn<unsigned> tri;     // block images: of every core row the words from its diagonal word on
  DevOwn<int> rowbase;      // per core row: offset inside its block's image - first stored word
  DevOwn<int> bid;          // per core row: its block
  DevOwn<int4> blk;         // per block: {first row, rows, image offset, image words}
  int n = 0;
};
// k-clique: the wide DAG vertices (clique_is_wide), longest rows first.  Built and read by get_clique_plan (gm_clique_plan.hip).
struct WideVerts {
  DevOwn<int> sorted;
  size_t n = 0;
};
// What is true of the graph itself, each found on first use (the slow path takes g->mu: no caller may hold it).
struct GraphFacts {
  Once<bool> rows_sorted;    // every row strictly ascending (graph_rows_sorted): the solvers refuse a handle that is not
  Once<bool> topological;    // every edge goes to a larger id, rows sorted (graph_is_topological)
  Once<unsigned long long> giant_edges;  // sum of the rows beyond kStageCapBig entries (giant_task_edges, gm_launch.hip)
  Once<double> tri_per_edge;  // triangles per entry of this DAG, estimated from a sample (ensure_tri_per_edge: the edge supports' stream switch)
  Once<double> mean_sq_deg;   // sum_v d(v)^2 / ne: the mean length of the row an entry sits in (ensure_mean_sq_deg: topo_view)
  Once<unsigned long long> sum_c2;  // sum_v C(d(v),2) (gm_motif_formula)
  Once<std::vector<int>> h_rp;  // host copy of the offsets (host_rp): download, k-clique tables, SgL renumbering, chunk dumps
};
// SgL (gm_solve_sgl.hip): what the map solvers index the graph by.  Each is built by the first call that needs it and read by the
// launches of that solver.
struct RectIdx {  // ensure_idx0: #neighbours below v
  DevOwn<int> idx0;
};
struct WedgeBlocks {  // rectangle per wedge block (sgl_rect_wedges): the wedge-block prefix
  DevOwn<unsigned long long> prefix;
  unsigned long long n = 0;
};
struct CentreTaskList {  // rectangle / house by wedge accumulation without LDS maps (build_centre_tasks): the task list
  DevOwn<int4> tasks;
  unsigned long long n = 0;
};
struct HouseTables {  // ensure_edge_tables: the per-entry tables of the house
  DevOwn<unsigned> t, tlt;
};
struct HouseBlocks {  // house per entry block: per-entry task-block prefix
  DevOwn<unsigned long long> prefix;
  unsigned long long n = 0;
};
// rectangle / house with the heavy centres' maps in LDS (round 6, gm_mine.hip rect_lds_kernel / house_lds_kernel): the id ranges and the
// plan (ensure_rect_plan / ensure_house_plan)
struct RectLdsPlan {
  gm::RectLdsRanges ranges;
  CentrePlan plan;
};
struct HouseLdsPlan {
  gm::HouseLdsRanges ranges;
  CentrePlan plan;
};
// the weighted 4-cycle kernel of the 6-vertex closed forms (gm_wrect.hip, gm_sgl6_raw), on the graph it walks (the copy numbered ascending
// in degree, or the handle itself): ids per range (GM_WRECT_RANGE), ranges per bit of the row masks, the masks, the task list
struct WrectPlan {
  DevOwn<unsigned long long> mask;
  DevOwn<int2> tasks;
  unsigned long long n_tasks = 0;
  int range = 0, grp = 1;
};
// the local 4-cycle counts (gm_rect_local.hip, gm_rect_local), on the graph the walk runs on (the copy numbered ascending in degree, or the
// handle itself): ids per range (GM_RECT_LOCAL_RANGE), ranges per bit of the row masks, the masks, the task list -- wrect_kernel's plan at
// a range of its own
struct RectLocalPlan {
  DevOwn<unsigned long long> mask;
  DevOwn<int2> tasks;
  unsigned long long n_tasks = 0;
  int range = 0, grp = 1;
};
struct SymDegrees {  // the 5-vertex closed forms (gm_sgl5_raw): the symmetric degrees of the DAG's vertices
  DevOwn<int> deg;
};
// local counts (gm_solve_local.hip), on the SYMMETRIC handle
struct RevIndex {  // per entry (u, v): the entry (v, u) (gm_ktruss / gm_truss_decompose / gm_clique_local)
  DevOwn<int> rev;
};
struct ListOffsets {  // triangle listing (gm_tc_list): the first slot of every batch of 64 entries of the oriented copy (batches + 1 values,
  DevOwn<unsigned long long> off;  // the last one T), counted and scanned by the first call and kept for the windows that follow
  unsigned long long total = 0;
};
struct CliqueListOffsets {  // k-clique listing (gm_clique_list), one per k: the first slot of every entry of the oriented copy (entries + 1
  DevOwn<unsigned long long> off;  // values, the last one the total), counted and scanned by the first call of that k
  unsigned long long total = 0;
};

// triangle nuclei (gm_nucleus34.hip), on the SYMMETRIC handle.  The index: a triangle's id is its slot in gm_tc_list's order
struct TriIndex {
  DevOwn<unsigned long long> off;  // entries of the oriented copy + 1: the exclusive scan of |N+(u) & N+(v)|, the last one T
  DevOwn<int> w, e;                // per triangle: the third vertex (ascending inside an entry's segment), the entry
  unsigned long long total = 0;
};
struct Nucleus34State {  // the peel's state, initialised by every call: K4(t), the marks, the frontier list, the 64 bytes of round words
  DevOwn<unsigned> cnt;
  DevOwn<unsigned char> mark;
  DevOwn<unsigned> front;
  DevOwn<unsigned long long> words;
};

struct gm_graph {
  int device = 0;
  int nv = 0;
  long long ne = 0;
  int max_deg = 0;
  DevOwn<int> d_rp;   // int32 offsets, owned
  DevOwn<long long> d_rp64;  // a BIG handle (ne >= 2^31): 64-bit offsets instead -- orientation, formula 3-motif and download only
  int *d_col = nullptr;  // col_idx: the view every reader uses -- d_col_mem's array, or the caller's (gm_graph_from_device: borrowed)
  DevOwn<int> d_col_mem;
  DevOwn<int> d_symdeg;  // a DAG made by gm_graph_orient: the degrees of the symmetric graph it came from (its topological numbering sorts by them)
  // ---- built on first use, published whole (the group structs above; gm_once.h) ------------------------------------------------------
  Once<DevOwn<int2>> edesc;  // per CSR entry: {rp[col[e]], degree(col[e])} (ensure_edesc, gm_tasks.hip; read by the table / task-list builds and fill_mine_params)
  Once<TaskLists> tasklists;
  Once<SupCorner> sup_corner;
  Once<SupMasks> sup_masks;
  Once<KeyStream> kst;
  Once<KeyEntries> kst_entries;
  Once<LongRows> long_rows;
  Once<HubCore> core;
  Once<CoreBlocks> core_blocks;
  Once<WideVerts> wide;
  GraphFacts facts;
  Once<RectIdx> rect_idx;
  Once<WedgeBlocks> wedge_blocks;
  Once<CentreTaskList> rect_tasks, house_tasks;
  Once<HouseTables> house_tables;
  Once<HouseBlocks> house_blocks;
  Once<RectLdsPlan> rect_lds;
  Once<HouseLdsPlan> house_lds;
  Once<WrectPlan> wrect;
  Once<RectLocalPlan> rect_local;
  Once<SymDegrees> w5deg;
  Once<RevIndex> lrev;
  Once<ListOffsets> list_off;
  Once<CliqueListOffsets> clique_list_off[6];  // k = 3 .. 8
  Once<TriIndex> tri_index;
  Once<Nucleus34State> nuc34;
  // gm_graph_sort_neighbors rewrites the rows: it refuses a handle on which one of these describes them already.  NOT checked (the list
  // predates them): core, core_blocks, long_rows, sup_corner, sup_masks, kst_entries, facts other than sum_c2, rect_lds, house_lds, wrect, rect_local,
  // w5deg, lrev, list_off, clique_list_off, tri_index, nuc34, relabel_cache[2], clique_plans -- most of them cannot exist without one that is
  bool rows_in_use() const {
    return !tables.empty() || edesc.built() || tasklists.built() || kst.built() || dag_cache || relabel_cache[0] || relabel_cache[1] || rect_idx.built() ||
           wedge_blocks.built() || rect_tasks.built() || house_tables.built() || house_tasks.built() || house_blocks.built() || !bitmap_sets.empty() ||
           wide.built() || facts.sum_c2.built();
  }
  // ---- keyed lists under g->mu, handed out whole ---------------------------------------------------------------------------------------
  std::list<ChunkTable> tables;          // list: handed-out pointers stay valid (get_table)
  std::list<BitmapSet> bitmap_sets;      // the hub rows' bitmaps, shared by the tables (get_table)
  // k-clique: the per-(rank, world, policy) plans of the two phases of the wide vertices (row-group chunks of phase 1, count classes of
  // phase 2, matrix offsets, arena rounds; get_clique_plan)
  std::list<CliquePlan> clique_plans;
  // ---- work buffers: grown on demand by the calls named, which is legal because one call at a time runs per handle; no protocol ---------
  struct DiamondWork {  // gm_diamond_support_* / the diamond of gm_sgl (gm_sup.hip): one counter per DAG entry
    DevOwn<unsigned> sup;
  } diamond;
  // gm_sgl5_raw / gm_sgl6_raw (gm_wtri.hip, gm_wrect.hip), on the DAG of the pass: a support array of their own (the diamond's is not
  // touched), d(u) + d(v) per entry, 2 T_v per vertex, the eight sums of one call, e1 per vertex of the 6-vertex forms
  struct ClosedFormWork {
    DevOwn<unsigned> sup, ed;
    DevOwn<unsigned long long> tv2, out;
    DevOwn<unsigned> s6e1;
  } w5;
  // gm_tc_local / gm_ktruss / gm_truss_decompose / gm_clique_local (gm_local.hip, gm_kcl_local.hip).  The DAG the triangle pass runs on has
  // a support array of the local counts' own (sup); the SYMMETRIC handle holds what lives in the caller's entry order: the supports /
  // peeling state, the marks, the frontier list, the trussness, the counters of a round
  struct LocalWork {
    DevOwn<unsigned> sup;    // per DAG entry (diamond_support_entries)
    DevOwn<unsigned> ent;    // per entry of the symmetric graph: the support of its edge; while peeling, exact at the canonical entries
    DevOwn<unsigned char> mark;
    DevOwn<int> front;       // ne / 2 + 1 canonical entries
    DevOwn<unsigned> truss;
    DevOwn<unsigned> cnt;    // 64 bytes: [0] frontier size, [1] 0xFFFFFFFF - smallest alive support
    // local k-clique counts, on the DAG the kernels run on: the k-cliques of every entry, the list of the rows beyond the LDS matrix, the
    // workgroups' scratch slots.  On the SYMMETRIC handle: the counts in the caller's entry order when the caller gives no array for them
    DevOwn<unsigned long long> kcl;   // per DAG entry: the counts, then (ne further values) the undivided sums of the out-edges
    DevOwn<int> kcl_heavy;            // ne / (kKclLocalLdsRow + 1) + 1 rows, then ne / (kKclLocalSplitRow + 1) + 1 split rows
    DevOwn<unsigned> kcl_scratch;
    size_t kcl_scratch_bytes = 0;
    DevOwn<unsigned long long> ent64; // per entry of the symmetric graph
    // k-clique listing, on the SYMMETRIC handle: the scratch slots of the rows beyond the LDS matrix (the local counts' slots are left alone)
    DevOwn<unsigned> kcl_list_scratch;
    size_t kcl_list_scratch_bytes = 0;
    // local 4-cycle counts, on the graph the walk runs on: the credits of every entry (zeroed by every call).  On the SYMMETRIC handle the
    // counts in the caller's entry order are ent64's, as for the k-cliques
    DevOwn<unsigned long long> racc;
    // local motif counts: on the DAG the credit pass runs on, the rim credits of every entry (zeroed by every call); on the SYMMETRIC
    // handle five vertex arrays of the call's own -- T_v, R_v, K_v, half the row sums of the credits, e1 -- and eight column sums
    DevOwn<unsigned long long> wacc;
    DevOwn<unsigned long long> orb;
    // k-clique cores (gm_kcl_core.hip), on the SYMMETRIC handle: K_v while peeling, the marks and the frontier list of the vertices (the
    // k-truss keeps its own, per entry), the 64 bytes of round words, the list of the frontier vertices of more than kKclLocalLdsRow
    // survivors and the wide kernel's scratch slots.  Core numbers and rounds go straight to the caller's arrays
    DevOwn<unsigned long long> core_cnt;
    DevOwn<unsigned char> core_mark;
    DevOwn<int> core_front;            // nv vertices
    DevOwn<unsigned long long> core_words;
    DevOwn<int> core_heavy;            // ne / (kKclLocalLdsRow + 1) + 1 vertices
    DevOwn<unsigned> core_scratch;
    size_t core_scratch_bytes = 0;
    // k-clique trusses (gm_kcl_truss.hip), on the SYMMETRIC handle: K_e per entry while peeling, the marks and the frontier list of the
    // canonical entries (the k-truss keeps its own over 32-bit supports), the 64 bytes of round words, the list of the frontier edges of
    // more than kKclLocalLdsRow survivors and the wide kernel's scratch slots.  theta and the rounds go straight to the caller's arrays
    DevOwn<unsigned long long> ktr_cnt;
    DevOwn<unsigned char> ktr_mark;
    DevOwn<int> ktr_front;             // ne / 2 + 1 entries
    DevOwn<unsigned long long> ktr_words;
    DevOwn<int> ktr_heavy;             // ne / 2 + 1 entries on a handle with a row beyond kKclLocalLdsRow, else one
    DevOwn<unsigned> ktr_scratch;
    size_t ktr_scratch_bytes = 0;
  } local;
  struct MapWork {  // the global counter maps of run_rect_acc / run_house_acc (rectangle, pentagon, house by wedge accumulation)
    DevOwn<unsigned> rect_acc;
    size_t rect_acc_bytes = 0;
    DevOwn<unsigned long long> house_acc;  // 64-bit maps
    size_t house_acc_bytes = 0;
    DevOwn<int> house_touched;
    DevOwn<int> pent_touched;              // touched-vertex lists (same shape as rect_acc)
    size_t pent_touched_bytes = 0;
  } maps;
  struct CliqueArena {  // launch_clique_wide (gm_clique, k = 4)
    DevOwn<unsigned> mat;      // matrix arena (largest round so far)
    size_t mat_bytes = 0;
    DevOwn<unsigned> queue;    // dequeue words of the wide launches of one call (zeroed per call)
  } arena;
  struct Scratch {  // the launch layer's per-call scratch (gm_launch.hip)
    DevOwn<unsigned> p;
    size_t bytes = 0;
  } scratch;
  // ---- the handle's own ---------------------------------------------------------------------------------------------------------------------
  DevOwn<int> d_newid;       // a copy made by get_relabeled, mode 0 (ascending in degree) or 2 (topological): id in the graph it was made from -> id here (nv)
  DevOwn<unsigned long long> d_counters;  // [4] + queue word, 64 B
  static constexpr int kEvRing = 64;  // HIP-event pairs of the most recent launches
  hipEvent_t ev[kEvRing][4] = {};      // [0], [1]: around the launch; [2], [3]: around its hub-corner kernel (gm_ctc.hip) when it has one
  bool ev_corner[kEvRing] = {};
  unsigned long long ev_launches = 0;
  int cu_count = 256;
  gm_graph *dag_cache = nullptr;          // oriented copy, built on demand by gm_motif_formula
  gm_graph *relabel_cache[3] = {nullptr, nullptr, nullptr};  // renumbered copies: by degree ascending / descending, topological (get_relabeled)
  bool topo_relabel_failed = false;  // the (degree, id) numbering is not topological for this DAG: it runs as given
  const gm_graph *ring_alias = nullptr;  // handle whose event ring holds this handle's most recent launch
  const gm_graph *ring_extra[2] = {nullptr, nullptr};  // 4-motif: the handles that ran the other sub-launches of the most recent calls (gm_kernel_times adds them)
  hipStream_t aux_stream[3] = {nullptr, nullptr, nullptr};  // class kernels that cannot fill the chip run beside the others (run_pattern)
  hipEvent_t aux_done[3] = {nullptr, nullptr, nullptr};
  TempPool pool;  // temporaries of the setup paths (PoolScope)
  bool counted = false;            // finish_handle has registered the handle with its device (dev_handle_born)
  gm_graph *pool_owner = nullptr;  // a derived handle (renumbered copy, cached orientation) borrows its owner's pool: the owner outlives it,
                                   // and one caller works on a handle family at a time -- a pool of its own is ~0.8 ms of hipMalloc
  gm_setup_times setup = {0, 0, 0, 0, 0};  // accumulated pre-processing time of this handle (gm_graph_setup_times)
  std::mutex mu;
  std::mutex dag_mu;  // guards the lazy creation of dag_cache (ensure_dag_cache, gm_launch.hip)
};

// Opens the handle's temp pool for the DevBufs of the enclosing setup function (nested scopes share it, stack discipline). The pool is
// ONE allocation per handle, made on first use and kept: 24 bytes per vertex + 16 MB, at most 256 MB -- room for the O(nv) and
// O(chunks) arrays of a table build; the sort buffers of a renumbering or a task-list build (O(ne), once per graph) fall through to
// hipMalloc. (A pool sized for everything and regrown per scope was measured first: allocating hundreds of MB per table cost more
// than the twenty small hipMallocs it replaced -- diamond R-MAT-22 table_ms 11.6 -> 40.)
struct PoolScope {
  gm_graph *g;
  TempPool *prev;
  size_t mark = 0;
  bool mine = false;  // this scope holds (a level of) the claim on the root's pool
  explicit PoolScope(gm_graph *g_) : g(g_), prev(g_temp_pool) {
    while (g->pool_owner) g = g->pool_owner;
    TempPool &pl = g->pool;
    {
      std::lock_guard<std::mutex> lk(pl.claim_mu);
      if (pl.depth == 0 || pl.owner == std::this_thread::get_id()) {
        pl.owner = std::this_thread::get_id();
        ++pl.depth;
        mine = true;
      }
    }
    if (!mine) {  // another thread is inside a scope of this handle family: no pool for this one
      g_temp_pool = nullptr;
      return;
    }
    if (!pl.base && !gm_opt("GM_NO_TEMP_POOL")) {
      const size_t need = std::min<size_t>((size_t)256 << 20, (size_t)24 * ((size_t)g->nv + 1) + ((size_t)16 << 20));
      if (pl.base.alloc(need) == hipSuccess) pl.cap = need;
      else (void)hipGetLastError();  // (no pool: everything falls through to hipMalloc)
    }
    mark = pl.off;
    g_temp_pool = &pl;
  }
  ~PoolScope() {
    (void)hipDeviceSynchronize();  // nothing may still be reading the temporaries when the next scope reuses them
    if (mine) {
      TempPool &pl = g->pool;
      pl.off = mark;
      std::lock_guard<std::mutex> lk(pl.claim_mu);
      --pl.depth;
    }
    g_temp_pool = prev;
  }
};

// wall-clock stopwatch for the setup accounting (host clock: the steps mix host work, copies and synchronised kernels)
struct SetupTimer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Device-to-host copies of the O(chunks) / O(hub rows) arrays of the setup paths.  The FIRST device-to-host copy of 64 KB or more in a
// process costs 8 - 10 ms of one-time initialisation inside the HIP runtime (pageable or pinned destination alike; copies of 16 KB
// do not take that path: 15 us each -- measured with a bare HIP program, profiles/r04/ab_setup_first_call.txt).  Up to 1 MB goes in
// 16 KB pieces, so a first call on a fresh process does not pay for it; larger copies are worth the real path.
inline hipError_t copy_to_host(void *dst, const void *src, size_t bytes) {
  constexpr size_t kPiece = (size_t)16 << 10;
  if (bytes > ((size_t)1 << 20)) return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  for (size_t o = 0; o < bytes; o += kPiece) {
    const hipError_t e = hipMemcpy((char *)dst + o, (const char *)src + o, std::min(kPiece, bytes - o), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

inline hipError_t copy_to_device(void *dst, const void *src, size_t bytes) {  // (the same one-time cost the other way round)
  constexpr size_t kPiece = (size_t)16 << 10;
  if (bytes > ((size_t)1 << 20)) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  for (size_t o = 0; o < bytes; o += kPiece) {
    const hipError_t e = hipMemcpy((char *)dst + o, (const char *)src + o, std::min(kPiece, bytes - o), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// GM_SETUP_TRACE: wall-clock marks of the setup steps on stderr, each after a device synchronisation (where do the milliseconds of a
// first call go: kernels, allocations, copies back?).  Off: one predictable branch.
inline void setup_trace(const char *what) {
  static const bool on = getenv("GM_SETUP_TRACE") != nullptr;
  if (!on) return;
  static std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  const auto t0 = std::chrono::steady_clock::now();
  (void)hipDeviceSynchronize();
  const auto t1 = std::chrono::steady_clock::now();
  fprintf(stderr, "[setup] %-34s %8.3f ms (+ %.3f waiting for the device)\n", what, std::chrono::duration<double, std::milli>(t0 - last).count(),
          std::chrono::duration<double, std::milli>(t1 - t0).count());
  last = std::chrono::steady_clock::now();
}

// scope guard: the enclosed once-per-graph pattern setup (device work included) is charged to setup.other_ms
struct OtherSetupScope {
  gm_graph *g;
  SetupTimer t;
  explicit OtherSetupScope(gm_graph *g_) : g(g_) {}
  ~OtherSetupScope() {
    (void)hipDeviceSynchronize();
    g->setup.other_ms += t.ms();
  }
};

// module warm-up: one no-op kernel per translation unit (each is its own code object, loaded on first launch -- 20 ms for the unit
// with the hipCUB instantiations: without this the first table build / first mining launch of a process pays for it)
void gm_touch_mine();
void gm_touch_mine_wide();
void gm_touch_hrow();
void gm_touch_tch();
void gm_touch_sup();
void gm_touch_wtri();
void gm_touch_wrect();
void gm_touch_rect_local();
void gm_touch_orbit_local();
void gm_touch_local();
void gm_touch_list();
void gm_touch_kcl_local();
void gm_touch_kcl_core();
void gm_touch_kcl_truss();
void gm_touch_nucleus34();
void gm_touch_clique_list();
void gm_touch_cbuild();
void gm_touch_cmma();
void gm_touch_cgather();
void gm_touch_ctc();
void gm_touch_sgl();
void gm_touch_tables();
void gm_touch_tasks();
void gm_touch_clique_plan();
void gm_touch_launch();
void gm_touch_tools();

// ---- across translation units ---------------------------------------------------------------------------------------------
int finish_handle(gm_graph *g);                                 // gm_graph.hip: counters, events, CU count of a new handle
int host_rp(gm_graph *g, const std::vector<int> **out);          // gm_graph.hip: host copy of the offsets, fetched on first use
int convert_offsets(const int64_t *rp64, int nv, long long ne, std::vector<int> &out);  // gm_graph.hip: host-side narrowing / validation
int get_relabeled(gm_graph *g, int mode, gm_graph **out);  // gm_graph.hip: cached renumbered copy (0 / 1 by degree, 2 topological)
int graph_is_topological(gm_graph *g, bool *out);
int graph_rows_sorted(gm_graph *g, bool *out);
int ensure_long_rows(gm_graph *g);  // (gm_tasks.hip) g->long_rows: the rows of more than kTctStageMax entries
int ensure_core_tri(gm_graph *g);     // (gm_clique_plan.hip) g->core_blocks of a handle with a core bitmap; GM_OK also when not applicable
int ensure_core_bitmap(gm_graph *g);  // (gm_clique_plan.hip) g->core of a topologically numbered DAG; GM_OK also when not applicable
int get_table(gm_graph *g, int target, bool allow_split, int bit_words, unsigned long long part_cap, int stage_cap, ChunkTable **out,
              const RowFilter &rf = RowFilter(), int bitmap_min_deg = kBitmapMinDeg);
// (gm_tables.hip) one table on the device, into `t` (its parameters set by the caller: get_table, and the host-chunk tables of the clique
// rounds); trp / tlen / tstride: the task lists the costs of an rf.tct table are counted from; default: the graph's, gm_tch.hip
int build_table_device(gm_graph *g, ChunkTable &t, bool sym_table, double &bitmap_ms, const int *trp = nullptr, const int *tlen = nullptr, int tstride = 2);
void launch_gather_deg(int m, const int *verts, const int *rp, int *deg);  // (gm_tables.hip) deg[i] = the length of row verts[i]
// The placement passes that walk the rows eight lanes each (task_rows_kernel / kst_rows_kernel, gm_tasks.hip; cb_task_rows_kernel,
// gm_clique_plan.hip) count the in-edge tasks of the last kHubWin hosts of a topologically numbered DAG in an LDS histogram per workgroup;
// their grid: 8 rows per wave and trip, at most per_cu workgroups per CU
constexpr int kHubWin = 4096;
inline dim3 row_walk_grid(const gm_graph *g, int per_cu) {
  return dim3((unsigned)std::max<long long>(1, std::min<long long>(((long long)g->nv * 8 + 255) / 256, (long long)g->cu_count * per_cu)));
}
int ensure_edesc(gm_graph *g);  // (gm_tasks.hip)
int ensure_tasklists(gm_graph *g);
int ensure_keystream(gm_graph *g, bool edges, bool *built, bool allow_core = false);  // allow_core: the rows of the hub core may stay out (gm_ctc.hip)
int sup_mask_min_tail(const gm_graph *g);  // (gm_tasks.hip) kSupMaskMinTail or the option GM_SUP_MASK_MIN when the handle's masks were laid out
int ensure_sup_corner(gm_graph *g);  // (gm_tasks.hip) g->sup_corner of a handle whose task lists leave a hub corner out
int ensure_sup_masks(gm_graph *g);  // (gm_tasks.hip) g->sup_masks of a topologically numbered DAG with task lists; GM_OK also when not applicable
int ensure_mean_sq_deg(gm_graph *g);
int ensure_tri_per_edge(gm_graph *g);  // (gm_launch.hip) |N+(u) ^ N+(v)| averaged over a sample of the DAG's entries
unsigned long long task_part_cap(gm_graph *g, int world);
int clique_wide_min_words();
int get_clique_plan(gm_graph *g, int rank, int world, int policy, int target, unsigned long long part_cap, CliquePlan **out);
