// gm_launch.h -- the launch layer's internal interface: what the solver units (gm_launch.hip, gm_solve_sgl.hip, gm_solve_local.hip) share.
// A solver family is a unit of its own that includes this header; what is not declared here belongs to one unit.  Included by those units only.
#pragma once
#include "gm_host.h"

// What varies per call of run_pattern (gm_launch.hip), beside (handle, launch, h_out, nout, stats).
struct PatternReq {
  Pattern pat;
  int k;
  int fin_mode = -1;                // < 0: FIN_MOTIF3 for PAT_MOTIF3, else FIN_COPY (FinMode, below)
  unsigned long long fin_base = 0;  // FIN_MOTIF3_FORMULA: sum_v C(d, 2)
  unsigned *sup_out = nullptr;      // PAT_SUPPORT_PART's buffer
  bool wtri_tri = false, wtri_vert = false;  // PAT_WTRI: the second pass over the triangles (A, B) / the per-vertex sums (H, S) are wanted
  const unsigned *credit_sup = nullptr;      // PAT_ORBIT: the complete supports of the handle's entries ...
  unsigned long long *credit_w = nullptr;    // ... and the per-entry accumulator of the rim credits (zeroed inside the timed region)
};
int run_pattern(const PatternReq &rq, const gm_graph *cg, const gm_launch *la, uint64_t *h_out, int nout, gm_stats *st);

// (what follows is shared by the launch units only: it stays out of the library's symbol table)
#pragma GCC visibility push(hidden)

enum FinMode : int { FIN_COPY = 0, FIN_MOTIF3 = 1, FIN_MOTIF3_FORMULA = 2, FIN_RAW4 = 3, FIN_HALF_SIGNED = 4 };

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
inline unsigned *queue_word(const gm_graph *g, int w) { return reinterpret_cast<unsigned *>(g->d_counters + 4) + w; }
inline unsigned long long *queue_word64(const gm_graph *g, int w) { return reinterpret_cast<unsigned long long *>(queue_word(g, 2 * w)); }

inline gm_launch launch_or_default(const gm_launch *la) { return la ? *la : gm_launch{}; }  // the caller's launch descriptor, or the all-zero default

int reject_big(const gm_graph *g);     // GM_ERR_TOO_LARGE for a big handle (ne >= 2^31, 64-bit offsets)
int require_sorted_rows(gm_graph *g);  // GM_ERR_INVALID and the text that names gm_graph_sort_neighbors for a handle with unsorted rows
int begin_launch(const gm_graph *cg, const gm_launch *la, const uint64_t *h_out, LaunchCtx &c);
int start_timer(LaunchCtx &c);
int end_launch(LaunchCtx &c, int fin_mode, unsigned long long fin_base, uint64_t *h_out, int nout, gm_stats *st);

inline void fill_stats(gm_stats *st, uint64_t tasks, uint64_t chunks, int grid, int block) {
  if (!st) return;
  st->kernel_ms = 0.0;
  st->tasks = tasks;
  st->chunks = chunks;
  st->grid = (uint32_t)grid;
  st->block = (uint32_t)block;
}

// The sub-launches of a call that is several launches: each runs with a fresh gm_stats (`last`), their kernel times add up in `ms`.
struct SubLaunches {
  double ms = 0.0;
  gm_stats last;
  template <class Run>
  int run(Run run) {  // run(gm_stats *): one sub-launch (a failed one ends the call: its time is not counted)
    memset(&last, 0, sizeof last);
    const int rc = run(&last);
    ms += rc == GM_OK ? last.kernel_ms : 0.0;
    return rc;
  }
};

// Where gm_kernel_times / gm_corner_times find the launches of the call that just ended on `caller`: in the event ring of `run_on` (the
// caller itself: no alias).  set_extras: x0 / x1 become the handles whose launches of equal recency are added (the two other handles a
// 4-motif ran on; none: cleared); otherwise they stay as they are.  This function and start_timer are the only writers of ring_alias / ring_extra.
inline void record_ran_on(const gm_graph *caller, const gm_graph *run_on, bool set_extras = false, const gm_graph *x0 = nullptr, const gm_graph *x1 = nullptr) {
  gm_graph *c = const_cast<gm_graph *>(caller);
  c->ring_alias = run_on != caller ? run_on : nullptr;
  if (set_extras) c->ring_extra[0] = x0, c->ring_extra[1] = x1;
}
// ... of a call on a symmetric handle that ran on `run_on` through its cached oriented copy
inline void record_ran_on_dag(const gm_graph *sym, const gm_graph *run_on) {
  record_ran_on(sym->dag_cache, run_on);
  record_ran_on(sym, sym->dag_cache, true);
}

// the in-edge tasks stream only the part of N+(u) beyond v: a topologically numbered DAG (GM_TC_NO_TRIM: A/B, whole lists)
inline bool tails_trimmed(const gm_graph *g) { return *g->facts.topological && !gm_sweep_env("GM_TC_NO_TRIM"); }

// workgroups of a launch: one per unit of work, at most per_cu on every CU, at least one
inline int clamp_grid(long long want, long long cap) { return (int)std::max<long long>(1, std::min<long long>(want, cap)); }
inline int grid_for(long long count, int cu_count, long long per_cu) { return clamp_grid(count, (long long)cu_count * per_cu); }

// a device buffer of a handle, grown to `need` bytes (never shrunk; the old contents are not kept)
template <class T>
int grow_dev(DevOwn<T> &buf, size_t *bytes, size_t need) {
  if (need <= *bytes) return GM_OK;
  *bytes = 0;
  HIP_TRY(buf.alloc(need));
  *bytes = need;
  return GM_OK;
}
inline int ensure_scratch(gm_graph *g, size_t need) { return grow_dev(g->scratch.p, &g->scratch.bytes, need); }

// this rank's share of n units (gm_partition) as the first / step / count of a kernel's parameters; returns the count
template <class P>
int64_t take_range(const LaunchCtx &c, int64_t n, P &p) {
  int64_t first = 0, step = 1, count = 0;
  gm_partition(n, c.rank, c.world, c.la.policy, &first, &step, &count);
  p.first = (decltype(p.first))first;
  p.step = (decltype(p.step))step;
  p.count = (decltype(p.count))count;
  return count;
}

// the CSR of a handle as the kernels see it (the optional tables stay nullptr: whoever needs one fills it in)
inline GraphView graph_view(const gm_graph *g) {
  GraphView gv;
  gv.nv = g->nv;
  gv.ne = (int)g->ne;
  gv.rp = g->d_rp;
  gv.col = g->d_col;
  return gv;
}

int topo_view(const gm_graph *dag, const gm_launch *la, gm_graph **run_on);  // the handle a DAG kernel runs on: the DAG or its cached topological copy
int run_tc(const gm_graph *dag, const gm_launch *la, uint64_t *out, int nout, gm_stats *st, int fin_mode = -1, unsigned long long fin_base = 0);
int ensure_dag_cache(gm_graph *g);  // the oriented copy of a symmetric handle, built once
// gm_solve_sgl.hip: the handle the edge supports of a symmetric graph run on; the rectangle kernels (gm_motif4_partial takes them too)
int diamond_run_on(const gm_graph *sym, const gm_launch *la, gm_graph **run_on);
int ensure_idx0(gm_graph *g, const GraphView &gv);  // the neighbours below every vertex (RectIdx), built once per graph
int run_rect_acc(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st, bool pentagon = false);
int run_rect_flat(const gm_graph *cg, const gm_launch *la_in, uint64_t *h_out, gm_stats *st, bool pentagon = false);

#pragma GCC visibility pop
