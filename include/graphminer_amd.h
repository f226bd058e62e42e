/*
 * graphminer_amd.h -- C ABI of the MI355X-native subgraph-matching hot path.
 *
 * One shared object (graphminer_amd/libgraphminer_amd.so), plain pointers and sizes,
 * no C++/torch types. It is the drop-in boundary for GraphMiner's link-time solver
 * seam: each reference solver
 *     void TCSolver    (Graph&, uint64_t& total, int n_gpu, int chunk)            src/triangle/main.cc:5
 *     void SglSolver   (Graph&, Pattern&, uint64_t& total, int n_dev, int chunk)  src/sgl/main.cc:7
 *     void CliqueSolver(Graph&, int k, uint64_t& total, int, int)                 src/clique/main.cc:6
 *     void MotifSolver (Graph&, int k, std::vector<uint64_t>&, int, int)          src/motif/main.cc:7
 * becomes a ~10 line shim over gm_tc / gm_sgl / gm_clique / gm_motif (see INTEGRATION.md
 * and graphminer_amd/host/solvers.cc and integration/hip_solvers.cc, which are exactly that shim).
 *
 * Conventions
 *   - every entry point returns a gm_status (0 = ok); nothing calls exit().
 *   - host pointers are borrowed for the duration of the call only.
 *   - device buffers are owned by the opaque gm_graph handle.
 *   - outputs are WRITTEN, not accumulated (the reference multi-GPU solvers '+=' into
 *     a caller-zeroed total, src/triangle/multigpu.cu:84; the shim does that '+=').
 *   - vertex ids int32, CSR offsets int64, counts uint64 (include/common.h:36-40).
 *   - there is NO CPU fallback: without a HIP device every compute call fails with
 *     GM_ERR_NO_DEVICE.
 */
#ifndef GRAPHMINER_AMD_H
#define GRAPHMINER_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gm_status {
  GM_OK = 0,
  GM_ERR_INVALID = 1,      /* bad argument (null pointer, k out of range, ...) */
  GM_ERR_NO_DEVICE = 2,    /* no HIP device / HIP runtime error before launch */
  GM_ERR_HIP = 3,          /* HIP runtime error (see gm_last_error) */
  GM_ERR_TOO_LARGE = 4,    /* outside the 32-bit task index of the mining kernels: a solver asked to walk a graph of >= 2^31 entries
                              itself (such a graph CAN be uploaded, oriented, downloaded and 3-motif-counted), nv >= 2^31-1, or an
                              oriented graph of >= 2^31 entries */
  GM_ERR_UNSUPPORTED = 5,  /* pattern / k not implemented ("Not implemented", src/sgl/omp_base.cc:51) */
  GM_ERR_IO = 6,           /* file could not be opened / short read (custom_alloc.h:38-41) */
  GM_ERR_FORMAT = 7        /* meta.txt violates the loader asserts (src/common/graph.cc:30-34) */
} gm_status;

const char *gm_strerror(int status);
/* thread-local text of the last failing HIP call made through this library */
const char *gm_last_error(void);
int gm_version(void);

/* Exactly what Graph::V()/E()/get_max_degree()/out_rowptr()/out_colidx() expose
 * (include/graph.h:63-64,73,83-84). Host pointers. */
typedef struct gm_csr {
  int32_t nv;
  int64_t ne;
  int32_t max_deg;
  const int64_t *row_ptr; /* nv+1 */
  const int32_t *col_idx; /* ne, rows strictly ascending */
} gm_csr;

/* Device-resident CSR (+ task-chunk tables). Replaces GraphGPU, include/graph_gpu.h:6-211. */
typedef struct gm_graph gm_graph;

int gm_device_count(int *n);

/* GraphGPU::init (include/graph_gpu.h:69-122): H->D copy of row_ptr / col_idx on `device`.
 * ne >= 2^31 (twitter40, friendster: src/triangle/README.md:60-61; eidType is int64, include/common.h:37) gives a BIG handle: it keeps
 * 64-bit offsets and supports gm_graph_orient (the oriented graph must have < 2^31 entries: then gm_tc / gm_clique run on it),
 * gm_motif(k = 3) / gm_motif_formula (the formula solver), gm_graph_meta / _download / _free; every other solver -> GM_ERR_TOO_LARGE. */
int gm_graph_upload(const gm_csr *host, int device, gm_graph **out);
/* Adopt CSR arrays that already live in HBM (e.g. built on the GPU); the arrays are BORROWED
 * and must outlive the handle. d_row_ptr is int64[nv+1], d_col_idx int32[ne]. */
int gm_graph_from_device(int32_t nv, int64_t ne, const int64_t *d_row_ptr, const int32_t *d_col_idx,
                         int device, gm_graph **out);
/* Graph::orientation (src/common/graph.cc:233-279) on the GPU: keep s->d iff
 * deg[d] > deg[s] || (deg[d] == deg[s] && d > s). Returns a new handle. */
int gm_graph_orient(const gm_graph *sym, gm_graph **dag);
/* Graph::sort_neighbors (src/common/graph.cc:138-146), the `adj_sorted = 0` case of tc_* (src/triangle/main.cc:22): sorts
 * every row ascending, in place on the device (one segmented radix sort). Every solver assumes sorted rows, so call it
 * before the first solver / gm_graph_orient result is used; after a solver has run on the handle -> GM_ERR_INVALID. */
int gm_graph_sort_neighbors(gm_graph *g);
/* nv / ne / max_deg of a handle (pointers in *meta are left NULL). */
int gm_graph_meta(const gm_graph *g, gm_csr *meta);
/* D->H copy (row_ptr: nv+1 int64, col_idx: ne int32); either pointer may be NULL. */
int gm_graph_download(const gm_graph *g, int64_t *row_ptr, int32_t *col_idx);
/* The renumbered copy the solvers take for this handle, BORROWED (owned by g, freed with it; do not gm_graph_free it): mode 0 / 1 ids
 * ascending / descending in degree (the SgL kernels), 2 the topological numbering of an oriented graph (TC, k-clique; *view == g when
 * the handle is a DAG that some other rule oriented). A permutation of the same graph with every row ascending; built once on the device
 * (the reference has no counterpart: its kernels walk the graph as numbered, src/common/graph.cc:233-279). For tests and tools. */
int gm_graph_renumbered(gm_graph *g, int mode, gm_graph **view);
void gm_graph_free(gm_graph *g);

/* Scheduler policy for the multi-GPU task split (include/scheduler.h, src/common/scheduler.cc). */
enum {
  GM_PART_ROUND_ROBIN = 0, /* Scheduler::round_robin, scheduler.cc:34-85: the j-th chunk of the dequeue order -> rank
                              j mod world (order = estimated work, heaviest first, when world > 1) */
  GM_PART_RANGE = 1,       /* even contiguous split of the task chunks (EVEN_SPLIT, src/clique/multigpu.cu:42-44) */
  GM_PART_VERTEX = 2       /* vertex-balanced: rank r owns the tasks of vertices [nv*r/world, nv*(r+1)/world)
                              (1-D vertex ranges of src/common/graph_partition.cc:82-132, without the halo copies:
                              the CSR is replicated); solvers only, gm_partition treats it like GM_PART_RANGE */
};

typedef struct gm_launch {
  void *stream;       /* hipStream_t; NULL = the null stream */
  int32_t rank;       /* this process' share of the task chunks: rank in [0, world) */
  int32_t world;      /* 0 or 1 = single GPU */
  int32_t policy;     /* GM_PART_* */
  int32_t chunk;      /* tasks (edges) per scheduling chunk; 0 = library default. Reference default 1024
                         (src/triangle/main.cc:16) */
  uint64_t *d_counts; /* optional DEVICE buffer (>= ncounts uint64). When set the result is left on the
                         device, no host sync is done (use it to feed an RCCL all-reduce). */
  int32_t tune[8];    /* kernel tuning / ablation knobs, all 0 = defaults. Counts never depend on them
                         (tests/test_gpu_parity.py) unless a bit is marked "ablation" (work is skipped, counts wrong).
                         [0] task edges per chunk, [1] chunks per dequeue, [2] xs+1 and [3] ys+1 of the direction rule
                         b*(xb+xs*lg a) <= a*(yb+ys*lg b), [4] workgroups per CU, [5] 1 = never stage adjacency in LDS,
                         [7] bits 0..7 xb*16+yb, bits 8.. price of a pass-Y key against a bitmapped row (0 = as a bisection).
                         [6] bit mask of GM_T6_* (below). */
} gm_launch;

/* The bits of gm_launch.tune[6]. The values are ABI (callers pass them as numbers): they never change.
 * Two names may share a value where two solvers read the same bit differently. */
enum {
  /* ---- alternative implementations (same counts) ---- */
  GM_T6_NO_HUB_BITMAPS = 0x100,        /* mining kernels ignore the hub bitmaps */
  GM_T6_AS_NUMBERED = 0x200,           /* SgL / TC / 4-clique on the graph as numbered (no degree / topological renumbering) */
  GM_T6_SGL_NESTED = 0x400,            /* SgL wave-per-edge loop nests (diamond: the reference's listing form) */
  GM_T6_SGL_FLAT = 0x800,              /* rectangle / pentagon as wedges + flat intersections, house flattened over (v0,v1,v3) */
  GM_T6_EAGER_PARTS = 0x1000,          /* cut every chunk above 4096 estimated entries into parts */
  GM_T6_SWAP_ORDERS = 0x2000,          /* swap the two dequeue orders */
  GM_T6_CHUNK_ID_ORDER = 0x4000,       /* plain chunk-id order */
  GM_T6_HOUSE_NO_BITMAP = 0x8000,      /* house: flattened form without the LDS S-bitmap */
  GM_T6_GLOBAL_MAPS = 0x20000,         /* rectangle / house with every counter map in global memory */
  GM_T6_CLIQUE4_MINING = 0x40000,      /* 4-clique in the mining kernel alone (its arena path; no two-phase re-hosted build) */
  GM_T6_NO_CLASSES = 0x80000,          /* per-edge kernels: every row through the general kernel (SPLIT chunks, dense HBM bitmaps) */
  GM_T6_FORCE_CLASSES = 0x100000,      /* per-edge kernels: the workgroup classes also on a graph without long rows */
  GM_T6_KCLIQUE_ANY_WIDTH = 0x200000,  /* k >= 5: the any-width pair count instead of the tile walk */
  GM_T6_CLASSES_SORTED_COPY = 0x400000, /* class kernels: the sorted LDS copy + bit filter + bisection instead of the hashed set */
  GM_T6_HSET_FALLBACK = 0x800000,      /* hashed sets on their global-memory fallback lookup */
  GM_T6_GIANT_SPLIT = 0x1000000,       /* giant rows stay SPLIT chunks of the general kernel (no hashed sets of row pieces) */
  GM_T6_HROW_MUL32 = 0x2000000,        /* hashed-row classes: the 32-bit multiply of id spaces beyond 2^24 */
  GM_T6_TC_CHUNKED = 0x4000000,        /* TC by the chunked mining kernel (default: the shorter list of every edge against a
                                          hashed set, gm_tch.hip) */
  GM_T6_CLIQUE4_ROW_GATHER = 0x8000000, /* 4-clique: the wide rows of the hub core gathered row by row from the core bitmap
                                           (default: by blocks of core rows resident in LDS) */
  GM_T6_PER_EDGE = 0x10000000,         /* diamond / 3-motif by one intersection of the two symmetric lists per edge (the reference's
                                          loop nests; default: from the triangles of the oriented copy) */
  GM_T6_NO_KEYSTREAM = 0x20000000,     /* TC / edge supports without the key stream: every edge a task of the lists, read from their rows */
  GM_T6_SUP_ATOMICS = 0x40000000,      /* edge supports (diamond) with one atomic per streamed edge instead of the match masks (gm_sup.hip) */
  /* ---- ablation (mining kernels: work is skipped, counts wrong) ---- */
  GM_T6_ABL_SKIP_CLIQUE_PHASE2 = 0x1,  /* skip clique phase 2 */
  GM_T6_ABL_SKIP_BITMATRIX = 0x2,      /* skip bit-matrix writes */
  GM_T6_ABL_NO_FILTER = 0x4,           /* no filter */
  GM_T6_ABL_FILTER_STAGE0 = 0x8,       /* filtered-pass stages, first */
  GM_T6_ABL_FILTER_STAGE1 = 0x10,      /* filtered-pass stages, second */
  GM_T6_ABL_FILTER_STAGE2 = 0x20,      /* filtered-pass stages, third (k >= 5: the per-sub-tree walk everywhere, same counts) */
  GM_T6_ABL_SKIP_SPLIT = 0x40,         /* skip SPLIT chunks */
  GM_T6_ABL_ONLY_SPLIT = 0x80,         /* only SPLIT chunks */
  GM_T6_ABL_SKIP_PASS_X = 0x400,       /* skip pass X */
  GM_T6_ABL_SKIP_PASS_Y = 0x8000,      /* skip pass Y */
  /* ---- the low 16 bits reach the mining kernels as they are (MineParams::flags bits 1..16, gm_mine.hip) ---- */
  GM_T6_KERNEL_FLAGS_MASK = 0xffff
};

typedef struct gm_stats {
  double kernel_ms;  /* HIP-event time of the mining kernel(s) on the launch stream (0 when d_counts is set
                        and the call did not synchronise) */
  uint64_t tasks;    /* "edges processed" as the reference's TEPS line defines nnz (src/triangle/gpu_base.cu:69) */
  uint64_t chunks;   /* task chunks owned by this rank */
  uint32_t grid;     /* workgroups launched */
  uint32_t block;    /* threads per workgroup */
} gm_stats;

/* The multi-GPU task split as index arithmetic: rank owns chunk ids first + i*step, i in [0,count).
 * Host-only (no device needed). */
int gm_partition(int64_t n_chunks, int32_t rank, int32_t world, int32_t policy, int64_t *first, int64_t *step,
                 int64_t *count);
/* Host-only view of the task-chunk table the solvers build for a CSR: recs receives up to `cap` records
 * {u_begin, u_end, e_begin, e_end} (4 x int32 each); *n_out = number of chunks. for_clique = 1 gives the
 * table of gm_clique (whole rows only). */
int gm_chunk_table(int32_t nv, const int64_t *row_ptr, int32_t chunk, int32_t for_clique, int32_t *recs, int64_t cap,
                   int64_t *n_out);

/* Pre-processing ("setup") accounting. The reference leaves these steps untimed ("Time on generating the DAG",
 * "Time on generating the edgelist", src/common/graph.cc:233-279,297-326); here every handle accumulates the wall-clock
 * milliseconds (host clock around device work + host work, synchronised) it has spent in them, so that a caller can report
 * them beside the kernel time:
 *   orient_ms   gm_graph_orient that produced this handle (recorded on the DAG handle)
 *   table_ms    task-chunk tables: chunk records, cost estimate, parts, dequeue orders (all tables built so far)
 *   bitmap_ms   hub-row bitmaps (symmetric-graph patterns)
 *   relabel_ms  renumbered copies (SgL patterns, clique topological numbering), including their own setup
 *   other_ms    per-pattern tables (idx0, 2-path estimates, per-entry triangle tables, task lists)
 * Cached structures cost nothing on later calls. */
typedef struct gm_setup_times {
  double orient_ms, table_ms, bitmap_ms, relabel_ms, other_ms;
} gm_setup_times;
int gm_graph_setup_times(const gm_graph *g, gm_setup_times *out);

/* HIP-event durations (ms) of the mining kernels of the most recent launches on this handle, oldest
 * first; at most 64 are remembered. The caller must have synchronised the launch stream(s).
 * This is how an asynchronous (d_counts) caller reads the kernel time the reference prints as
 * "runtime [gpu_base]" (src/triangle/gpu_base.cu:53-68). */
int gm_kernel_times(const gm_graph *g, int n, double *ms_out, int *n_out);
/* The part of those durations spent in the launch's hub-corner kernel on the matrix cores (csrc/gm_ctc.hip; 0 for a launch without one):
 * the rest is the streamed kernels' -- the time bench.py prices against the HBM roofline. Same order, same synchronisation rule. */
int gm_corner_times(const gm_graph *g, int n, double *ms_out, int *n_out);

/* ---- solvers ------------------------------------------------------------------------------ */
/* launch may be NULL (single GPU, null stream, defaults). stats may be NULL. */

/* TCSolver: total = sum_{(u,v) in DAG} |N+(u) ^ N+(v)|  (src/triangle/omp_base.cc:15-21,
 * src/triangle/gpu_kernels/bs_warp_edge.cuh:2-18). `dag` must be an ORIENTED graph. */
int gm_tc(const gm_graph *dag, const gm_launch *launch, uint64_t *total, gm_stats *stats);
/* Tooling (tests, the byte model of bench.py): on a DAG whose hubs are its last ids (the topologically renumbered copy of a graph with long
 * rows) the triangles whose smallest member is one of the last H vertices are counted as ONE masked bit-matrix product on the matrix
 * cores (csrc/gm_ctc.hip: sum_{i<j, M_ij} popc(M_i & M_j) over the H x H corner of the adjacency matrix -- the loop of omp_base.cc:15-21 on
 * bit rows) and the streamed kernel takes every other edge.  After a first gm_tc: info[0] = H (0: no such corner on this handle),
 * info[1] = DAG entries inside the corner, info[2] = 64 x 64 blocks of the product, info[3] = vertices of the core bitmap.
 * gm_dev_option("GM_TC_CORE_H", ..) (read when the handle's key stream is built): 0 = off, any other value = that H. */
int gm_tc_core_info(const gm_graph *dag, int64_t info[4]);
/* ... and, since the corner is chosen per PAIR of 256-row blocks (IB <= JB) of a region at the end of the core bitmap -- a pair goes to
 * the product iff the keys the stream would move for its edges, times R, exceed the pair's 65536 * (region - 512 * (JB >> 1)) bit-products --
 * what was chosen: info[0] = rows of the region (0: no selection on this handle), [1] = pairs taken, [2] = pairs that hold keys,
 * [3] = DAG entries in the product, [4] = modelled keys moved out of the stream, [5] = R.  gm_tc_core_info keeps describing the base corner
 * of the density rule.  gm_dev_option (read when the handle's key stream is built): "GM_TC_PAIRS" = rule (default) | off (the full triangle
 * of the base corner) | all | none | checker | diag | offdiag, "GM_TC_PAIR_R" = R, "GM_TC_PAIR_REGION" = rows of the region whatever the
 * density rule says (tests).  A forced GM_TC_CORE_H means the full triangle of that size, no selection. */
int gm_tc_pairs_info(const gm_graph *dag, int64_t info[6]);
/* the rule itself, on the host: keys[IB * nb + JB] (nb = region / 256 <= 128) -> bit IB * nb + JB of
 * bits[(nb * nb + 31) / 32] for every pair taken; returns their number, < 0 for invalid arguments */
int gm_tc_pair_rule(const uint32_t *keys, int nb, int region, uint64_t R, uint32_t *bits);

/* SglSolver: edge-induced subgraph listing on the SYMMETRIC graph, pattern by NAME
 * (include/pattern.hh:62-78). Implemented: "diamond" (src/sgl/cpu_kernels/diamond.h:1-14,
 * src/sgl/gpu_kernels/diamond_count.cuh:3-21), "rectangle" (rectangle.h:1-11), "house" (house.h:1-16),
 * "pentagon" (pentagon.h:2-17), and -- one rank (several: gm_sgl4_partial), from the per-edge sums of the formula 4-motif, no enumeration of their own --
 * "tailedtriangle" (tailedtriangle.h:1-12), "4path" (4path.h:1-14), "3star" (3star.h:1-13), and -- one rank, no d_counts: gm_sgl5_raw
 * followed by gm_sgl5_finish, closed forms over edge supports, triangles and degrees -- "5path", "semihouse", "closedhouse", "hourglass",
 * "taileddiamond", "taileddiamond2" (src/sgl/cpu_kernels/ of the same names).  Others ("6path", "dumbbell", src/sgl/omp_base.cc:46-49)
 * -> GM_ERR_UNSUPPORTED, *total = 0: "6path" and "dumbbell" are counted by gm_sgl6 below, behind entry points of their own -- an existing
 * test pins this call's answer for the two names, and routing them to gm_sgl6 is a later one-line change that goes with that test.
 * With world > 1 a rank's house / pentagon value is a partial MODULO 2^64 (a centre's positive and negative terms may be tasks of different
 * ranks): add the ranks' values as uint64 (an all-reduce does), do not compare a single rank's value with anything.
 * rectangle / house keep the counter maps of their heavy centres in LDS (gm_mine.hip rect_lds_kernel / house_lds_kernel; tune[6] & GM_T6_GLOBAL_MAPS:
 * in global memory, round 5's form).
 * diamond = sum over the edges of C(|N(v0) ^ N(v1)|, 2). One GPU: |N(v0) ^ N(v1)| of every edge -- its triangles -- from ONE pass over
 * the triangles of the oriented copy (edge supports, gm_sup.hip; the copy is built and cached on first use; also for a graph of
 * >= 2^31 entries); world > 1, a DAG row beyond 2048 entries, or tune[6] & GM_T6_PER_EDGE: one intersection of the two symmetric lists per
 * edge (gm_hrow.hip, gm_chunk.h). Same count. */
int gm_sgl(const gm_graph *sym, const char *pattern, const gm_launch *launch, uint64_t *total, gm_stats *stats);

/* tailedtriangle / 4path / 3star on SEVERAL ranks (the reference's sgl has no multi-GPU binary for them; same contract as
 * gm_motif4_partial): every rank calls gm_sgl4_partial for its share of the four per-edge sums (plain sums over its tasks; with
 * launch->d_counts they are left in that device buffer without synchronising and raw may be NULL), the ranks all-reduce raw[0..3],
 * then gm_sgl4_finish(pattern, raw, &total) applies the pattern's closed form.  gm_sgl itself refuses world > 1 for these three. */
int gm_sgl4_partial(const gm_graph *sym, const gm_launch *launch, uint64_t raw[4], gm_stats *stats);
int gm_sgl4_finish(const char *pattern, const uint64_t raw[4], uint64_t *total);

/* The six 5-vertex patterns (hourglass, taileddiamond, taileddiamond2, semihouse, closedhouse, 5path) as closed forms of eleven raw sums
 * (DESIGN.md "SgL, 5-vertex closed forms"; t(e) = edge support, x = t - 1, d = degree, T_v = triangles at v, uint64 modulo 2^64):
 *   raw[0] T = triangles          raw[1] D = sum_e C(t,2)               raw[2] W = sum_e C(t,2) (d(u) + d(v) - 6)
 *   raw[3] A = sum_tri [x(bc)(d(a)-2) + x(ac)(d(b)-2) + x(ab)(d(c)-2)]   raw[4] B = sum_tri [x(ab)x(ac) + x(ab)x(bc) + x(ac)x(bc)]
 *   raw[5] H = sum_v C(T_v,2)     raw[6] S = sum_v T_v d(v)             raw[7] P = sum_v (e1(v)^2 - p2(v)) / 2
 *   raw[8] K4 = 4-cliques         raw[9] R = the rectangle count        raw[10] Q = sum_e (t - 2) sum_{c in S_e} |S_e ^ N(c)|
 *   hourglass = H - 2 D, taileddiamond2 = W, taileddiamond = A - 12 K4, semihouse = B - 12 K4, closedhouse = Q, 5path = P - 2 S + 9 T - 4 R.
 * gm_sgl5_raw fills the sums `pattern` needs (one of the six names, or "all") and sets the others to 0; T .. S come from the supports of the
 * oriented copy and one more pass over its triangles (csrc/gm_wtri.hip), K4 and R from gm_clique / gm_sgl("rectangle"), P and Q from one
 * kernel each on the symmetric graph.  stats->kernel_ms covers every kernel of the call, stats->tasks = the graph's directed entries.
 * One GPU, synchronous: world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED (the closed forms are applied on the host), a handle of
 * >= 2^31 entries -> GM_ERR_TOO_LARGE, any other name -> GM_ERR_INVALID.  gm_sgl5_finish is host-only (no device).
 * gm_sgl5_raw_need: the same with the sums named by a bit mask (bit i = raw[i]) instead of a pattern -- A or B without the 4-clique count
 * of a dense graph; need == 0 or bits beyond GM_SGL5_NRAW -> GM_ERR_INVALID. */
#define GM_SGL5_NRAW 11
int gm_sgl5_raw(const gm_graph *sym, const char *pattern, const gm_launch *launch, uint64_t raw[GM_SGL5_NRAW], gm_stats *stats);
int gm_sgl5_raw_need(const gm_graph *sym, uint32_t need, const gm_launch *launch, uint64_t raw[GM_SGL5_NRAW], gm_stats *stats);
int gm_sgl5_finish(const char *pattern, const uint64_t raw[GM_SGL5_NRAW], uint64_t *total);

/* The two 6-vertex patterns of the reference's dispatcher (src/sgl/omp_base.cc:46-50; cpu_kernels/6path.h, dumbbell.h) as closed forms of
 * nine raw sums (DESIGN.md "SgL, 6-vertex closed forms"; e1(v) = sum_{a in N(v)} (d(a) - 1), R_v = 4-cycles through v, the rest as above):
 *   raw[0] X = sum_{u,v} s(u,v) s(v,u) over the undirected edges, s(u,v) = e1(u) - (d(v) - 1) - t(e)     raw[1] Y = sum_v T_v (d(v) - 2)^2
 *   raw[2] Z = sum_v d(v) R_v = sum over the 4-cycles of the degrees of their four vertices               raw[3] R = the rectangle count
 *   raw[4] D = sum_e C(t,2)      raw[5] C5 = the pentagon count      raw[6] M = sum_{u,v} (T_u - t(e)) (T_v - t(e)) over the undirected edges
 *   raw[7] B = sum_tri [x(ab)x(ac) + x(ab)x(bc) + x(ac)x(bc)]         raw[8] K4 = 4-cliques
 *   6path = X - Y - 2 Z + 12 R + 4 D - 5 C5,   dumbbell = M - B + 6 K4.
 * gm_sgl6_need (host-only): bit i of *mask = raw[i] is needed by `pattern` ("6path", "dumbbell", or "all").  gm_sgl6_raw fills the sums of the
 * bit mask `need` and writes the others as 0: Z by a kernel of its own on the copy numbered ascending in degree (csrc/gm_wrect.hip: the
 * rectangle's pruned walk with two counters per 2-path end, in LDS one range of ids at a time; tune[6] & GM_T6_AS_NUMBERED: on the graph as
 * numbered; gm_dev_option("GM_WRECT_RANGE", ..), read when a handle's plan is built: ids per range, at most 4096); R from that kernel when Z
 * is asked too, else from gm_sgl("rectangle"); D, B, K4 as gm_sgl5_raw takes them; X, M, Y from the supports, triangles and degrees the
 * 5-vertex pass leaves on the oriented copy; C5 from gm_sgl("pentagon").  gm_sgl6_finish (host-only) applies a closed form modulo 2^64;
 * gm_sgl6 = need -> raw -> finish.  The contract of gm_sgl5_raw: SYMMETRIC graph, one GPU, synchronous -- world > 1 or launch->d_counts ->
 * GM_ERR_UNSUPPORTED, a handle of >= 2^31 entries -> GM_ERR_TOO_LARGE, an unknown name, need == 0 or bits beyond GM_SGL6_NRAW ->
 * GM_ERR_INVALID, unsorted rows -> GM_ERR_INVALID as in every solver, ne == 0 -> GM_OK with zeros.  stats->kernel_ms covers every kernel of
 * the call, stats->tasks = the graph's directed entries.  The arrays of the diamond, the 5-vertex forms and the local counts stay usable. */
#define GM_SGL6_NRAW 9
int gm_sgl6_need(const char *pattern, uint32_t *mask);
int gm_sgl6_raw(const gm_graph *sym, uint32_t need, const gm_launch *launch, uint64_t raw[GM_SGL6_NRAW], gm_stats *stats);
int gm_sgl6_finish(const char *pattern, const uint64_t raw[GM_SGL6_NRAW], uint64_t *total);
int gm_sgl6(const gm_graph *sym, const char *pattern, const gm_launch *launch, uint64_t *total, gm_stats *stats);

/* Diamond on SEVERAL ranks with the one-GPU algorithm (one shared pass over the triangles of the oriented copy; the reference has no
 * multi-GPU diamond: src/sgl/multigpu.cu:117 is commented out).  Per step, on every rank:
 *   1. gm_diamond_support_partial: the rank's share (launch->rank / world) of the triangle pass adds its three increments per triangle
 *      into d_support -- the caller's DEVICE buffer of n_entries uint32 (AT LEAST gm_diamond_support_size = S: |E+| of the oriented copy
 *      rounded up so that every rank's slice is equal and 256-byte aligned; fewer -> GM_ERR_INVALID; a larger buffer is accepted and only
 *      its first S entries are used), zeroed by the call, ordered on launch->stream;
 *   2. the caller sums the ranks' arrays with ONE reduce-scatter (ncclReduceScatter, ncclUint32, ncclSum / torch reduce_scatter_tensor):
 *      rank r receives the S / world entries from r * S / world on (S = gm_diamond_support_size, not the buffer's own length);
 *   3. gm_diamond_support_finish: sum C(t, 2) over `count` entries at d_support (the rank's reduced slice) -> total / launch->d_counts;
 *   4. the usual all-reduce of the 64-bit count.
 * Rows of the oriented copy beyond the 2048-entry stage take sup_long_kernel (one wave per edge) inside the same call. */
int gm_diamond_support_size(const gm_graph *sym, int world, int64_t *n_entries);
/* Tooling (bench.py's byte model, tests): after a one-GPU gm_sgl(.., "diamond") on this handle -- info[0] = 64-bit words of the match-mask
 * arena (the in-edge tasks of the triangle pass report their streamed edges as bit masks of their tails, gm_sup.hip; 0 = no masks on this
 * graph), info[1] = streamed-edge increments the most recent launch issued as global atomics, info[2] = rows with masks of several words,
 * info[3] = the shortest tail that gets a mask.  Synchronises the device. */
int gm_diamond_support_info(const gm_graph *sym, int64_t info[4]);
/* Tooling: the supports of the edges inside the hub corner (the last H vertices of the renumbered oriented copy) are one bit-matrix product
 * on the matrix cores, t(i, j) = (A A)_ij over the symmetric corner A (csrc/gm_ctc.hip), and the triangle pass leaves the corner's rows
 * out: info[0] = H (0: none), info[1] = DAG entries inside the corner, info[2] = pairs of 256-row blocks, info[3] = 512-column chunks per
 * row.  gm_dev_option("GM_SUP_CORE_H", ..) (read when the handle's task lists are built): 0 = off, a multiple of 512 = that H. */
int gm_sup_core_info(const gm_graph *sym, int64_t info[4]);
/* Tooling (tests): the plan gm_sgl "rectangle" / "house" built for its LDS maps on this handle -- valid after a first such call with the maps
 * in LDS, GM_ERR_INVALID before -- read from the copy that call ran on (the copy numbered ascending in degree, or the handle itself: the
 * house, and the rectangle under GM_T6_AS_NUMBERED).  Read-only.  out[0] = ranges n, [1] = cut (first id of the ranges), [2] = (centre,
 * range) LDS tasks, [3] = one-task (centre, -1) LDS tasks, [4] = tasks in front of the acc list (LDS centres: their ends below the cut),
 * [5] = whole-workgroup acc tasks, [6] = four-centres-to-a-task acc tasks, [7] = whole-workgroup tasks among the front; the rectangle then
 * out[8 .. 8 + n] = the range bounds rb[0 .. n] and out[9 + n .. 9 + 2 n) = log2 of the counter width of every range (3, 4 or 5).
 * n_out below what is written -> GM_ERR_INVALID; 80 is always enough. */
int gm_map_plan_info(const gm_graph *sym, const char *pattern, int64_t *out, int n_out);
int gm_diamond_support_partial(const gm_graph *sym, const gm_launch *launch, uint32_t *d_support, int64_t n_entries, gm_stats *stats);
int gm_diamond_support_finish(const gm_graph *sym, const gm_launch *launch, const uint32_t *d_support, int64_t count, uint64_t *total,
                              gm_stats *stats);

/* ---- local counts and the k-truss (csrc/gm_local.hip; DESIGN.md "Local counts and k-truss") ----------------------------------------
 * What a caller asks of a triangle counter after the total: the triangles at every vertex and the support |N(u) ^ N(v)| of every edge, in
 * the CALLER's numbering and entry order -- and their first consumer, the k-truss.  The supports come from the one pass over the triangles
 * of the oriented copy that the one-GPU diamond takes (every path of it; launch->tune[6] is honoured), into an array of these calls' own:
 * the calls work before or after any other solver on the handle and leave the diamond's and the 5-vertex forms' arrays alone.
 * SYMMETRIC graph, one GPU, synchronous: a null handle -> GM_ERR_INVALID, a handle of >= 2^31 entries -> GM_ERR_TOO_LARGE, world > 1 or
 * launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows -> GM_ERR_INVALID as in every solver, ne == 0 -> GM_OK with zeros.
 * ONE of these calls at a time per handle: the supports, the peeling state and the reverse-entry index live on the handle (as the other
 * solvers' per-handle arrays do); different handles may be used from different threads.
 * stats->kernel_ms covers every kernel of the call (a k-truss: also the host's one read-back per round), stats->tasks = the directed entries.
 *
 * gm_tc_local -- the CALLER's numbering and entry order:
 *   d_vertex_tri: DEVICE uint64[nv] or NULL -- T_v, the triangles at v (half the sum of the supports of row v).
 *   d_entry_sup:  DEVICE uint32[ne] or NULL -- for entry i = (u, v) of row u: |N(u) ^ N(v)|; the two directions of an edge are equal.
 *   total (may be NULL): the triangle count, sum_v T_v / 3. */
int gm_tc_local(const gm_graph *sym, const gm_launch *launch, uint64_t *d_vertex_tri, uint32_t *d_entry_sup, uint64_t *total, gm_stats *stats);

#define GM_TRUSS_REMOVED 0xFFFFFFFFu
/* k-truss, k >= 2 (k < 2 -> GM_ERR_INVALID): the largest edge set in which every edge lies in >= k - 2 triangles OF THAT SET.
 *   d_entry_sup (DEVICE uint32[ne] or NULL): the support of the entry's edge inside the k-truss, GM_TRUSS_REMOVED for an edge outside it
 *   (both directions of every edge are written).  n_edges: undirected edges of the k-truss.  rounds (may be NULL): peeling rounds run.
 * A round marks the alive edges of support < k - 2 as the frontier, counts them (the one word the host reads per round), and one wave per
 * frontier edge takes the edge's triangles from the supports of their surviving edges; the frontier is removed after the round.  The round
 * that finds an empty frontier ends the call and counts: rounds >= 1 on a graph with edges. */
int gm_ktruss(const gm_graph *sym, int k, const gm_launch *launch, uint32_t *d_entry_sup, uint64_t *n_edges, int32_t *rounds, gm_stats *stats);
/* trussness of every edge: tau(e) = the largest k whose k-truss holds e (>= 2).  d_entry_truss: DEVICE uint32[ne] (NULL -> GM_ERR_INVALID).
 * k_max = max tau (0 for a graph without edges).  rounds as above, over all levels: the same rounds with k rising from 3 -- an edge
 * removed while the threshold is k - 2 gets tau = k - 1 -- and from a level whose frontier is empty k goes straight to the smallest alive
 * support + 3, the first level that removes an edge. */
int gm_truss_decompose(const gm_graph *sym, const gm_launch *launch, uint32_t *d_entry_truss, int32_t *k_max, int32_t *rounds, gm_stats *stats);

/* ---- triangle listing (csrc/gm_list.hip; DESIGN.md "Triangle listing") --------------------------------------------------------------
 * Every triangle of a SYMMETRIC graph exactly once, as three ids of the CALLER's numbering, a < b < c, 12 bytes per triangle.
 *   d_tri   DEVICE int32[3 * cap], or NULL (then cap is ignored: count only)
 *   first   index of the first triangle wanted in the handle's listing order;  cap: at most this many are written
 *   total   (may be NULL) T, the number of triangles of the graph -- always the whole count, whatever the window
 *   n_written (may be NULL) min(cap, T - first), 0 when first >= T or d_tri == NULL
 * The listing order is fixed for a handle: calls with windows [0,c), [c,2c), ... write, concatenated, exactly the sequence one call
 * with first = 0, cap >= T writes.  Nothing is written beyond 3 * n_written ints.  The order: ascending entry (u, v) of the handle's
 * oriented copy (gm_graph_orient's), then ascending position of the third vertex in the shorter of N+(u), N+(v) (N+(u) when equal).
 * The first call on a handle counts the matches of every batch of 64 entries and scans them (kept on the handle); every call with a
 * buffer then walks only the batches whose slots meet its window.  The call runs on the oriented copy as numbered -- it keeps the
 * caller's ids -- so launch->tune[6] is ignored, GM_T6_AS_NUMBERED included: there is no renumbered copy to turn off.
 * The contract of the local counts above: one GPU, synchronous; a null handle -> GM_ERR_INVALID, >= 2^31 entries -> GM_ERR_TOO_LARGE,
 * world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows -> GM_ERR_INVALID, ne == 0 -> GM_OK with zeros; launch->stream is
 * honoured; stats->kernel_ms covers every kernel of the call, stats->tasks = the directed entries; before or after any other solver on
 * the handle, whose arrays it leaves alone; ONE such call at a time per handle. */
int gm_tc_list(const gm_graph *sym, const gm_launch *launch, uint64_t first, uint64_t cap, int32_t *d_tri, uint64_t *total,
               uint64_t *n_written, gm_stats *stats);

#define GM_MAX_CLIQUE_K 12
/* CliqueSolver on the DAG, 3 <= k <= GM_MAX_CLIQUE_K (src/clique/cpu_kernels/automine_omp.h:67-83,138-157;
 * src/clique/gpu_kernels/clique4_warp_edge.cuh:3-31 ... clique8; k = 9..12: the same levels once more, as the reference's generic
 * clique_omp_recursive / edge_warp_iterative.cuh:2-75 count them -- its gpu_base.cu:59-71 stops at 8), any out-degree. k = 4: the first DFS level is re-hosted (every
 * edge at the endpoint with the longer out-list, gm_cbuild.hip), rows of up to 2048 entries keep their adjacency bit-matrix in an
 * arena in HBM, longer rows one per workgroup. k >= 5: the deeper levels run on induced sub-matrices; rows of up to 4096 entries sweep
 * them with two words per lane, longer rows out of the workgroup's global scratch (slow, exact; the degree-ordered DAG of com-Orkut has
 * rows of at most 535 entries, of a scale-24 R-MAT graph 1744). The workgroups' scratch slots must fit the device memory, else
 * GM_ERR_TOO_LARGE -- a count is refused, never wrong. TC (k = 3) and k = 4 run on a topologically renumbered copy of a DAG whose
 * rows are long (cached on the handle; tune[6] & GM_T6_AS_NUMBERED: as numbered). */
int gm_clique(const gm_graph *dag, int k, const gm_launch *launch, uint64_t *total, gm_stats *stats);

/* ---- local k-clique counts (csrc/gm_kcl_local.hip; DESIGN.md "Local k-clique counts") ------------------------------------------------
 * What a caller asks of a clique counter after the total: the k-cliques at every vertex and on every edge, in the CALLER's numbering and
 * entry order (the input of a k-clique densest subgraph, a nucleus decomposition, higher-order clustering coefficients).  SYMMETRIC
 * graph, as for the local triangle counts; the call takes the oriented copy from the handle itself.
 *   d_vertex_cnt: DEVICE uint64[nv] or NULL -- K_v, the k-cliques that contain v (the sum of row v of the entry counts / (k - 1)).
 *   d_entry_cnt:  DEVICE uint64[ne] or NULL -- for entry i = (u, v) of row u: K_uv, the k-cliques that contain the edge; the two
 *                 directions of an edge are equal.  Both arrays are 64-bit: an edge of a graph of a few hundred vertices can lie in
 *                 more than 2^32 cliques.
 *   total (may be NULL): the k-clique count, sum_v K_v / k.
 * All arithmetic is integer: the results do not depend on the launch or on the order in which the workgroups arrive.
 * 3 <= k <= 8.  k < 3 or k > GM_MAX_CLIQUE_K -> GM_ERR_INVALID as in the clique solver above; 9 <= k <= GM_MAX_CLIQUE_K ->
 * GM_ERR_UNSUPPORTED for now.  k = 3 gives the supports and triangles of the local triangle counts, widened to 64 bits.
 * Every root u of the DAG builds the symmetric adjacency bit-matrix of its out-list and attributes the cliques it roots with ONE 64-bit
 * atomic per DAG triangle and one per out-edge, nothing per clique.  Out-lists of up to 512 entries keep the matrix in LDS (k >= 5:
 * those beyond 128 entries are shared by several workgroups); longer ones, of any length, take a slot of a global scratch per workgroup
 * (slow, exact; the slots must fit the device memory, else GM_ERR_HIP -- a count is refused, never wrong).
 * By default the call runs on the copy the one-GPU diamond's triangle pass runs on: the oriented copy renumbered topologically when its
 * rows are long (cached on the handle), else the oriented copy as numbered.  launch->tune[6] & GM_T6_AS_NUMBERED: always the oriented
 * copy as numbered, no renumbered copy.  The counts are the same on both.
 * The contract of the local counts above: one GPU, synchronous; a null handle -> GM_ERR_INVALID, >= 2^31 entries -> GM_ERR_TOO_LARGE,
 * world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows -> GM_ERR_INVALID, ne == 0 -> GM_OK with zeros (d_vertex_cnt is
 * zeroed when given); launch->stream is honoured; stats->kernel_ms covers every kernel of the call, stats->tasks = the directed
 * entries; before or after any other solver on the handle, whose arrays it leaves alone; ONE such call at a time per handle; every
 * array it keeps on the handle is freed with the handle. */
int gm_clique_local(const gm_graph *sym, int k, const gm_launch *launch, uint64_t *d_vertex_cnt, uint64_t *d_entry_cnt, uint64_t *total,
                    gm_stats *stats);

/* ---- k-clique listing (csrc/gm_clique_list.hip; DESIGN.md "k-clique listing") ----------------------------------------------------------
 * Every k-clique of a SYMMETRIC graph exactly once, 3 <= k <= 8, as k ids of the CALLER's numbering, strictly ascending, 4 k bytes per row.
 *   d_cliques DEVICE int32[k * cap], or NULL (then cap is ignored: count only)
 *   first     index of the first row wanted in the listing order of (handle, k);  cap: at most this many are written
 *   total     (may be NULL) the k-clique count of the whole graph, whatever the window: gm_clique(k) of the oriented copy
 *   n_written (may be NULL) min(cap, total - first), 0 when first >= total or d_cliques == NULL
 * The listing order is fixed for a (handle, k): calls with windows [0,c), [c,2c), ... write, concatenated, exactly the sequence one call
 * with first = 0, cap >= total writes.  Nothing is written beyond k * n_written ints.  The order: ascending ROOT -- the clique's lowest
 * vertex in the order of gm_graph_orient, by degree and then by id -- and within a root lexicographic on the other k - 1 members taken as
 * their ascending positions in N+(root) of the oriented copy as numbered (which are ascending ids).  At k = 3 the SET of rows is
 * gm_tc_list's, the order is not.
 * The first call of a k on a handle counts, per entry (root, L[i]) of the oriented copy, the cliques whose lowest out-list position is i,
 * and scans the counts (kept on the handle per k); every call with a buffer then walks only the roots, entries and pairs whose slots meet
 * its window.  The call runs on the oriented copy as numbered -- it keeps the caller's ids -- so launch->tune[6] is ignored.  Rows of any
 * length are exact: those beyond 512 entries take a scratch slot per workgroup (sized by the longest row; a slot that does not fit the
 * device refuses the call).
 * The contract of the local counts and of gm_tc_list: one GPU, synchronous; a null handle -> GM_ERR_INVALID, >= 2^31 entries ->
 * GM_ERR_TOO_LARGE, world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows -> GM_ERR_INVALID, k < 3 or k > GM_MAX_CLIQUE_K ->
 * GM_ERR_INVALID, 9 <= k <= GM_MAX_CLIQUE_K -> GM_ERR_UNSUPPORTED, ne == 0 -> GM_OK with zeros; launch->stream is honoured;
 * stats->kernel_ms covers every kernel of the call; before or after any other solver on the handle, whose arrays it leaves alone; ONE
 * such call at a time per handle; what it keeps on the handle is freed with the handle. */
int gm_clique_list(const gm_graph *sym, int k, const gm_launch *launch, uint64_t first, uint64_t cap, int32_t *d_cliques, uint64_t *total,
                   uint64_t *n_written, gm_stats *stats);

/* ---- k-clique cores (csrc/gm_kcl_core.hip; DESIGN.md "k-clique cores") ------------------------------------------------------------------
 * The first consumer of the local k-clique counts: the (1,k)-nuclei.  SYMMETRIC graph with ascending rows and no self loops, 2 <= k <= 8.
 * K_v(H) = the k-cliques of the vertex-induced subgraph H that contain v (k = 2: the degree).
 *   The (k, c)-core is the largest vertex set H with K_v(H) >= c for every v of H (k = 2: the ordinary c-core).
 *   The core number kappa_k(v) is the largest c whose (k, c)-core holds v; it does not depend on the peeling order.
 *   The densest prefix: the rounds of the decomposition define nested vertex sets; the one with the most k-cliques per vertex is returned.
 *   The c_max-core is one of them and holds at least 1/k of the optimum k-clique density (Tsourakakis 2015): a 1/k-approximation of the
 *   k-clique densest subgraph.
 * Rounds, the k-truss's scheme with vertices in place of edges: a round's frontier is every alive vertex whose count is below the
 * threshold; the host reads back 24 bytes -- the frontier's size, the smallest count that stays alive, the cliques destroyed so far --,
 * the peel kernel runs, and the frontier becomes removed when the next round marks.  The round that finds an empty frontier ends the level
 * and is counted.  Decomposition: the level starts at the smallest count of the graph, the threshold is level + 1, a vertex that enters
 * the frontier gets kappa = level and round = the 1-based index of that round, from an empty frontier the level goes to the smallest alive
 * count; the call ends with the empty frontier that leaves nothing alive.
 * The rule of the decrements: a k-clique counts only if none of its members was removed before the round began.  Such a clique with at
 * least one frontier member is destroyed in this round: accounted once, by its frontier member of the smallest id, and every member
 * outside the frontier loses one (the counts of frontier members are not maintained).  So frontier vertex v works on S_v = the members of
 * N(v) that are not removed, without the frontier vertices of an id below v: it subtracts the (k-1)-cliques of G[S_v] that hold w from
 * every w of S_v outside the frontier, and adds their sum / (k - 1) to the destroyed total: one 64-bit atomic per member of S_v and one per
 * frontier vertex, nothing per clique.  The path follows |S_v|: up to 64 survivors a wave, up to 512 a workgroup with the matrix in LDS,
 * beyond that a scratch slot per workgroup (sized by the longest row; a slot that does not fit the device refuses the call).
 *
 * gm_clique_kcore: n_vertices / n_cliques (may be NULL) = the vertices and the k-cliques of the (k, c)-core (the graph's total minus the
 *   destroyed; the call checks it against sum K_v / k over the core), rounds (may be NULL) = the rounds run (>= 1).  c = 0 removes nothing.
 * gm_clique_core_decompose: c_max = max kappa, rounds over all levels; dense (may be NULL): the state at the start of round r is the set
 *   {v : round[v] >= r} -- round 1 is the whole graph --; of the states with a vertex the one with the largest cliques / vertices (exact:
 *   cross products in 128 bits; a tie goes to the earliest round) as (round, vertices, cliques).  Isolated vertices: kappa 0, round 1.
 * The contract of gm_clique_local: one GPU, synchronous; a null handle -> GM_ERR_INVALID, k < 2 or k > GM_MAX_CLIQUE_K -> GM_ERR_INVALID,
 * 9 <= k <= GM_MAX_CLIQUE_K -> GM_ERR_UNSUPPORTED, >= 2^31 entries -> GM_ERR_TOO_LARGE, world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED,
 * unsorted rows -> GM_ERR_INVALID; ne == 0 -> GM_OK, every vertex kappa 0 and round 1, the arrays written when given; launch->stream is
 * honoured; launch->tune[6] & GM_T6_AS_NUMBERED is passed on to the initial count (gm_clique_local on the same handle; k = 2: the row
 * lengths) and to nothing else; stats->kernel_ms covers every kernel and the per-round read-backs, stats->tasks = the directed entries;
 * before or after any other solver on the handle, whose arrays it leaves alone; state is initialised per call; ONE such call at a time per
 * handle; everything it keeps on the handle is freed with the handle. */
#define GM_CORE_REMOVED 0xFFFFFFFFFFFFFFFFull
typedef struct gm_core_dense { int32_t round; uint64_t vertices, cliques; } gm_core_dense;
int gm_clique_kcore(const gm_graph *sym, int k, uint64_t c, const gm_launch *launch,
                    uint64_t *d_vertex_cnt,     /* DEVICE uint64[nv] or NULL: K_v inside the (k,c)-core, GM_CORE_REMOVED outside it */
                    uint64_t *n_vertices, uint64_t *n_cliques, int32_t *rounds, gm_stats *stats);
int gm_clique_core_decompose(const gm_graph *sym, int k, const gm_launch *launch,
                    uint64_t *d_vertex_core,    /* DEVICE uint64[nv], NULL -> GM_ERR_INVALID: kappa_k(v) */
                    uint32_t *d_vertex_round,   /* DEVICE uint32[nv] or NULL: the round whose frontier held v (>= 1) */
                    uint64_t *c_max, int32_t *rounds, gm_core_dense *dense /* may be NULL */, gm_stats *stats);

/* ---- k-clique trusses (csrc/gm_kcl_truss.hip; DESIGN.md "k-clique trusses") ---------------------------------------------------------------
 * The consumer of the per-edge k-clique counts: the (2,k)-nuclei.  SYMMETRIC graph with ascending rows and no self loops, 3 <= k <= 8.
 * K_e(H) = the k-cliques, all of whose edges lie in the edge set H, that contain e.
 *   The (k, c)-truss is the largest edge set H with K_e(H) >= c for every e of H (k = 3: the ordinary (c + 2)-truss).
 *   The clique trussness theta_k(e) is the largest c whose (k, c)-truss holds e; it does not depend on the peeling order, and
 *   theta_3(e) = trussness(e) - 2.
 * The calls return numbers per edge, not the connected components of a nucleus nor a hierarchy of them.
 * Rounds, the cores' scheme with edges in place of vertices; the state of an undirected edge sits at its canonical entry min(e, rev[e]): a
 * round's frontier is every alive edge whose count is below the threshold; the host reads back 24 bytes -- the cliques destroyed so far, the
 * frontier's size, the smallest count that stays alive --, the peel kernel runs, and the frontier becomes removed when the next round marks.
 * The round that finds an empty frontier ends the level and is counted.  Decomposition: the level starts at the smallest count of the
 * graph, the threshold is level + 1, an edge that enters the frontier gets theta = level and round = the 1-based index of that round, from
 * an empty frontier the level goes to the smallest alive count; the call ends with the empty frontier that leaves nothing alive.
 * The rule of the decrements: a k-clique counts only if none of its edges was removed before the round began.  Such a clique with at least
 * one frontier edge is destroyed in this round: accounted once, by its frontier edge of the smallest canonical entry, and every edge of it
 * outside the frontier loses one (the counts of frontier edges are not maintained).  Call an edge blocked for frontier edge e = (u, v) if
 * it is removed, or in the frontier with a canonical entry below e's.  e works on S_e = the common neighbours w of u and v with neither
 * (u, w) nor (v, w) blocked, and on the graph on S_e of the edges (w, x) that are not blocked: with c_i = the (k-2)-cliques of that graph
 * that hold w_i it subtracts c_i from (u, w_i) and from (v, w_i), with c_ij = those that hold w_i and w_j (k >= 4) it subtracts c_ij from
 * (w_i, w_j) -- each only outside the frontier -- and adds sum_i c_i / (k - 2) to the destroyed total: two 64-bit atomics per member of
 * S_e, one per adjacent pair of members and one per frontier edge, nothing per clique.  The path follows |S_e|: up to 64 survivors a wave,
 * up to 512 a workgroup with the matrix in LDS, beyond that a scratch slot per workgroup (sized by the longest row; a slot that does not
 * fit the device refuses the call).  k = 3 runs through the same kernels with empty pair terms.
 *
 * gm_clique_ktruss: n_edges / n_cliques (may be NULL) = the undirected edges and the k-cliques of the (k, c)-truss (the graph's total minus
 *   the destroyed; the call checks it against sum K_e / C(k, 2) over the truss), rounds (may be NULL) = the rounds run (>= 1).  c = 0
 *   removes nothing.
 * gm_clique_truss_decompose: c_max = max theta, rounds over all levels; the call checks that the rounds destroyed every clique.  An entry
 *   that is not an edge (a self loop): theta 0, round 0, GM_CORE_REMOVED.
 * The contract of the cores: one GPU, synchronous; a null handle -> GM_ERR_INVALID, k < 3 or k > GM_MAX_CLIQUE_K -> GM_ERR_INVALID,
 * 9 <= k <= GM_MAX_CLIQUE_K -> GM_ERR_UNSUPPORTED, >= 2^31 entries -> GM_ERR_TOO_LARGE, world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED,
 * unsorted rows or an oriented copy (gm_graph_orient) -> GM_ERR_INVALID; ne == 0 -> GM_OK, zeros, rounds = 1; launch->stream is honoured; launch->tune[6] & GM_T6_AS_NUMBERED is
 * passed on to the initial count (gm_clique_local on the same handle, entry counts only) and to nothing else; stats->kernel_ms covers every
 * kernel and the per-round read-backs, stats->tasks = the directed entries; before or after any other solver on the handle, whose arrays
 * it leaves alone; state is initialised per call; ONE such call at a time per handle; everything it keeps on the handle is freed with the
 * handle. */
int gm_clique_ktruss(const gm_graph *sym, int k, uint64_t c, const gm_launch *launch,
                     uint64_t *d_entry_cnt,   /* DEVICE uint64[ne] or NULL: K_e inside the (k,c)-truss, GM_CORE_REMOVED outside it; both directions of an edge equal */
                     uint64_t *n_edges, uint64_t *n_cliques, int32_t *rounds, gm_stats *stats);
int gm_clique_truss_decompose(const gm_graph *sym, int k, const gm_launch *launch,
                     uint64_t *d_entry_theta, /* DEVICE uint64[ne], NULL -> GM_ERR_INVALID: theta_k of the entry's edge, both directions */
                     uint32_t *d_entry_round, /* DEVICE uint32[ne] or NULL: the 1-based round whose frontier held the edge */
                     uint64_t *c_max, int32_t *rounds, gm_stats *stats);

/* ---- triangle nuclei (csrc/gm_nucleus34.hip; DESIGN.md "Triangle nuclei") ---------------------------------------------------------------
 * The third member of the nucleus line (Sariyuce et al.): triangles as the peeled unit, 4-cliques as what holds them together -- the
 * (3,4)-nuclei.  SYMMETRIC graph with ascending rows.  Every per-triangle array is indexed by the triangle's ID = its row in gm_tc_list's
 * listing on the same handle (ascending entry (u, v) of the oriented copy, then ascending third vertex): a caller lines values up with
 * gm_tc_list rows, window by window.  n_tri is the length the caller allocated and must equal T, the total of a count-only gm_tc_list
 * (else GM_ERR_INVALID); T >= 2^32 - 1 -> GM_ERR_TOO_LARGE.
 * K4(t) = the 4-cliques that contain triangle t = |N(a) & N(b) & N(c)| of its corners, at most nv - 3.  For a triangle set H, K4_t(H) = the
 * 4-cliques containing t all four of whose triangles lie in H; the (3,4)-c-nucleus set is the largest H with K4_t(H) >= c for every t of H,
 * theta(t) the largest c whose set holds t.  The calls return numbers per triangle, not connected components nor a hierarchy.
 * Rounds, the k-clique trusses' scheme with triangles in place of edges: a round's frontier is every alive triangle whose count is below
 * the threshold; the host reads back 24 bytes -- the cliques destroyed so far, the frontier's size, the smallest count that stays alive --,
 * the peel kernel runs, and the frontier becomes removed when the next round marks.  The round that finds an empty frontier is counted.
 * Decomposition: the level starts at the smallest count, the threshold is level + 1, a triangle that enters the frontier gets theta = level
 * and round = the 1-based index of that round, from an empty frontier the level goes to the smallest alive count; the call ends with the
 * empty frontier that leaves nothing alive.
 * The rule of the decrements: a 4-clique counts only if none of its four triangles was removed before the round began.  Such a clique with
 * at least one frontier triangle is destroyed in this round: accounted once, by its frontier triangle of the smallest id, and every
 * triangle of it outside the frontier loses one (the counts of frontier triangles are not maintained).  Frontier triangle t = (a, b, c)
 * takes every common neighbour x of its corners, looks up the ids of (a, b, x), (a, c, x), (b, c, x), skips x if one of them is removed or
 * in the frontier below t's id, and otherwise adds one to the destroyed total and subtracts one from each of the three outside the
 * frontier: three 32-bit atomics per destroyed clique at most.  The marks do not change while a peel kernel runs: the result does not
 * depend on the order of arrival.
 *
 * gm_tri_clique4_local: d_tri_cnt (DEVICE uint32[n_tri] or NULL) = K4(t); total_k4 (may be NULL) = sum K4(t) / 4 = the 4-cliques of the
 *   graph (the call checks that the division is exact).
 * gm_nucleus34: n_triangles / n_cliques (may be NULL) = the triangles and the 4-cliques of the c-nucleus set (the graph's total minus the
 *   destroyed; the call checks it against sum of the surviving counts / 4), rounds (may be NULL) = the rounds run (>= 1).  c = 0 removes
 *   nothing.
 * gm_nucleus34_decompose: c_max = max theta, rounds over all levels; the call checks that the rounds destroyed every 4-clique.
 * The contract of the k-clique trusses: one GPU, synchronous; a null handle -> GM_ERR_INVALID, >= 2^31 entries -> GM_ERR_TOO_LARGE,
 * world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows or an oriented copy (gm_graph_orient) -> GM_ERR_INVALID; T == 0 ->
 * GM_OK, zeros, rounds = 1; launch->stream is honoured, launch->tune[6] is ignored; stats->kernel_ms covers every kernel and the per-round
 * read-backs (a handle's first call also builds the triangle index), stats->tasks = T; before or after any other solver on the handle,
 * whose arrays it leaves alone; state is initialised per call; ONE such call at a time per handle; the index (8 bytes per entry of the
 * oriented copy + 8 per triangle) and the state (9 bytes per triangle) stay on the handle and are freed with it. */
int gm_tri_clique4_local(const gm_graph *sym, const gm_launch *launch, uint64_t n_tri,
                     uint32_t *d_tri_cnt,     /* DEVICE uint32[n_tri] or NULL: K4(t) */
                     uint64_t *total_k4, gm_stats *stats);
int gm_nucleus34(const gm_graph *sym, uint32_t c, const gm_launch *launch, uint64_t n_tri,
                     uint32_t *d_tri_cnt,     /* DEVICE uint32[n_tri] or NULL: K4_t inside the c-nucleus set, GM_TRUSS_REMOVED outside it */
                     uint64_t *n_triangles, uint64_t *n_cliques, int32_t *rounds, gm_stats *stats);
int gm_nucleus34_decompose(const gm_graph *sym, const gm_launch *launch, uint64_t n_tri,
                     uint32_t *d_tri_theta,   /* DEVICE uint32[n_tri], NULL -> GM_ERR_INVALID: theta of the triangle */
                     uint32_t *d_tri_round,   /* DEVICE uint32[n_tri] or NULL: the 1-based round whose frontier held the triangle */
                     uint32_t *c_max, int32_t *rounds, gm_stats *stats);

/* ---- local 4-cycle counts (csrc/gm_rect_local.hip; DESIGN.md "Local 4-cycle counts") --------------------------------------------------
 * The 4-cycles (edge-induced, as the `rectangle` of gm_sgl counts them: src/sgl/cpu_kernels/rectangle.h) at every vertex and on every
 * edge, in the CALLER's numbering and entry order: the input of square clustering coefficients, of butterfly supports on bipartite data,
 * of the 4-vertex orbit counts.  SYMMETRIC graph with ascending rows, as for the local triangle counts.
 *   d_vertex_cnt: DEVICE uint64[nv] or NULL -- R_v, the 4-cycles that contain v (half the sum of row v of the entry counts: a 4-cycle
 *                 at v uses two of v's entries).
 *   d_entry_cnt:  DEVICE uint64[ne] or NULL -- for entry i = (u, v) of row u: R_uv, the 4-cycles that contain the edge; the two
 *                 directions of an edge are equal.
 *   total (may be NULL): the 4-cycle count, sum of the entries / 8 = sum_v R_v / 4; equal to gm_sgl("rectangle").
 * All arithmetic is uint64 modulo 2^64 and integer: the results do not depend on the launch or on the order in which the workgroups arrive.
 * The kernel makes the pruned walk of the 6-vertex closed forms' 4-cycle kernel twice per centre and range of ids -- count the 2-paths of
 * every end in LDS, then credit every 2-path edge -- with one 64-bit atomic per 2-path whose end has at least two, and one per spoke.
 * By default the call runs on the copy numbered ascending in degree (cached on the handle, the copy gm_sgl6_raw's Z runs on).
 * launch->tune[6] & GM_T6_AS_NUMBERED: on the graph as given.  The counts are the same on both.  gm_dev_option("GM_RECT_LOCAL_RANGE", ..),
 * read when a graph's plan is built: ids per LDS range, 16 up to the default (gm_constant "rect_local_range").
 * The contract of the local counts above: one GPU, synchronous; a null handle -> GM_ERR_INVALID, >= 2^31 entries -> GM_ERR_TOO_LARGE,
 * world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows -> GM_ERR_INVALID, ne == 0 -> GM_OK with zeros (d_vertex_cnt is
 * zeroed when given); launch->stream is honoured; stats->kernel_ms covers every kernel of the call, stats->tasks = the directed
 * entries, stats->chunks = the (centre, range) tasks; before or after any other solver on the handle, whose arrays it leaves alone; ONE
 * such call at a time per handle; every array it keeps on the handle is freed with the handle. */
int gm_rect_local(const gm_graph *sym, const gm_launch *launch, uint64_t *d_vertex_cnt, uint64_t *d_entry_cnt, uint64_t *total,
                  gm_stats *stats);

/* ---- local motif counts (csrc/gm_orbit_local.hip, csrc/gm_orbit.h; DESIGN.md "Local motif counts") ----------------------------------------
 * The per-vertex form of the 3- and 4-motif: the graphlet degree vector, the vertex-induced orbit counts of every vertex in Przulj's /
 * ORCA's numbering (the input of network alignment, role features, higher-order clustering).  SYMMETRIC graph with ascending rows, as for
 * the local triangle counts.
 *   k = 3: orbits 0 .. 3 (n_orbits = 4), counts[2];  k = 4: orbits 0 .. 14 (n_orbits = 15), counts[6].
 *   d_orbits: DEVICE uint64[n_orbits * nv] or NULL -- orbit-major in the CALLER's numbering: orbit o of vertex v at d_orbits[o * nv + v].
 *     0 edge (the degree)          1 2-path, end              2 2-path, middle            3 triangle
 *     4 4-path, end                5 4-path, inner            6 3-star, leaf              7 3-star, centre
 *     8 4-cycle                    9 tailed triangle, the tail's end (degree 1)           10 tailed triangle, a triangle vertex of degree 2
 *     11 tailed triangle, the vertex carrying the tail        12 diamond, degree-2 vertex 13 diamond, degree-3 (chord) vertex
 *     14 4-clique
 *   counts (may be NULL; else ncounts must be 2 for k = 3, 6 for k = 4 -> GM_ERR_INVALID): exactly what gm_motif(k) returns, in its order,
 *     here from the column sums: k = 3 [sum o2, sum o3 / 3]; k = 4 [sum o7, sum o4 / 2, sum o9, sum o8 / 4, sum o13 / 2, sum o14 / 4] =
 *     [3-star, 4-path, tailed triangle, 4-cycle, diamond, 4-clique].
 * All arithmetic is uint64 modulo 2^64 and integer: the results do not depend on the launch or on the order in which the workgroups arrive.
 * The call obtains t(e) and T_v, R_v and K_v through gm_tc_local, gm_rect_local and gm_clique_local(4) on the same handle, adds one pass
 * over the triangles that credits every diamond to its rim edges (two 64-bit atomics per triangle and one per task), gathers the neighbour
 * sums per vertex and turns the non-induced counts into induced orbits (gm_orbit.h).  k = 3 runs the support pass and one gather only: no
 * rectangle plan is built, no k-clique kernel runs.  launch->tune[6] & GM_T6_AS_NUMBERED is passed on to the three input calls and the
 * new pass (the oriented copy and the graph as numbered, no renumbered copies).  The counts are the same either way.
 * The contract of the local counts above: one GPU, synchronous; a null handle or k not in {3, 4} -> GM_ERR_INVALID, >= 2^31 entries ->
 * GM_ERR_TOO_LARGE, world > 1 or launch->d_counts -> GM_ERR_UNSUPPORTED, unsorted rows -> GM_ERR_INVALID, ne == 0 -> GM_OK with zeros
 * (d_orbits is zeroed when given); launch->stream is honoured; stats->kernel_ms covers every kernel of the call, the three input
 * computations included, stats->tasks = the directed entries; before or after any other solver on the handle, whose arrays it leaves
 * alone; ONE such call at a time per handle; every array it keeps on the handle is freed with the handle. */
int gm_motif_local(const gm_graph *sym, int k, const gm_launch *launch, uint64_t *d_orbits, uint64_t *counts, int ncounts, gm_stats *stats);

/* MotifSolver on the SYMMETRIC graph. k = 3: counts[0] = wedges, counts[1] = triangles
 * (the CPU order, src/motif/cpu_kernels/automine_base.h:13,18; NOT the swapped order of
 * src/motif/gpu_kernels/motif3_edge_warp.cuh:19-22). ncounts must be
 * num_possible_patterns[k] (include/pattern.hh:4-15): 2 for k = 3, 6 for k = 4 (see gm_motif4_partial).
 * k = 3 takes the reference's formula solver by default (gm_motif_formula below: the triangles of the oriented copy, wedges derived);
 * tune[6] & GM_T6_PER_EDGE: automine_3motif's enumeration, one bounded intersection of the two symmetric lists per edge. Same counts;
 * stats->tasks = the graph's directed entries either way.
 * With world > 1 a rank's wedge value is a partial modulo 2^64 (formula: rank 0 contributes sum C(d,2); enumeration: one intersection
 * per undirected edge serves both directed edges, which may belong to different ranks); the uint64 sum over ranks is the exact count. */
int gm_motif(const gm_graph *sym, int k, const gm_launch *launch, uint64_t *counts, int ncounts, gm_stats *stats);

/* 4-motif in the reference's formula form (src/motif/cpu_kernels/automine_formula.h:21-56, host fix-up
 * src/motif/omp_formula.cc:41-45). gm_motif(k = 4, ncounts = 6) returns [3-star, 4-path, tailed-triangle, 4-cycle,
 * diamond, 4-clique] (vertex-induced, the order of src/motif/README.md:50-60) on one GPU. Multi-GPU: every rank calls
 * gm_motif4_partial (raw[6] are plain sums over its tasks), the ranks all-reduce raw, then gm_motif4_finish.
 * Asynchronous form: with launch->d_counts set, gm_motif4_partial leaves raw[0..5] in that device buffer without
 * synchronising (raw may then be NULL) -- all-reduce it in place, copy it back, call gm_motif4_finish. gm_motif(k = 4)
 * accepts counts == NULL with d_counts set like every other solver (the fix-up then runs on the device). */
int gm_motif4_partial(const gm_graph *sym, const gm_launch *launch, uint64_t raw[6], gm_stats *stats);
int gm_motif4_finish(const uint64_t raw[6], uint64_t counts[6]);

/* motif_omp_formula / motif_gpu_formula (src/motif/omp_formula.cc:39-46, src/motif/gpu_formula.cu:86-92): same
 * counts as gm_motif(k = 3), obtained by enumerating only the triangles (TC kernel on the oriented graph, built once
 * per handle) and deriving wedges = sum_v C(d(v),2) - 3T. */
int gm_motif_formula(const gm_graph *sym, int k, const gm_launch *launch, uint64_t *counts, int ncounts, gm_stats *stats);

/* ---- set-operation primitives (batch form) -------------------------------------------------- */
/* The wave64 equivalents of include/set_intersect.cuh / set_difference.cuh, exposed so the
 * per-primitive parity tests can drive them directly. One wave per pair of ascending int32 lists.
 * All pointers are DEVICE pointers. */
enum {
  GM_OP_INTERSECT_NUM = 0,       /* |A ^ B|                                  set_intersect.cuh:352  */
  GM_OP_INTERSECT_NUM_UPPER = 1, /* |{x in A ^ B : x < upper_i}|              set_intersect.cuh:392  */
  GM_OP_INTERSECT_SET = 2,       /* A ^ B -> out (ascending)                  set_intersect.cuh:73   */
  GM_OP_DIFFERENCE_NUM = 3,      /* |{x in A : x not in B}|                   set_difference.cuh:20  */
  GM_OP_DIFFERENCE_NUM_UPPER = 4,/* |{x in A : x < upper_i, x not in B}|      set_difference.cuh:62  */
  GM_OP_DIFFERENCE_SET = 5,      /* A \ B -> out (ascending)                  set_difference.cuh:112 */
  GM_OP_INTERSECT_SET_UPPER = 6, /* {x in A ^ B : x < upper_i} -> out         set_intersect.cuh:152  */
  GM_OP_DIFFERENCE_SET_UPPER = 7,/* {x in A \ B : x < upper_i} -> out         set_difference.cuh:171 */
  GM_OP_COUNT_SMALLER = 8        /* |{x in A : x < upper_i}| (B unused)       operations.cuh:61-105  */
};
/* Pair i is A_i = values[a_begin[i] .. a_end[i]), B_i = values[b_begin[i] .. b_end[i]).
 * out_num: npairs uint32 (count, or size of the materialised set). For *_SET ops the result of pair
 * i is written at out_values[a_begin[i] ..) (capacity |A_i|; may be NULL for count-only ops).
 * d_upper may be NULL for ops without a bound. d_skip (may be NULL) is the CPU-oracle "other.vid"
 * exclusion of the difference ops (src/common/VertexSet.cc:29,37): elements equal to skip[i] are dropped. */
int gm_setop_batch(int op, int64_t npairs, const int32_t *d_values, const int64_t *d_a_begin, const int64_t *d_a_end,
                   const int64_t *d_b_begin, const int64_t *d_b_end, const int32_t *d_upper, const int32_t *d_skip,
                   uint32_t *d_out_num, int32_t *d_out_values, void *stream);

/* ---- tooling ------------------------------------------------------------------------------- */
/* Deterministic R-MAT edge generator: edge i of 2^scale*edge_factor,
 * quadrant probabilities (0.57, 0.19, 0.19, 0.05), SplitMix64 counter hash of (seed, i, level).
 * Writes 2 keys per edge (src<<32|dst and dst<<32|src) to DEVICE buffer d_keys[2*n_edges];
 * self-loops are written as the sentinel 0xFFFFFFFFFFFFFFFF. */
int gm_rmat_keys(int scale, int64_t n_edges, uint64_t seed, uint64_t *d_keys, void *stream);

/* Tooling: level-2 part of the ALGORITHMIC bytes of one 4-clique launch on `dag`:
 * sum_e [8|S1| + sum_{v2 in S1}(4(|S1| + d+(v2)) + 16)]; the level-1 part is the TC formula. Runs one statistics
 * kernel (per-edge |S1| and the out-degrees of the matched vertices). */
int gm_clique4_level2_bytes(const gm_graph *dag, uint64_t *bytes);

/* Tooling (bench.py's byte model): after a whole-graph gm_clique(dag, 4) -- the blocked gather of the wide vertices' core rows
 * (csrc/gm_cgather.hip): info[0] = (vertex, block of core rows) units, info[1] = the bytes they read by construction (a 16-byte record, 4 B per
 * row, the 16-bit column table from the unit's first row on), info[2] = work items, info[3] = blocks of the core.  All 0: the row-major gather. */
int gm_clique4_gather_info(const gm_graph *dag, int64_t info[4]);

/* Tooling (tests): after a whole-graph gm_clique(dag, 4) -- what the plan of that call holds, on the copy it ran on: the handle itself
 * (as_numbered != 0: a call under GM_T6_AS_NUMBERED; a DAG numbered topologically), else its topological copy.  Read-only, no device pass;
 * GM_ERR_INVALID: no such call yet, or n_out < 13.  out[0] = the copy is topological, [1] = LDS stage of the build kernel, [2] = first vertex
 * of the core bitmap (-1: no core), [3] = rounds, [4] = wide vertices, [5 .. 7] = ... per matrix-core class 0 / 1 / 2, [8] = build tasks,
 * [9] = gather units, [10] = gather items, [11] / [12] = chunks / entries of the rows beyond "cb_max_deg", left to the mining kernel's arena
 * path (-1 / -1: that launch built no table). */
int gm_clique_plan_info(const gm_graph *dag, int as_numbered, int64_t *out, int n_out);

/* PMC calibration (tooling): one pass of dword-per-lane coalesced loads over d_buf[0..n), sum -> *d_out.
 * Exactly 4n bytes are read once; run under `rocprofv3 --pmc FETCH_SIZE` to get the counter scale for the
 * access width the mining kernels use (MI355X_MICROARCH.md: FETCH_SIZE is calibrated only for 16 B/lane). */
int gm_calib_stream(const int32_t *d_buf, int64_t n, uint64_t *d_out, void *stream);

/* Measured stream ceiling (tooling): one pass of 16-byte-per-lane loads over d_buf[0..n) (n int32 words, 16-byte aligned),
 * xor-sum -> *d_out. Time it with events: bytes / t is the read bandwidth a plain stream reaches on this part (the MEASURED
 * ceiling bench.py prints beside the 8 TB/s spec). */
int gm_stream_ceiling(const int32_t *d_buf, int64_t n, uint64_t *d_out, void *stream);

/* Issue-rate calibration (tooling): `waves_per_simd` (1..8) waves on every SIMD of every CU each execute iters x 64 instructions of
 * one kind (0 v_add_u32, 1 v_mul_lo_u32, 2 v_mul_u32_u24, 3 v_cmp -> SGPR pair, 4 v_add_u32 DPP row_shr, 5 s_add_u32, 6 ds_read_b128,
 * 7 ds_read_b32, 8 ds_read_b32 with 32-way bank conflicts, 9 v_add + s_add interleaved, 10 v_readlane, 11 v_mbcnt, 12 v_bcnt,
 * 13 v_cmp SDWA, 14 ds_write_b32, 15 v_cndmask) between two s_memtime reads. Outputs: shader cycles per wave-instruction as one wave
 * sees it (median over the waves) and wave-instructions per cycle and SIMD. The basis of every "unit X is N % busy" statement in
 * DESIGN.md (scripts/issue_calibration.py -> profiles/r03/issue_calibration.txt). Uses the null stream of the current device. */
int gm_issue_calib(int kind, int waves_per_simd, int iters, double *cycles_per_wave_inst, double *inst_per_cycle_simd, double *ms,
                   double *residency /* measured: waves of the launch in flight per SIMD at the same time (mean over SIMDs of the maximum) */);

/* Tooling: a kernel constant by name ("tct_stage_max", "topo_min_mean_row", "motif_trim_min_list", "cb_min_deg", "cb_max_deg",
 * "long_list", "stage_cap", "default_chunk", "mma_words_small", "mma_words_big", "wide_max_deg", "bit_words") -- what the byte model
 * of bench.py needs to know about the kernels, read from the headers they are compiled with -- and the sizes at which the map kernels of
 * the rectangle / the house change path, for the tests that place graphs on both sides: "map_rect_block" (ids of a block of 32-bit
 * counters), "map_one_task_rows", "map_long_row", "map_tile_group", "map_mark_window", "map_house_ids", "map_house_wg_row",
 * "map_house_wg_queue", "map_heavy_centre", "map_house_fw16_rows", "map_lds_min_default", "map_house_walk_min_default"; "chouse_lds_keys": the
 * keys of the shorter list up to which closedhouse keeps an edge's common neighbours in LDS.  GM_ERR_INVALID for an unknown name. */
int gm_constant(const char *name, int64_t *value);

/* Developer / test options (tooling).  The library reads NO algorithm switch from the environment; the named switches that tests and A/B
 * runs need -- forcing a path on a small graph, the documented fallbacks (csrc/gm_mine.h lists them) -- are set here, process-wide:
 * value = NULL removes `name`, name = NULL removes every option.  Options that shape a handle's cached tables are read when those tables
 * are built (use a fresh handle after changing one).  gm_dev_option_get: the current value or NULL.  Nothing in a production caller
 * needs either. */
int gm_dev_option(const char *name, const char *value);
const char *gm_dev_option_get(const char *name);

/* Tooling: the number of device blocks the library has allocated and not yet got back, over all devices and handles of the process.  A block
 * that a freed handle left in the per-device cache of large blocks counts as returned.  Equal before creating a handle and after freeing it
 * (whatever ran in between), or the handle leaked. */
int gm_dev_live_blocks(int64_t *n);

/* wave-primitive self test (DPP scans, ballot rank, LDS search); returns GM_OK when the device
 * results equal the host expectation. *n_fail receives the number of mismatching lanes. */
int gm_selftest(int device, int *n_fail);

#ifdef __cplusplus
}
#endif
#endif
