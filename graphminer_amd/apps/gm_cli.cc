// gm_cli.cc -- one source for the whole command-line surface of the HIP solvers.
//
// Built with -DGM_APP=<TC|SGL|CLIQUE|MOTIF|TRUSS|SGL6|TCLIST|CLIQUELOCAL|RECTLOCAL|MOTIFLOCAL|CLIQUELIST|CLIQUECORE|CLIQUETRUSS|NUCLEUS34> (+ -DGM_APP_MULTIGPU, + -DGM_KCL_SPELLING) into
//   tc_gpu_base tc_multigpu tc_multigpu_base | sgl_gpu_base sgl_multigpu | clique_gpu_base clique_multigpu kcl_gpu_base |
//   motif_gpu_base motif_multigpu | truss_gpu_base | sgl6_gpu_base | tclist_gpu_base | cliquelocal_gpu_base | rectlocal_gpu_base | motiflocal_gpu_base |
//   cliquelist_gpu_base | cliquecore_gpu_base | cliquetruss_gpu_base | nucleus34_gpu_base
// The observable behaviour -- positional argv, defaults, usage text, banner and FINAL result lines -- is that of the
// reference mains (src/triangle/main.cc:7-27, src/sgl/main.cc:9-35, src/clique/main.cc:8-28, src/motif/main.cc:9-31,
// Pangolin spelling src/pangolin/clique/main.cc:20); scripts that grep those lines keep working.  truss_gpu_base <graph prefix> [k] has no
// counterpart there: the same loader, argv checks and exit codes, last line `ktruss_edges = N` (with k) or `max_truss = K` (without).
// sgl6_gpu_base <graph prefix> <6path|dumbbell> counts the two 6-vertex patterns sgl_gpu_base answers "Not implemented" for (gm_sgl6): the
// banner and the last line `total_num = N` are sgl_gpu_base's.
// tclist_gpu_base <graph prefix> [out.bin [first [cap]]] lists the triangles (gm_tc_list): `total_num_triangles = N` in tc_gpu_base's
// spelling, then `triangles_written = M`; with out.bin the M triples of the window go there as raw little-endian int32, a < b < c.
// cliquelocal_gpu_base <graph prefix> <k> [out prefix] counts the k-cliques at every vertex and on every edge (gm_clique_local):
// `total_num_cliques = N` in kcl_gpu_base's spelling, then `max_vertex_cliques = A` and `max_edge_cliques = B`; with an out prefix the
// per-vertex counts go to <out>.vertex.u64 and the per-entry counts to <out>.entry.u64 as raw little-endian uint64.
// rectlocal_gpu_base <graph prefix> [out prefix] counts the 4-cycles at every vertex and on every edge (gm_rect_local): `max_vertex_rectangles
// = A` and `max_edge_rectangles = B`, then `total_num = N` in sgl_gpu_base's spelling as the last line; the same two files with an out prefix.
// motiflocal_gpu_base <graph prefix> <k> [out prefix] counts the graphlet-degree orbits of every vertex (gm_motif_local, k = 3 | 4): one line
// `orbit <o>: sum = S max = M` per orbit, then `pattern <i>: <count>` as motif_gpu_base's last lines; with an out prefix the orbits go to
// <out>.orbits.u64 as raw little-endian uint64, orbit-major.
// cliquelist_gpu_base <graph prefix> <k> [out.bin [first [cap]]] lists the k-cliques (gm_clique_list, 3 <= k <= 8): `total_num_cliques = N`
// in kcl_gpu_base's spelling, then `cliques_written = M`; with out.bin the M rows of the window go there as raw little-endian int32, k ids
// ascending per row.
// cliquecore_gpu_base <graph prefix> <k> [c] [out prefix] peels the k-clique counts (2 <= k <= 8).  With c (a number) the (k, c)-core
// (gm_clique_kcore): `core_vertices = N`, `core_cliques = M`, `rounds = R`.  Without it the decomposition (gm_clique_core_decompose):
// `rounds = R`, `dense_round = r`, `dense_vertices = N`, `dense_cliques = M`, `dense_density = M / N`, last line `max_core = C`; with an out
// prefix the core numbers go to <out>.core.bin as raw little-endian uint64 and the rounds to <out>.round.bin as uint32.
// cliquetruss_gpu_base <graph prefix> <k> [c] [out prefix] peels the per-edge k-clique counts (3 <= k <= 8).  With c (a number) the (k, c)-truss
// (gm_clique_ktruss): `truss_edges = N`, `truss_cliques = M`, `rounds = R`; with an out prefix the per-entry counts go to <out>.cnt.bin as raw
// little-endian uint64.  Without c the decomposition (gm_clique_truss_decompose): `rounds = R`, last line `max_truss = C`; with an out prefix
// the per-entry theta goes to <out>.theta.bin as uint64 and the rounds to <out>.round.bin as uint32.
// nucleus34_gpu_base <graph prefix> [c] [out prefix] peels the per-triangle 4-clique counts into the (3,4)-nuclei: `total_num_triangles = T`
// and `total_num_cliques = N` (gm_tc_list, gm_tri_clique4_local) first.  With c (a number) the c-nucleus set (gm_nucleus34):
// `nucleus_triangles = N`, `nucleus_cliques = M`, `rounds = R`.  Without it the decomposition (gm_nucleus34_decompose): `rounds = R`, last
// line `max_nucleus = C`.  With an out prefix the gm_tc_list rows go to <out>.tri.bin as raw little-endian int32 triples -- row t is the
// triangle of every other file's value t --, the per-triangle counts to <out>.cnt.bin (with c) or theta to <out>.theta.bin and the rounds
// to <out>.round.bin (without), all uint32.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/graphminer_amd.h"
#include "../host/host_graph.h"

#define GM_TC 1
#define GM_SGL 2
#define GM_CLIQUE 3
#define GM_MOTIF 4
#define GM_TRUSS 5
#define GM_SGL6 6
#define GM_TCLIST 7
#define GM_CLIQUELOCAL 8
#define GM_RECTLOCAL 9
#define GM_MOTIFLOCAL 10
#define GM_CLIQUELIST 11
#define GM_CLIQUECORE 12
#define GM_CLIQUETRUSS 13
#define GM_NUCLEUS34 14
#if defined(GM_APP) && (GM_APP == GM_TRUSS || GM_APP == GM_TCLIST || GM_APP == GM_CLIQUELOCAL || GM_APP == GM_RECTLOCAL || GM_APP == GM_MOTIFLOCAL || \
                        GM_APP == GM_CLIQUELIST || GM_APP == GM_CLIQUECORE || GM_APP == GM_CLIQUETRUSS || GM_APP == GM_NUCLEUS34)
#include <hip/hip_runtime_api.h>
#endif
#ifndef GM_APP
#error "compile with -DGM_APP=GM_TC|GM_SGL|GM_CLIQUE|GM_MOTIF|GM_TRUSS|GM_SGL6|GM_TCLIST|GM_CLIQUELOCAL|GM_RECTLOCAL|GM_MOTIFLOCAL|GM_CLIQUELIST|GM_CLIQUECORE|GM_CLIQUETRUSS|GM_NUCLEUS34"
#endif

namespace {

struct Cli {
  std::string graph;   // <graph> prefix
  std::string second;  // <pattern> (sgl) or <k> (clique, motif)
  int n_gpu = 1;       // [num_gpu(1)]
  int chunk = 0;       // [chunk_size(1024)]: honoured when given; omitted = 0 = the library default (<= 1024 task edges, adapted to the rank count)
  int adj_sorted = 1;  // [adj_sorted(1)] (tc only)
};

#if GM_APP != GM_TRUSS && GM_APP != GM_TCLIST && GM_APP != GM_CLIQUELOCAL && GM_APP != GM_RECTLOCAL && GM_APP != GM_MOTIFLOCAL && GM_APP != GM_CLIQUELIST && \
    GM_APP != GM_CLIQUECORE && GM_APP != GM_CLIQUETRUSS && GM_APP != GM_NUCLEUS34
// positional layout: TC has no <second>; the others do
Cli parse(int argc, char **argv, bool has_second) {
  Cli c;
  int i = 1;
  c.graph = argv[i++];
  if (has_second) c.second = argv[i++];
  if (i < argc) c.n_gpu = std::atoi(argv[i++]);
  if (i < argc) c.chunk = std::atoi(argv[i++]);
  if (i < argc) c.adj_sorted = std::atoi(argv[i++]);
#ifndef GM_APP_MULTIGPU
  c.n_gpu = 1;  // *_gpu_base binaries ignore num_gpu, as the reference's gpu_base solvers do
#endif
  return c;
}
#endif

void usage_and_exit(const char *self) {
#if GM_APP == GM_TC
  std::printf("Usage: %s <graph> [num_gpu(1)] [chunk_size(1024)] [adj_sorted(1)]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph\n", self);
#elif GM_APP == GM_SGL
  std::fprintf(stderr, "usage: %s <graph prefix> <pattern> [num_gpu(1)] [chunk_size(1024)]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph rectangle\n", self);
#elif GM_APP == GM_SGL6
  std::fprintf(stderr, "usage: %s <graph prefix> <6path|dumbbell>\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 6path\n", self);
#elif GM_APP == GM_TRUSS
  std::printf("Usage: %s <graph prefix> [k]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4\n", self);
#elif GM_APP == GM_TCLIST
  std::printf("Usage: %s <graph prefix> [out.bin [first [cap]]]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph triangles.bin 0 1000000\n", self);
#elif GM_APP == GM_CLIQUELIST
  std::printf("Usage: %s <graph prefix> <k> [out.bin [first [cap]]]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4 cliques.bin 0 1000000\n", self);
#elif GM_APP == GM_CLIQUECORE
  std::printf("Usage: %s <graph prefix> <k> [c] [out prefix]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4 cores\n", self);
#elif GM_APP == GM_CLIQUETRUSS
  std::printf("Usage: %s <graph prefix> <k> [c] [out prefix]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4 trusses\n", self);
#elif GM_APP == GM_NUCLEUS34
  std::printf("Usage: %s <graph prefix> [c] [out prefix]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph nuclei\n", self);
#elif GM_APP == GM_CLIQUELOCAL
  std::printf("Usage: %s <graph prefix> <k> [out prefix]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4 cliques\n", self);
#elif GM_APP == GM_RECTLOCAL
  std::printf("Usage: %s <graph prefix> [out prefix]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph rectangles\n", self);
#elif GM_APP == GM_MOTIFLOCAL
  std::printf("Usage: %s <graph prefix> <k> [out prefix]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4 orbits\n", self);
#else
  std::printf("Usage: %s<graph> <k> [ngpu(0)] [chunk_size(1024)]\n", self);
  std::printf("Example: %s /graph_inputs/mico/graph 4\n", self);
#endif
  std::exit(1);
}

}  // namespace

// `--dev NAME=VALUE` anywhere on the command line sets a developer option of the library (gm_dev_option, include/graphminer_amd.h: the
// switches tests use to reach a path on a small graph) and is removed from argv before the reference's positional layout is read.
// Nothing is read from the environment.
static int strip_dev_options(int argc, char **argv) {
  int n = 0;
  for (int i = 0; i < argc; ++i) {
    if (std::string(argv[i]) == "--dev" && i + 1 < argc) {
      const std::string kv = argv[++i];
      const size_t eq = kv.find('=');
      const int rc = eq == std::string::npos ? gm_dev_option(kv.c_str(), "1") : gm_dev_option(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str());
      if (rc != GM_OK) {
        std::fprintf(stderr, "bad --dev option: %s\n", kv.c_str());
        std::exit(1);
      }
      continue;
    }
    argv[n++] = argv[i];
  }
  return n;
}

int main(int argc, char **argv) {
  argc = strip_dev_options(argc, argv);
  const bool has_second = (GM_APP != GM_TC && GM_APP != GM_TRUSS && GM_APP != GM_TCLIST && GM_APP != GM_RECTLOCAL && GM_APP != GM_NUCLEUS34);
  if (argc < (has_second ? 3 : 2)) usage_and_exit(argv[0]);
#if GM_APP == GM_TRUSS || GM_APP == GM_TCLIST || GM_APP == GM_CLIQUELOCAL || GM_APP == GM_RECTLOCAL || GM_APP == GM_MOTIFLOCAL || GM_APP == GM_CLIQUELIST || \
    GM_APP == GM_CLIQUECORE || GM_APP == GM_CLIQUETRUSS || GM_APP == GM_NUCLEUS34
  Cli c;
  c.graph = argv[1];
  if (argc > 2) c.second = argv[2];  // [k] / [out.bin] / <k> / [out prefix]
#else
  const Cli c = parse(argc, argv, has_second);
#endif

#if GM_APP == GM_TC
  std::printf("Triangle Counting: we assume the neighbor lists are sorted.\n");
  std::fflush(stdout);
  Graph g(c.graph, USE_DAG);
  g.print_meta_data();
  if (!c.adj_sorted) g.sort_neighbors();  // src/triangle/main.cc:22
  uint64_t total = 0;
  TCSolver(g, total, c.n_gpu, c.chunk);
  std::printf("total_num_triangles = %llu\n", (unsigned long long)total);

#elif GM_APP == GM_SGL
  std::printf("Subgraph Listing/Counting (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  Pattern patt(c.second);
  std::printf("Pattern: %s\n", patt.get_name().c_str());
  std::fflush(stdout);
  g.print_meta_data();
  uint64_t total = 0;
  SglSolver(g, patt, total, c.n_gpu, c.chunk);
  std::printf("total_num = %llu\n", (unsigned long long)total);

#elif GM_APP == GM_CLIQUE
  std::printf("k-clique listing with undirected graphs\n");
  if (USE_DAG) std::printf("Using DAG (static orientation)\n");
  std::fflush(stdout);
  Graph g(c.graph, USE_DAG);
  const int k = std::atoi(c.second.c_str());
  g.print_meta_data();
  uint64_t total = 0;
  CliqueSolver(g, k, total, c.n_gpu, c.chunk);
#ifdef GM_KCL_SPELLING
  std::printf("\ntotal_num_cliques = %llu\n\n", (unsigned long long)total);
#else
  std::printf("num_%d-cliques = %llu\n", k, (unsigned long long)total);
#endif

#elif GM_APP == GM_TRUSS
  std::printf("k-truss (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t n_edges = 0;
  int32_t k_max = 0, rounds = 0;
  const bool with_k = !c.second.empty();
  const int k = with_k ? std::atoi(c.second.c_str()) : 0;
  uint32_t *d_tau = nullptr;
  if (rc == GM_OK && with_k) rc = gm_ktruss(h, k, nullptr, nullptr, &n_edges, &rounds, nullptr);
  if (rc == GM_OK && !with_k) {
    // (the trussness array is the call's result and the caller's buffer)
    if (hipMalloc(reinterpret_cast<void **>(&d_tau), sizeof(uint32_t) * (size_t)(csr.ne > 0 ? csr.ne : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK) rc = gm_truss_decompose(h, nullptr, d_tau, &k_max, &rounds, nullptr);
    if (d_tau) (void)hipFree(d_tau);
  }
  gm_graph_free(h);
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("rounds = %d\n", (int)rounds);
  if (with_k) std::printf("ktruss_edges = %llu\n", (unsigned long long)n_edges);
  else std::printf("max_truss = %d\n", (int)k_max);

#elif GM_APP == GM_TCLIST
  std::printf("Triangle Listing (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const uint64_t first = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 0;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t total = 0, written = 0;
  if (rc == GM_OK) rc = gm_tc_list(h, nullptr, 0, 0, nullptr, &total, nullptr, nullptr);  // (count only: sizes the buffer)
  if (rc == GM_OK && !c.second.empty()) {
    uint64_t cap = first < total ? total - first : 0;
    if (argc > 4) cap = std::min<uint64_t>(cap, std::strtoull(argv[4], nullptr, 10));
    std::vector<int32_t> tri((size_t)(3 * cap));
    int32_t *d_tri = nullptr;
    if (cap > 0 && hipMalloc(reinterpret_cast<void **>(&d_tri), sizeof(int32_t) * tri.size()) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && cap > 0) rc = gm_tc_list(h, nullptr, first, cap, d_tri, &total, &written, nullptr);
    if (rc == GM_OK && written > 0 && hipMemcpy(tri.data(), d_tri, sizeof(int32_t) * 3 * (size_t)written, hipMemcpyDeviceToHost) != hipSuccess)
      rc = GM_ERR_HIP;
    if (d_tri) (void)hipFree(d_tri);
    if (rc == GM_OK) {  // (the hosts this runs on are little-endian: the ints go out as they lie in memory)
      FILE *f = std::fopen(c.second.c_str(), "wb");
      const size_t n = 3 * (size_t)written;
      const bool ok = f && std::fwrite(tri.data(), sizeof(int32_t), n, f) == n;
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  gm_graph_free(h);
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("total_num_triangles = %llu\n", (unsigned long long)total);
  std::printf("triangles_written = %llu\n", (unsigned long long)written);

#elif GM_APP == GM_CLIQUELIST
  std::printf("k-clique Listing (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const int k = std::atoi(c.second.c_str());
  const std::string out = argc > 3 ? argv[3] : "";
  const uint64_t first = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 0;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t total = 0, written = 0;
  if (rc == GM_OK) rc = gm_clique_list(h, k, nullptr, 0, 0, nullptr, &total, nullptr, nullptr);  // (count only: sizes the buffer)
  if (rc == GM_OK && !out.empty()) {
    uint64_t cap = first < total ? total - first : 0;
    if (argc > 5) cap = std::min<uint64_t>(cap, std::strtoull(argv[5], nullptr, 10));
    std::vector<int32_t> rows((size_t)k * (size_t)cap);
    int32_t *d_rows = nullptr;
    if (cap > 0 && hipMalloc(reinterpret_cast<void **>(&d_rows), sizeof(int32_t) * rows.size()) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && cap > 0) rc = gm_clique_list(h, k, nullptr, first, cap, d_rows, &total, &written, nullptr);
    if (rc == GM_OK && written > 0 && hipMemcpy(rows.data(), d_rows, sizeof(int32_t) * (size_t)k * (size_t)written, hipMemcpyDeviceToHost) != hipSuccess)
      rc = GM_ERR_HIP;
    if (d_rows) (void)hipFree(d_rows);
    if (rc == GM_OK) {  // (the hosts this runs on are little-endian: the ints go out as they lie in memory)
      FILE *f = std::fopen(out.c_str(), "wb");
      const size_t n = (size_t)k * (size_t)written;
      const bool ok = f && std::fwrite(rows.data(), sizeof(int32_t), n, f) == n;
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  gm_graph_free(h);
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("total_num_cliques = %llu\n", (unsigned long long)total);
  std::printf("cliques_written = %llu\n", (unsigned long long)written);

#elif GM_APP == GM_CLIQUELOCAL
  std::printf("local k-clique counts (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const int k = std::atoi(c.second.c_str());
  const std::string out = argc > 3 ? argv[3] : "";
  const size_t nv = (size_t)csr.nv, ne = (size_t)csr.ne;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t total = 0;
  std::vector<uint64_t> kv(nv), ke(ne);
  uint64_t *d_kv = nullptr, *d_ke = nullptr;
  // (the two arrays are the call's results and the caller's buffers)
  if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_kv), sizeof(uint64_t) * (nv > 0 ? nv : 1)) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_ke), sizeof(uint64_t) * (ne > 0 ? ne : 1)) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK) rc = gm_clique_local(h, k, nullptr, d_kv, d_ke, &total, nullptr);
  if (rc == GM_OK && nv > 0 && hipMemcpy(kv.data(), d_kv, sizeof(uint64_t) * nv, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK && ne > 0 && hipMemcpy(ke.data(), d_ke, sizeof(uint64_t) * ne, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
  if (d_kv) (void)hipFree(d_kv);
  if (d_ke) (void)hipFree(d_ke);
  gm_graph_free(h);
  if (rc == GM_OK && !out.empty()) {  // (the hosts this runs on are little-endian: the counts go out as they lie in memory)
    const struct { std::string path; const std::vector<uint64_t> *v; } files[2] = {{out + ".vertex.u64", &kv}, {out + ".entry.u64", &ke}};
    for (const auto &file : files) {
      FILE *f = std::fopen(file.path.c_str(), "wb");
      const bool ok = f && std::fwrite(file.v->data(), sizeof(uint64_t), file.v->size(), f) == file.v->size();
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("\ntotal_num_cliques = %llu\n\n", (unsigned long long)total);
  std::printf("max_vertex_cliques = %llu\n", (unsigned long long)(kv.empty() ? 0 : *std::max_element(kv.begin(), kv.end())));
  std::printf("max_edge_cliques = %llu\n", (unsigned long long)(ke.empty() ? 0 : *std::max_element(ke.begin(), ke.end())));

#elif GM_APP == GM_CLIQUECORE
  std::printf("k-clique cores (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const int k = std::atoi(c.second.c_str());
  // [c] is a number, [out prefix] is not
  const bool with_c = argc > 3 && argv[3][0] != '\0' && std::string(argv[3]).find_first_not_of("0123456789") == std::string::npos;
  const uint64_t cc = with_c ? std::strtoull(argv[3], nullptr, 10) : 0;
  const std::string out = argc > (with_c ? 4 : 3) ? argv[with_c ? 4 : 3] : "";
  const size_t nv = (size_t)csr.nv;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t n_vertices = 0, n_cliques = 0, c_max = 0;
  int32_t rounds = 0;
  gm_core_dense dense{1, 0, 0};
  std::vector<uint64_t> core(nv);
  std::vector<uint32_t> round(nv);
  if (rc == GM_OK && with_c) rc = gm_clique_kcore(h, k, cc, nullptr, nullptr, &n_vertices, &n_cliques, &rounds, nullptr);
  if (rc == GM_OK && !with_c) {
    // (the two arrays are the call's results and the caller's buffers)
    uint64_t *d_core = nullptr;
    uint32_t *d_round = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_core), sizeof(uint64_t) * (nv > 0 ? nv : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_round), sizeof(uint32_t) * (nv > 0 ? nv : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK) rc = gm_clique_core_decompose(h, k, nullptr, d_core, d_round, &c_max, &rounds, &dense, nullptr);
    if (rc == GM_OK && nv > 0 && hipMemcpy(core.data(), d_core, sizeof(uint64_t) * nv, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && nv > 0 && hipMemcpy(round.data(), d_round, sizeof(uint32_t) * nv, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (d_core) (void)hipFree(d_core);
    if (d_round) (void)hipFree(d_round);
  }
  gm_graph_free(h);
  if (rc == GM_OK && !with_c && !out.empty()) {  // (the hosts this runs on are little-endian: the values go out as they lie in memory)
    const struct { std::string path; const void *data; size_t size; } files[2] = {{out + ".core.bin", core.data(), sizeof(uint64_t)},
                                                                                 {out + ".round.bin", round.data(), sizeof(uint32_t)}};
    for (const auto &file : files) {
      FILE *f = std::fopen(file.path.c_str(), "wb");
      const bool ok = f && std::fwrite(file.data, file.size, nv, f) == nv;
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  if (with_c) {
    std::printf("core_vertices = %llu\n", (unsigned long long)n_vertices);
    std::printf("core_cliques = %llu\n", (unsigned long long)n_cliques);
    std::printf("rounds = %d\n", (int)rounds);
  } else {
    std::printf("rounds = %d\n", (int)rounds);
    std::printf("dense_round = %d\n", (int)dense.round);
    std::printf("dense_vertices = %llu\n", (unsigned long long)dense.vertices);
    std::printf("dense_cliques = %llu\n", (unsigned long long)dense.cliques);
    std::printf("dense_density = %.6f\n", dense.vertices ? (double)dense.cliques / (double)dense.vertices : 0.0);
    std::printf("max_core = %llu\n", (unsigned long long)c_max);
  }

#elif GM_APP == GM_CLIQUETRUSS
  std::printf("k-clique trusses (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const int k = std::atoi(c.second.c_str());
  // [c] is a number, [out prefix] is not
  const bool with_c = argc > 3 && argv[3][0] != '\0' && std::string(argv[3]).find_first_not_of("0123456789") == std::string::npos;
  const uint64_t cc = with_c ? std::strtoull(argv[3], nullptr, 10) : 0;
  const std::string out = argc > (with_c ? 4 : 3) ? argv[with_c ? 4 : 3] : "";
  const size_t ne = (size_t)csr.ne;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t n_edges = 0, n_cliques = 0, c_max = 0;
  int32_t rounds = 0;
  std::vector<uint64_t> wide(ne);   // K_e inside the truss, or theta
  std::vector<uint32_t> round(ne);
  if (rc == GM_OK) {
    // (the arrays are the call's results and the caller's buffers)
    uint64_t *d_wide = nullptr;
    uint32_t *d_round = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_wide), sizeof(uint64_t) * (ne > 0 ? ne : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_round), sizeof(uint32_t) * (ne > 0 ? ne : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && with_c) rc = gm_clique_ktruss(h, k, cc, nullptr, d_wide, &n_edges, &n_cliques, &rounds, nullptr);
    if (rc == GM_OK && !with_c) rc = gm_clique_truss_decompose(h, k, nullptr, d_wide, d_round, &c_max, &rounds, nullptr);
    if (rc == GM_OK && ne > 0 && hipMemcpy(wide.data(), d_wide, sizeof(uint64_t) * ne, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && !with_c && ne > 0 && hipMemcpy(round.data(), d_round, sizeof(uint32_t) * ne, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (d_wide) (void)hipFree(d_wide);
    if (d_round) (void)hipFree(d_round);
  }
  gm_graph_free(h);
  if (rc == GM_OK && !out.empty()) {  // (the hosts this runs on are little-endian: the values go out as they lie in memory)
    const struct { std::string path; const void *data; size_t size; } files[2] = {{out + (with_c ? ".cnt.bin" : ".theta.bin"), wide.data(), sizeof(uint64_t)},
                                                                                 {out + ".round.bin", round.data(), sizeof(uint32_t)}};
    for (int i = 0; i < (with_c ? 1 : 2); ++i) {
      FILE *f = std::fopen(files[i].path.c_str(), "wb");
      const bool ok = f && std::fwrite(files[i].data, files[i].size, ne, f) == ne;
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  if (with_c) {
    std::printf("truss_edges = %llu\n", (unsigned long long)n_edges);
    std::printf("truss_cliques = %llu\n", (unsigned long long)n_cliques);
    std::printf("rounds = %d\n", (int)rounds);
  } else {
    std::printf("rounds = %d\n", (int)rounds);
    std::printf("max_truss = %llu\n", (unsigned long long)c_max);
  }

#elif GM_APP == GM_NUCLEUS34
  std::printf("triangle nuclei (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  // [c] is a number, [out prefix] is not
  const bool with_c = argc > 2 && argv[2][0] != '\0' && std::string(argv[2]).find_first_not_of("0123456789") == std::string::npos;
  const uint32_t cc = with_c ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 0;
  const std::string out = argc > (with_c ? 3 : 2) ? argv[with_c ? 3 : 2] : "";
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t T = 0, written = 0, total_k4 = 0, n_tri = 0, n_cliques = 0;
  uint32_t c_max = 0;
  int32_t rounds = 0;
  if (rc == GM_OK) rc = gm_tc_list(h, nullptr, 0, 0, nullptr, &T, nullptr, nullptr);  // (count only: sizes the per-triangle arrays)
  const size_t nt = (size_t)T;
  std::vector<int32_t> tri(3 * nt);
  std::vector<uint32_t> val(nt), round(nt);  // the count inside the set, or theta
  if (rc == GM_OK) {
    // (the arrays are the calls' results and the caller's buffers)
    int32_t *d_tri = nullptr;
    uint32_t *d_val = nullptr, *d_round = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_tri), sizeof(int32_t) * 3 * (nt > 0 ? nt : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_val), sizeof(uint32_t) * (nt > 0 ? nt : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_round), sizeof(uint32_t) * (nt > 0 ? nt : 1)) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && nt > 0 && !out.empty()) rc = gm_tc_list(h, nullptr, 0, T, d_tri, &T, &written, nullptr);
    if (rc == GM_OK) rc = gm_tri_clique4_local(h, nullptr, T, nullptr, &total_k4, nullptr);
    if (rc == GM_OK && with_c) rc = gm_nucleus34(h, cc, nullptr, T, d_val, &n_tri, &n_cliques, &rounds, nullptr);
    if (rc == GM_OK && !with_c) rc = gm_nucleus34_decompose(h, nullptr, T, d_val, d_round, &c_max, &rounds, nullptr);
    if (rc == GM_OK && written > 0 && hipMemcpy(tri.data(), d_tri, sizeof(int32_t) * 3 * nt, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && nt > 0 && hipMemcpy(val.data(), d_val, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (rc == GM_OK && !with_c && nt > 0 && hipMemcpy(round.data(), d_round, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
    if (d_tri) (void)hipFree(d_tri);
    if (d_val) (void)hipFree(d_val);
    if (d_round) (void)hipFree(d_round);
  }
  gm_graph_free(h);
  if (rc == GM_OK && !out.empty()) {  // (the hosts this runs on are little-endian: the values go out as they lie in memory)
    const struct { std::string path; const void *data; size_t n; } files[3] = {{out + ".tri.bin", tri.data(), 3 * nt},
                                                                              {out + (with_c ? ".cnt.bin" : ".theta.bin"), val.data(), nt},
                                                                              {out + ".round.bin", round.data(), nt}};
    for (int i = 0; i < (with_c ? 2 : 3); ++i) {
      FILE *f = std::fopen(files[i].path.c_str(), "wb");
      const bool ok = f && std::fwrite(files[i].data, 4, files[i].n, f) == files[i].n;
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("total_num_triangles = %llu\n", (unsigned long long)T);
  std::printf("total_num_cliques = %llu\n", (unsigned long long)total_k4);
  if (with_c) {
    std::printf("nucleus_triangles = %llu\n", (unsigned long long)n_tri);
    std::printf("nucleus_cliques = %llu\n", (unsigned long long)n_cliques);
    std::printf("rounds = %d\n", (int)rounds);
  } else {
    std::printf("rounds = %d\n", (int)rounds);
    std::printf("max_nucleus = %u\n", (unsigned)c_max);
  }

#elif GM_APP == GM_RECTLOCAL
  std::printf("local 4-cycle counts (undirected graph only)\n");
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const std::string out = c.second;
  const size_t nv = (size_t)csr.nv, ne = (size_t)csr.ne;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t total = 0;
  std::vector<uint64_t> rv(nv), re(ne);
  uint64_t *d_rv = nullptr, *d_re = nullptr;
  // (the two arrays are the call's results and the caller's buffers)
  if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_rv), sizeof(uint64_t) * (nv > 0 ? nv : 1)) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_re), sizeof(uint64_t) * (ne > 0 ? ne : 1)) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK) rc = gm_rect_local(h, nullptr, d_rv, d_re, &total, nullptr);
  if (rc == GM_OK && nv > 0 && hipMemcpy(rv.data(), d_rv, sizeof(uint64_t) * nv, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK && ne > 0 && hipMemcpy(re.data(), d_re, sizeof(uint64_t) * ne, hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
  if (d_rv) (void)hipFree(d_rv);
  if (d_re) (void)hipFree(d_re);
  gm_graph_free(h);
  if (rc == GM_OK && !out.empty()) {  // (the hosts this runs on are little-endian: the counts go out as they lie in memory)
    const struct { std::string path; const std::vector<uint64_t> *v; } files[2] = {{out + ".vertex.u64", &rv}, {out + ".entry.u64", &re}};
    for (const auto &file : files) {
      FILE *f = std::fopen(file.path.c_str(), "wb");
      const bool ok = f && std::fwrite(file.v->data(), sizeof(uint64_t), file.v->size(), f) == file.v->size();
      if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
      if (!ok) rc = GM_ERR_IO;
    }
  }
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("max_vertex_rectangles = %llu\n", (unsigned long long)(rv.empty() ? 0 : *std::max_element(rv.begin(), rv.end())));
  std::printf("max_edge_rectangles = %llu\n", (unsigned long long)(re.empty() ? 0 : *std::max_element(re.begin(), re.end())));
  std::printf("total_num = %llu\n", (unsigned long long)total);

#elif GM_APP == GM_MOTIFLOCAL
  const int k = std::atoi(c.second.c_str());
  std::printf("local %d-motif counts (undirected graph only)\n", k);
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  const std::string out = argc > 3 ? argv[3] : "";
  const size_t nv = (size_t)csr.nv, no = k == 3 ? 4 : 15, nc = k == 3 ? 2 : 6;
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  std::vector<uint64_t> orb(no * nv), counts(nc, 0);
  uint64_t *d_orb = nullptr;
  // (the array is the call's result and the caller's buffer)
  if (rc == GM_OK && hipMalloc(reinterpret_cast<void **>(&d_orb), sizeof(uint64_t) * (orb.empty() ? 1 : orb.size())) != hipSuccess) rc = GM_ERR_HIP;
  if (rc == GM_OK) rc = gm_motif_local(h, k, nullptr, d_orb, counts.data(), (int)nc, nullptr);
  if (rc == GM_OK && !orb.empty() && hipMemcpy(orb.data(), d_orb, sizeof(uint64_t) * orb.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = GM_ERR_HIP;
  if (d_orb) (void)hipFree(d_orb);
  gm_graph_free(h);
  if (rc == GM_OK && !out.empty()) {  // (the hosts this runs on are little-endian: the counts go out as they lie in memory)
    FILE *f = std::fopen((out + ".orbits.u64").c_str(), "wb");
    const bool ok = f && std::fwrite(orb.data(), sizeof(uint64_t), orb.size(), f) == orb.size();
    if (f && std::fclose(f) != 0) rc = GM_ERR_IO;
    if (!ok) rc = GM_ERR_IO;
  }
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  for (size_t o = 0; o < no; ++o) {
    uint64_t sum = 0, mx = 0;
    for (size_t v = 0; v < nv; ++v) {
      sum += orb[o * nv + v];
      mx = std::max(mx, orb[o * nv + v]);
    }
    std::printf("orbit %d: sum = %llu max = %llu\n", (int)o, (unsigned long long)sum, (unsigned long long)mx);
  }
  std::printf("num_patterns: %d\n", (int)nc);
  for (size_t i = 0; i < nc; ++i) std::printf("pattern %d: %llu\n", (int)i, (unsigned long long)counts[i]);

#elif GM_APP == GM_SGL6
  std::printf("Subgraph Listing/Counting (undirected graph only)\n");
  std::printf("Pattern: %s\n", c.second.c_str());
  std::fflush(stdout);
  Graph g(c.graph);
  g.print_meta_data();
  const gm_csr csr = g.csr();
  gm_graph *h = nullptr;
  int rc = gm_graph_upload(&csr, 0, &h);
  uint64_t total = 0;
  if (rc == GM_OK) rc = gm_sgl6(h, c.second.c_str(), nullptr, &total, nullptr);
  gm_graph_free(h);
  if (rc != GM_OK) {
    std::fprintf(stderr, "%s: %s %s\n", argv[0], gm_strerror(rc), gm_last_error());
    return 1;
  }
  std::printf("total_num = %llu\n", (unsigned long long)total);

#elif GM_APP == GM_MOTIF
  Graph g(c.graph);
  const int k = std::atoi(c.second.c_str());
  std::printf("%d-motif counting (only for undirected graphs)\n", k);
  std::fflush(stdout);
  g.print_meta_data();
  if (k < 0 || k > 9) return 1;
  const int np = num_possible_patterns[k];
  std::printf("num_patterns: %d\n", np);
  std::fflush(stdout);
  std::vector<uint64_t> counts((size_t)np, 0);
  MotifSolver(g, k, counts, c.n_gpu, c.chunk);
  for (int i = 0; i < np; ++i) std::printf("pattern %d: %llu\n", i, (unsigned long long)counts[(size_t)i]);
#endif
  return 0;
}
