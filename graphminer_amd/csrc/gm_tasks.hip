// gm_tasks.hip -- the task structures of the triangle-count family, built on the device once per handle: edge descriptors, the task lists
// and the key stream of gm_tch.hip (with the hub corner / the block pairs gm_ctc.hip takes), the match masks and the symmetric corner of
// the edge supports (gm_sup.hip), the rows beyond the stage.  Each is a Once<T> of the handle (gm_host.h).
#include "gm_host.h"
#include "gm_scan.h"
using namespace gm;

// Edge descriptors (GraphView::edesc): one gather pass over the CSR, once per graph -- the device-side counterpart of
// Graph::init_edgelist (src/common/graph.cc:297-326), which builds the reference's COO task list serially on the host.
__global__ __launch_bounds__(256) void edesc_kernel(long long ne, const int *__restrict__ rp, const int *__restrict__ col, int2 *__restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += stride) {
    const int v = col[e];
    const int r = rp[v];
    out[e] = make_int2(r, rp[v + 1] - r);
  }
}

// ---- task lists of gm_tch.hip / gm_tch.hip: every edge u -> v of the DAG is a task of ONE of its endpoints (ensure_tasklists, below) ------
// ---- task-major copies of the short lists (gm_host.h: TaskLists::colk / tdesck) -- for the handles that cannot have the key stream -----------
#ifndef GM_TC_INLINE_MAX_DEFAULT
#define GM_TC_INLINE_MAX_DEFAULT 32
#endif
// len[t] = keys of task t that go into the copies (0: none)
__global__ __launch_bounds__(256) void inl_len_kernel(long long nt, const int2 *__restrict__ tdesc, int lmax, unsigned long long *__restrict__ len) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t <= nt; t += stride) {
    const int n = t < nt ? tdesc[t].y : 0;
    len[t] = (n > 0 && n <= lmax) ? (unsigned long long)n : 0ull;
  }
}
// eight lanes per task: its keys move from their row of col[] to their place in task order, the descriptor follows
__global__ __launch_bounds__(256) void inl_copy_kernel(long long nt, const int2 *__restrict__ tdesc, const unsigned long long *__restrict__ off, int lmax,
                                                        long long ne, int *__restrict__ colk, int2 *__restrict__ tdesck) {
  const long long stride = ((long long)gridDim.x * blockDim.x) >> 3;
  const int sub = threadIdx.x & 7;
  for (long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 3; t < nt; t += stride) {
    const int2 d = tdesc[t];
    if (d.y > 0 && d.y <= lmax) {
      const long long o = ne + (long long)off[t];
      for (int i = sub; i < d.y; i += 8) colk[o + i] = colk[d.x + i];  // (the first ne entries of colk are col itself)
      if (sub == 0) tdesck[t] = make_int2((int)o, d.y);
    } else if (sub == 0) {
      tdesck[t] = d;
    }
  }
}
// after the lists, into the same local of ensure_tasklists, which drops the code: failures here leave the handle without copies (the kernels then stream the rows themselves)
static int build_inline_copies(gm_graph *g, TaskLists &tl, ScanTemp &tmp) {
  int lmax = GM_TC_INLINE_MAX_DEFAULT;
  if (const char *e = gm_sweep_env("GM_TC_INLINE_MAX")) lmax = atoi(e);  // (sweeps; 0: no copies)
  if (lmax <= 0 || g->ne <= 0 || tl.tdesc == nullptr) return GM_OK;
  const long long nt = g->ne;
  DevOwn<unsigned long long> off;  // (lengths in, offsets out: the scan runs in place)
  DevOwn<int> colk;
  DevOwn<int2> tdk;
  HIP_TRY(off.alloc(8 * (size_t)(nt + 1)));
  const long long nblocks = std::min<long long>((nt + 256) / 256, (long long)g->cu_count * 32);
  unsigned long long total = 0;
  for (;;) {  // the copies share the 32-bit index space of col[]: halve the limit until they fit
    hipLaunchKernelGGL(inl_len_kernel, dim3((unsigned)nblocks), dim3(256), 0, 0, nt, tl.tdesc.get(), lmax, off.get());
    HIP_TRY(dev_scan_total(tmp, off.get(), off.get(), (size_t)nt, &total));
    if ((unsigned long long)nt + total < 0x7fffff00ull) break;
    lmax >>= 1;
    if (lmax < 4) return GM_OK;
  }
  if (total == 0) return GM_OK;
  HIP_TRY(tdk.alloc(sizeof(int2) * (size_t)nt));
  HIP_TRY(colk.alloc(4 * ((size_t)nt + (size_t)total)));
  HIP_TRY(hipMemcpyAsync(colk, g->d_col, 4 * (size_t)nt, hipMemcpyDeviceToDevice, 0));
  const long long cblocks = std::min<long long>((nt * 8 + 255) / 256, (long long)g->cu_count * 64);
  hipLaunchKernelGGL(inl_copy_kernel, dim3((unsigned)cblocks), dim3(256), 0, 0, nt, tl.tdesc.get(), off.get(), lmax, nt, colk.get(), tdk.get());
  HIP_TRY(hipDeviceSynchronize());
  off.reset();
  tl.colk = std::move(colk);
  tl.tdesck = std::move(tdk);
  tl.n_copy_keys = total;
  return GM_OK;
}

// The task lists by COUNTING PLACEMENT (round 4; until then: one (host, entry) key per edge found by a bisection of the offsets, a radix
// sort of 40 - 260 M key / value pairs, a descriptor pass): eight lanes walk a row; pass 1 counts the tasks of every host, a scan gives
// the offsets, pass 2 repeats the walk and drops every task at its host's cursor -- descriptor, own entry and the low 8 bits of the host
// (the tag of the key stream) written where they stay.  The partner's {start, length} comes from the edge descriptors (coalesced) instead
// of two random reads of the offsets.  The order of a host's tasks is the order of arrival: nothing depends on it.
// Same-address atomics are what such a placement costs on a skewed graph (a hub of R-MAT-22 hosts 10^5 in-edges: 4.3 + 4.6 ms for the two
// passes, no better than the sort): (i) the tasks a row hosts itself are counted per 8-lane group, one atomic per group and step;
// (ii) on a topologically numbered DAG the hubs are the LAST ids: in-edge tasks of the last kHubWin hosts are counted in an LDS
// histogram per workgroup -- pass 2 reserves a range per (workgroup, hub) with one atomic and ranks its tasks inside it in LDS.
// (kHubWin and the passes' grid, row_walk_grid: gm_host.h)
struct TaskWalk {
  int nv, stage_max, topo, hub0;  // hosts >= hub0 are aggregated in LDS (nv: none)
  const int *rp, *col;
  const int2 *edesc;
  int skip_from = 0x7fffffff;     // the out-edges of the rows >= skip_from are no tasks (the triangle count takes them from the core bitmap, gm_ctc.hip)
  // ... or, chosen per pair of 256-row blocks (tc_pairs_setup): the edge u -> v of a row u >= region_from is no task when bit
  // ((u - region_from) >> 8) * pair_nb + ((v - region_from) >> 8) of pair_bits is set.  Its row keeps its length: positions and tails stay
  int region_from = 0x7fffffff, pair_nb = 0;
  const unsigned *pair_bits = nullptr;
};
// the walk over a handle's DAG (after ensure_edesc): every row that fits the stage, the last `win` hosts of a topological numbering
// aggregated in LDS; the callers set what differs (skip_from, the pair fields)
static TaskWalk task_walk_of(const gm_graph *g, const bool topo, const int win) {
  TaskWalk w;
  w.nv = g->nv; w.stage_max = kTctStageMax; w.topo = topo ? 1 : 0;
  w.hub0 = topo ? std::max(0, g->nv - win) : g->nv;
  w.rp = g->d_rp; w.col = g->d_col; w.edesc = *g->edesc;
  return w;
}
// calls f(u, i, e, ru, du, dv, tail, u_hosts) for every task edge of the rows u0 + 8 * (wave's trips of `stride` rows) below u_end (all 64
// lanes of a wave stay together: f may use wave ballots; `act` = the lane holds a task)
template <class F>
__device__ __forceinline__ void task_walk_rows(const TaskWalk &w, const long long u0, const long long u_end, const long long stride, F f) {
  const int sub = threadIdx.x & 7;
  for (long long ub = u0; ub < u_end; ub += stride) {
    const long long u = ub + ((threadIdx.x & 63) >> 3);
    int ru = 0, du = 0;
    if (u < u_end) {
      ru = w.rp[u];
      du = w.rp[u + 1] - ru;
      if (du > w.stage_max || u >= w.skip_from) du = 0;  // a row the stage cannot take hosts nothing, and its out-edges stay with the chunked kernel (run_pattern)
    }
    const int dmax = wave_max_nonneg(du);
    for (int i = sub; i - sub < dmax; i += 8) {  // wave-uniform trip count
      bool act = i < du;
      const int e = ru + (act ? i : 0);
      if (act && u >= w.region_from) {  // (topological: v > u, inside the region too)
        const int b = ((int)(u - w.region_from) >> 8) * w.pair_nb + ((w.col[e] - w.region_from) >> 8);
        act = ((w.pair_bits[b >> 5] >> (b & 31)) & 1u) == 0u;
      }
      const int2 dv = act ? w.edesc[e] : make_int2(0, 0);  // {rp[v], d+(v)} of the entry's target v
      // the host = the endpoint whose list is NOT streamed: N+(v) whole, or N+(u) -- under a topological numbering only its part beyond
      // v -- whichever is shorter (ties: the source hosts); a list that does not fit the stage never hosts
      const int tail = w.topo ? du - i - 1 : du;
      const bool u_hosts = dv.y > w.stage_max || tail >= dv.y;
      f(act, (int)u, i, e, ru, du, dv, tail, u_hosts);
    }
  }
}
// ... for every row of the graph, dealt to the waves of the grid (8 rows per wave and trip)
template <class F>
__device__ __forceinline__ void task_walk(const TaskWalk &w, F f) {
  task_walk_rows(w, ((long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63)) >> 3, (long long)w.nv, ((long long)gridDim.x * blockDim.x) >> 3, f);
}

template <bool PLACE>
__global__ __launch_bounds__(256) void task_rows_kernel(const TaskWalk w, int *__restrict__ cnt /* PLACE: the cursors */, const int *__restrict__ trp,
                                                         int2 *__restrict__ tdesc, int *__restrict__ tedge) {
  __shared__ int hist[kHubWin];
  for (int h = threadIdx.x; h < kHubWin; h += 256) hist[h] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane & 7, g8 = lane & ~7;
  auto put = [&](const int slot, const int host, const int e, const int ru, const int du, const int2 dv, const int tail, const bool u_hosts) {
    tdesc[slot] = u_hosts ? dv : (w.topo ? make_int2(e + 1, tail) : make_int2(ru, du));
    tedge[slot] = e;
  };
  task_walk(w, [&](const bool act, const int u, const int i, const int e, const int ru, const int du, const int2 dv, const int tail, const bool u_hosts) {
    // (i) the tasks the row hosts itself: one atomic per 8-lane group
    const unsigned long long mu = __ballot(act && u_hosts);
    const unsigned gm = (unsigned)(mu >> g8) & 255u;
    int ubase = 0;
    if (gm != 0u && sub == (int)__builtin_ctz(gm)) ubase = atomicAdd(&cnt[u], (int)__builtin_popcount(gm));
    if (PLACE && gm != 0u) {
      ubase = __shfl(ubase, g8 + (int)__builtin_ctz(gm));
      if (act && u_hosts) put(trp[u] + ubase + (int)__builtin_popcount(gm & ((1u << sub) - 1u)), u, e, ru, du, dv, tail, true);
    }
    // (ii) in-edge tasks: the target hosts -- a hub through the LDS histogram, anybody else through its global cursor
    if (act && !u_hosts) {
      const int host = w.col[e];
      if (host >= w.hub0) {
        atomicAdd(&hist[host - w.hub0], 1);
      } else if (!PLACE) {
        atomicAdd(&cnt[host], 1);
      } else {
        put(trp[host] + atomicAdd(&cnt[host], 1), host, e, ru, du, dv, tail, false);
      }
    }
  });
  __syncthreads();
  for (int h = threadIdx.x; h < kHubWin; h += 256) {
    const int c = hist[h];
    if (c) {
      const int b = atomicAdd(&cnt[w.hub0 + h], c);  // pass 1: the count; pass 2: this workgroup's range among the hub's tasks
      if (PLACE) hist[h] = b;  // (the ranks inside the range are taken from the same word)
    }
  }
  if (!PLACE) return;
  __syncthreads();
  task_walk(w, [&](const bool act, const int u, const int i, const int e, const int ru, const int du, const int2 dv, const int tail, const bool u_hosts) {
    if (act && !u_hosts) {
      const int host = w.col[e];
      if (host >= w.hub0) {
        const int h = host - w.hub0;
        put(trp[host] + atomicAdd(&hist[h], 1), host, e, ru, du, dv, tail, false);
      }
    }
  });
}

// ---- the key stream of the triangle count, built DIRECTLY (round 4: until then from the task lists above -- every task placed as a 13-byte
// record by scattered stores, three scans over the edges, the records read back to copy their keys: 7.9 of the 18 ms a first triangle count
// of R-MAT-22 took, 43 of 119 on R-MAT-24).  The same two walks with one packed counter per host -- keys of the short lists in the low
// 32 bits, tasks with longer lists in the high 32: pass 1 counts, two scans over the VERTICES give the hosts' offsets, pass 2 reserves a
// task's place with the same atomic and writes the keys (tagged with the host's low byte) or the {start, length} of a longer list where
// they stay.  A group of eight lanes copies the short lists of its eight tasks together, eight keys a step.  The order of a host's keys
// is the order of arrival: the kernel looks every key up on its own.
static bool keystream_possible(const gm_graph *g) {  // ids must leave bits 24..31 to the host tag
  return g->nv <= (1 << 24) && !gm_sweep_env("GM_TC_NO_KEY_STREAM");
}
struct KeyCopy { int src, dst, len, own; unsigned tag; };
// EDGES (the edge supports, gm_sup.hip): beside every key the DAG entry it was copied from and the entry of its task's own edge, beside
// every longer list the entry of its task's own edge -- read only where a key is found
struct KstEdges { int2 *kst_et; int *tedgel; };  // kst_et[k] = {entry of key k, entry of its task's own edge}
template <bool PLACE, int WIN, bool EDGES>
__global__ __launch_bounds__(256) void kst_rows_kernel(const TaskWalk w, const int lmax, unsigned long long *__restrict__ cnt /* PLACE: the cursors */,
                                                        const int *__restrict__ kst_rp, const int *__restrict__ trpl, unsigned *__restrict__ kst,
                                                        int2 *__restrict__ tdescl, const KstEdges ed) {
  __shared__ unsigned long long hist[WIN];
  const int hubwin = w.nv - w.hub0;  // (<= WIN: ensure_keystream)
  for (int h = threadIdx.x; h < hubwin; h += 256) hist[h] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane & 7, g8 = lane & ~7;
  // the list a task streams, and its weight in the packed counters
  auto task_list = [&](const bool act, const int e, const int ru, const int du, const int2 dv, const int tail, const bool u_hosts, int &start, int &len) {
    start = u_hosts ? dv.x : (w.topo ? e + 1 : ru);
    len = !act ? 0 : (u_hosts ? dv.y : (w.topo ? tail : du));
    return len == 0 ? 0ull : (len <= lmax ? (unsigned long long)len : (1ull << 32));
  };
  auto copy_group = [&](const KeyCopy c) {  // c.len = 0: nothing of this lane's
    for (int j = 0; j < 8; ++j) {
      const int lj = __shfl(c.len, g8 + j), sj = __shfl(c.src, g8 + j), dj = __shfl(c.dst, g8 + j);
      const unsigned tj = (unsigned)__shfl((int)c.tag, g8 + j);
      for (int i = sub; i < lj; i += 8) kst[dj + i] = (unsigned)w.col[sj + i] | tj;
      if (EDGES) {
        const int oj = __shfl(c.own, g8 + j);
        for (int i = sub; i < lj; i += 8) ed.kst_et[dj + i] = make_int2(sj + i, oj);
      }
    }
  };
  auto put = [&](const bool mine, const int host, const unsigned long long pos, const int start, const int len, const int e) {
    KeyCopy c{start, 0, 0, e, (unsigned)(host & 255) << 24};
    if (mine) {
      if (len > lmax) {
        const int slot = trpl[host] + (int)(pos >> 32);
        tdescl[slot] = make_int2(start, len);
        if (EDGES) ed.tedgel[slot] = e;
      } else {
        c.dst = kst_rp[host] + (int)(unsigned)pos;
        c.len = len;
      }
    }
    copy_group(c);
  };
  task_walk(w, [&](const bool act, const int u, const int i, const int e, const int ru, const int du, const int2 dv, const int tail, const bool u_hosts) {
    int start, len;
    const unsigned long long wgt = task_list(act, e, ru, du, dv, tail, u_hosts, start, len);
    // (i) the tasks the row hosts itself: one atomic per 8-lane group (an inclusive scan of the packed weights over the group)
    const unsigned long long mine = u_hosts ? wgt : 0ull;
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      const unsigned lo = (unsigned)__shfl((int)(unsigned)incl, lane - d), hi = (unsigned)__shfl((int)(unsigned)(incl >> 32), lane - d);
      if (sub >= d) incl += ((unsigned long long)hi << 32) | lo;
    }
    const unsigned long long total = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(incl >> 32), g8 + 7) << 32) | (unsigned)__shfl((int)(unsigned)incl, g8 + 7);
    unsigned long long ubase = 0ull;
    if (total != 0ull && sub == 0) ubase = atomicAdd(&cnt[u], total);
    // (ii) in-edge tasks: the target hosts -- a hub through the LDS histogram, anybody else through its global cursor
    int host = u;
    unsigned long long pos = 0ull;
    bool now = mine != 0ull;
    if (!u_hosts && wgt != 0ull) {
      host = w.col[e];
      if (host >= w.hub0) atomicAdd(&hist[host - w.hub0], wgt);
      else { pos = atomicAdd(&cnt[host], wgt); now = true; }
    }
    if (PLACE) {
      if (total != 0ull) {
        ubase = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(ubase >> 32), g8) << 32) | (unsigned)__shfl((int)(unsigned)ubase, g8);
        if (mine != 0ull) pos = ubase + incl - mine;
      }
      put(now, host, pos, start, len, e);
    }
  });
  __syncthreads();
  for (int h = threadIdx.x; h < hubwin; h += 256) {
    const unsigned long long c = hist[h];
    if (c) {
      const unsigned long long b = atomicAdd(&cnt[w.hub0 + h], c);  // pass 1: the count; pass 2: this workgroup's range among the hub's
      if (PLACE) hist[h] = b;
    }
  }
  if (!PLACE || w.hub0 >= w.nv) return;
  __syncthreads();
  task_walk(w, [&](const bool act, const int u, const int i, const int e, const int ru, const int du, const int2 dv, const int tail, const bool u_hosts) {
    int start, len;
    const unsigned long long wgt = task_list(act, e, ru, du, dv, tail, u_hosts, start, len);
    int host = 0;
    unsigned long long pos = 0ull;
    bool now = false;
    if (!u_hosts && wgt != 0ull) {
      host = w.col[e];
      if (host >= w.hub0) { pos = atomicAdd(&hist[host - w.hub0], wgt); now = true; }
    }
    put(now, host, pos, start, len, e);
  });
}
// the instances in use: the count pass (never with the entries), the place pass with / without them, each with the hub window that holds `win` hosts
static void launch_kst_rows(const bool place, const int win, const bool edges, const dim3 grid, const TaskWalk &w, const int lmax, unsigned long long *cnt,
                            const int *kst_rp, const int *trpl, unsigned *kst, int2 *tdescl, const KstEdges ed) {
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, 0, w, lmax, cnt, kst_rp, trpl, kst, tdescl, ed); };
  const bool half = win <= 2048;
  if (!place) half ? go(kst_rows_kernel<false, 2048, false>) : go(kst_rows_kernel<false, kHubWin, false>);
  else if (edges) half ? go(kst_rows_kernel<true, 2048, true>) : go(kst_rows_kernel<true, kHubWin, true>);
  else half ? go(kst_rows_kernel<true, 2048, false>) : go(kst_rows_kernel<true, kHubWin, false>);
}
__global__ __launch_bounds__(256) void kst_unpack_kernel(int nv, const unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ keys, int *__restrict__ longs) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v > nv) return;
  const unsigned long long c = v < nv ? cnt[v] : 0ull;
  keys[v] = c & 0xffffffffull;
  longs[v] = (int)(c >> 32);
}
__global__ __launch_bounds__(256) void kst_narrow_kernel(int nv, const unsigned long long *__restrict__ in, int *__restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v <= nv) out[v] = (int)in[v];
}

// the hub corner the triangle count takes on the matrix cores (gm_ctc.hip): its size on this handle -- the last h vertices, word-aligned in the
// core bitmap -- or 0.  The masked product costs h^3 / 6 bit-products whatever the corner holds, the streamed kernel ~rho^2 h^3 / 8 keys for
// a corner of density rho (|E| = rho h^2 / 2 edges, lists of rho h / 2 keys, half of a list streamed), so the corner pays from a density
// on: measured (profiles/r05/ab_tc_core.txt) R-MAT-22 at h = 8 K / 16 K / 32 K (11 / 4.5 / 2.0 %): 1.96 / 1.89 / 3.09 ms against 2.47
// without, R-MAT-24 at 16 K / 32 K (12.7 / 5.4 %): 26.1 / 24.5 against 32.2 -- the largest power-of-two fraction of the core bitmap whose
// density is >= kTcCoreMinDensity.  GM_TC_CORE_H = 0 switches the corner off, any other value forces that size (tests: small graphs).
constexpr double kTcCoreMinDensity = 0.03;
static int tc_core_size(gm_graph *g, const char *env = "GM_TC_CORE_H", bool blocks_only = false) {
  long long want = kTcCoreHDefault;
  bool forced = false;
  if (const char *e = gm_opt(env)) { want = atoll(e); forced = true; }
  if (want <= 0 || g->nv < 64) return 0;
  if (ensure_core_bitmap(g) != GM_OK || !g->core.built()) return 0;  // (not topologically numbered, no room: everything through the stream)
  const long long core_h = g->core->h;
  const long long cap = std::min<long long>(core_h, (long long)kCtcMaxH);
  auto aligned = [&](long long h) {  // the corner starts at a word of the bitmap's rows
    const long long off = (core_h - h + 31) / 32 * 32;
    return off >= core_h ? 0ll : core_h - off;
  };
  if (forced) {
    const long long h = aligned(std::min(want, cap));
    return (int)((blocks_only && h % 512 != 0) ? 0 : h);  // (the supports' corner runs on the block kernel only)
  }
  // a corner is worth its MFMA pass where the hubs are a small part of the graph: at most a quarter of the vertices, at least 1024 of them
  for (long long h = cap; h >= 1024; h >>= 1) {
    if ((long long)g->nv < 4 * h) continue;
    int e0 = 0;
    if (hipMemcpy(&e0, g->d_rp + (g->nv - h), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const double rho = (double)(g->ne - (long long)e0) / (0.5 * (double)h * (double)h);
    if (rho >= kTcCoreMinDensity && !(blocks_only && aligned(h) % 512 != 0)) return (int)aligned(h);
  }
  return 0;
}

// ---- the hub corner chosen per PAIR of 256-row blocks ------------------------------------------------------------------------------------
// The product takes the edges of a pair (IB <= JB) of 256-row blocks of a region at the end of the core bitmap for
// 65536 * (columns from JB's 512-column chunk to the region's end) bit-products whatever the pair holds; the stream takes them for the
// min(d+(v), tail_u(v)) keys of each.  Every triangle is counted by its (smallest, middle) edge, so ANY set of pairs is exact as long as the
// stream leaves out exactly the edges of the chosen ones: a pair is taken iff its keys * R > its bit-products.
// kTcPairR: the bit-products a streamed key is worth.  From profiles/r07/ab_tc_long_list.txt (R-MAT-22, full corner of 16 K): tch_kernel<1024>
// 1.436 ms for the 1.716 G keys outside the corner = 0.837 ps per key, core_tc_block_kernel<false> 0.247 ms for 16384^3 / 6 = 7.33e11
// bit-products = 0.337 fs each: 2480.  GM_TC_PAIR_R overrides (sweep: profiles/r09/ab_tc_corner_pairs.txt).
constexpr unsigned long long kTcPairR = 2480;
// the rule, on the host: keys[IB * nb + JB] = the stream's keys of the pair's edges; sets bit IB * nb + JB of bits[(nb * nb + 31) / 32] for
// every pair taken and returns their number (< 0: invalid arguments)
// (keys * R > cost  <=>  keys > floor(cost / R) for integers: no overflow whatever R)
__host__ __device__ inline bool tc_pair_pays(const unsigned keys, const int jb, const int region, const unsigned long long R) {
  const unsigned long long cost = 65536ull * (unsigned long long)(region - 512 * (jb >> 1));
  return R != 0ull && (unsigned long long)keys > cost / R;
}
extern "C" int gm_tc_pair_rule(const uint32_t *keys, int nb, int region, uint64_t R, uint32_t *bits) {
  if (!keys || !bits || nb < 1 || nb > 128 || region != nb * 256) return -1;
  const int nwords = (nb * nb + 31) / 32;
  for (int i = 0; i < nwords; ++i) bits[i] = 0u;
  int taken = 0;
  for (int ib = 0; ib < nb; ++ib)
    for (int jb = ib; jb < nb; ++jb)
      if (tc_pair_pays(keys[ib * nb + jb], jb, region, R)) {
        const int b = ib * nb + jb;
        bits[b >> 5] |= 1u << (b & 31);
        ++taken;
      }
  return taken;
}
// the cells of the rule: a workgroup per block of 256 rows, its row of cells in LDS -- per (IB, JB) the keys the stream would move for the
// pair's edges (the list a task streams, as kst_rows_kernel's task_list) and the edges themselves
constexpr int kPairMaxNb = kCtcMaxH / 256;
__global__ __launch_bounds__(1024) void tc_pair_cells_kernel(const TaskWalk w, const int region_from, const int nb, unsigned *__restrict__ keys,
                                                              unsigned *__restrict__ edges) {
  __shared__ unsigned ck[kPairMaxNb], ce[kPairMaxNb];
  for (int j = threadIdx.x; j < kPairMaxNb; j += blockDim.x) ck[j] = ce[j] = 0u;
  __syncthreads();
  const int ib = blockIdx.x;
  const long long r0 = (long long)region_from + 256ll * ib;
  task_walk_rows(w, r0 + ((threadIdx.x & ~63) >> 3), r0 + 256, (long long)(blockDim.x >> 3),
                 [&](const bool act, const int, const int, const int e, const int, const int, const int2 dv, const int tail, const bool u_hosts) {
                   if (!act) return;
                   const int jb = (w.col[e] - region_from) >> 8;  // (topological: ib <= jb < nb)
                   atomicAdd(&ck[jb], (unsigned)(u_hosts ? dv.y : tail));
                   atomicAdd(&ce[jb], 1u);
                 });
  __syncthreads();
  for (int j = threadIdx.x; j < nb; j += blockDim.x) {
    keys[ib * nb + j] = ck[j];
    edges[ib * nb + j] = ce[j];
  }
}
// the selection on the device (the host fetches 2 KB of bits and four sums instead of the cells: a copy of 128 KB into pageable memory
// cost 5 ms of the first call): kind 0 = the rule (tc_pair_pays, what gm_tc_pair_rule evaluates), 1 all, 2 none, 3 checker, 4 diag,
// 5 offdiag -- a pair without keys is never taken; sums = {taken, pairs with keys, edges taken, keys taken}; bits / sums zeroed before
__global__ __launch_bounds__(256) void tc_pair_select_kernel(const int nb, const int region, const unsigned long long R, const int kind,
                                                              const unsigned *__restrict__ keys, const unsigned *__restrict__ edges,
                                                              unsigned *__restrict__ bits, unsigned long long *__restrict__ sums) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb * nb) return;
  const int ib = b / nb, jb = b - ib * nb;
  const unsigned k = keys[b];
  if (ib > jb || k == 0u) return;
  atomicAdd(&sums[1], 1ull);
  const bool take = kind == 0 ? tc_pair_pays(k, jb, region, R)
                              : (kind == 1 || (kind == 3 && ((ib + jb) & 1)) || (kind == 4 && ib == jb) || (kind == 5 && ib < jb));
  if (!take) return;
  atomicOr(&bits[b >> 5], 1u << (b & 31));
  atomicAdd(&sums[0], 1ull);
  atomicAdd(&sums[2], (unsigned long long)edges[b]);
  atomicAdd(&sums[3], (unsigned long long)k);
}
// Decides the pairs of the key stream `ks` being built (under g->mu, before the stream's count pass): tc_h = the base corner of the density rule (0: none).
// Leaves ks.pair_region = 0 -- the full triangle of tc_h, as before -- when the corner is forced (GM_TC_CORE_H), switched off
// (GM_TC_PAIRS=off), there is no base corner and no forced region, or the region cannot run on the block kernel.
// GM_TC_PAIRS = rule | off | all | none | checker ((IB + JB) odd) | diag | offdiag (tests: the last five); GM_TC_PAIR_R = R of the rule;
// GM_TC_PAIR_REGION = rows of the region whatever the density rule says (tests: small graphs)
static int tc_pairs_setup(gm_graph *g, KeyStream &ks, const TaskWalk &tw, const int tc_h) {
  ks.pair_region = 0;
  const char *mode = gm_opt("GM_TC_PAIRS");
  if (!mode || !*mode) mode = "rule";
  const char *forced_region = gm_opt("GM_TC_PAIR_REGION");
  // (a misspelt option is an error on every graph, not only where a selection would have been made)
  const int kind = !strcmp(mode, "rule") ? 0 : !strcmp(mode, "all") ? 1 : !strcmp(mode, "none") ? 2 : !strcmp(mode, "checker") ? 3 : !strcmp(mode, "diag") ? 4 : !strcmp(mode, "offdiag") ? 5 : !strcmp(mode, "off") ? 6 : -1;
  if (kind < 0) return GM_ERR_INVALID;
  long long region_want = 0;
  if (forced_region) {
    char *end = nullptr;
    region_want = strtoll(forced_region, &end, 10);
    if (end == forced_region || *end != '\0' || region_want <= 0) return GM_ERR_INVALID;
  }
  if (const char *e = gm_opt("GM_TC_PAIR_R")) {
    char *end = nullptr;
    if (strtoll(e, &end, 10) < 0 || end == e || *end != '\0') return GM_ERR_INVALID;
  }
  if (kind == 6 || gm_opt("GM_TC_CORE_H") || (tc_h <= 0 && !forced_region)) return GM_OK;
  if (!g->core.built() || !tw.topo) return GM_OK;
  const int core_h = g->core->h;
  // the region: the largest multiple of 512 rows at the end of the core bitmap, at most a quarter of the vertices, starting where the block
  // kernel's 16-byte loads can (core_tc_fast_path)
  long long region = std::min<long long>(std::min<long long>(core_h, kCtcMaxH), (long long)g->nv / 4) / 512 * 512;
  if (forced_region) region = region_want;
  else while (region >= 512 && (core_h - region) % 128 != 0) region -= 512;
  if (region < 512 || region % 512 != 0 || region > core_h || region > kCtcMaxH || region < tc_h) return GM_OK;
  CoreTcParams cp;
  memset(&cp, 0, sizeof cp);
  cp.core = g->core->bits;
  cp.row_words = (core_h + 31) / 32;
  cp.row0 = core_h - (int)region;
  cp.word0 = cp.row0 >> 5;
  cp.h = (int)region;
  if (cp.row0 % 32 != 0 || !core_tc_fast_path(cp)) return GM_OK;
  unsigned long long R = kTcPairR;
  if (const char *e = gm_opt("GM_TC_PAIR_R")) R = (unsigned long long)std::max(0ll, atoll(e));
  const int nb = (int)region / 256, nc = (int)region / 512, region_from = g->nv - (int)region, ncell = nb * nb, nwords = (ncell + 31) / 32;
  DevBuf<unsigned> cells;
  DevBuf<unsigned long long> sel;  // four sums, then the bits
  HIP_TRY(cells.alloc((size_t)ncell * 2));
  HIP_TRY(sel.alloc(4 + (size_t)(nwords + 1) / 2));
  HIP_TRY(hipMemsetAsync(sel.p, 0, 8 * (4 + (size_t)(nwords + 1) / 2), 0));
  hipLaunchKernelGGL(tc_pair_cells_kernel, dim3((unsigned)nb), dim3(1024), 0, 0, tw, region_from, nb, cells.p, cells.p + ncell);
  hipLaunchKernelGGL(tc_pair_select_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, 0, nb, (int)region, R, kind, (const unsigned *)cells.p,
                     (const unsigned *)(cells.p + ncell), reinterpret_cast<unsigned *>(sel.p + 4), sel.p);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> h_sel(4 + (size_t)(nwords + 1) / 2, 0ull);
  HIP_TRY(hipMemcpy(h_sel.data(), sel.p, 8 * h_sel.size(), hipMemcpyDeviceToHost));
  const unsigned *bits = reinterpret_cast<const unsigned *>(h_sel.data() + 4);
  setup_trace("key stream: cells and choice of the block pairs");
  // the product's tasks: the non-empty pieces (16 chunks from JB's on) of the chosen pairs, the longest first
  std::vector<unsigned> tasks;
  const long long taken = (long long)h_sel[0], possible = (long long)h_sel[1], p_edges = (long long)h_sel[2], p_keys = (long long)h_sel[3];
  for (int ib = 0; ib < nb; ++ib)
    for (int jb = ib; jb < nb; ++jb) {
      const int b = ib * nb + jb;
      if (!((bits[b >> 5] >> (b & 31)) & 1u)) continue;
      for (int piece = 0, cb = jb >> 1; cb < nc; ++piece, cb += kCtcBPiece) tasks.push_back(ctc_pack_task(ib, jb, piece));
    }
  auto chunks_of = [&](const unsigned t) {
    const int cb = (int)((t >> 8) & 255u) / 2 + (int)(t >> 16) * kCtcBPiece;
    return std::min(cb + kCtcBPiece, nc) - cb;
  };
  std::stable_sort(tasks.begin(), tasks.end(), [&](const unsigned a, const unsigned b) { return chunks_of(a) > chunks_of(b); });
  HIP_TRY(ks.pair_bits.alloc(sizeof(unsigned) * (size_t)nwords));
  HIP_TRY(ks.pair_tasks.alloc(sizeof(unsigned) * std::max<size_t>(tasks.size(), 1)));
  HIP_TRY(hipMemcpy(ks.pair_bits, bits, sizeof(unsigned) * (size_t)nwords, hipMemcpyHostToDevice));
  if (!tasks.empty()) HIP_TRY(hipMemcpy(ks.pair_tasks, tasks.data(), sizeof(unsigned) * tasks.size(), hipMemcpyHostToDevice));
  ks.n_pair_tasks = (int)tasks.size();
  ks.pair_from = region_from;
  const long long info[6] = {region, taken, possible, p_edges, p_keys, (long long)R};
  for (int i = 0; i < 6; ++i) ks.pair_info[i] = info[i];
  ks.pair_region = (int)region;
  setup_trace("key stream: tasks of the product, uploads");
  return GM_OK;
}

// One build of the key stream.  first == nullptr: the FIRST set into `ks` -- offsets, stream, longer lists, with the entries when `edges`,
// with the hub corner / the block pairs when allow_core.  Else only the place pass over the offsets of *first, into the second set `ke`.
// kOnceBuilt, kOnceNotApplicable (first set: this handle cannot have a stream) or an error code.  Under g->mu; `topo` from the caller.
static int build_keystream(gm_graph *g, const bool edges, const bool allow_core, const int tc_h, bool topo, const KeyStream *first, KeyStream &ks, KeyEntries &ke) {
  const bool second = first != nullptr;  // the offsets exist: only the place pass, into the second set
  int lmax = second ? first->lmax : GM_TC_INLINE_MAX_DEFAULT;
  if (!second) {
    if (const char *e = gm_sweep_env("GM_TC_INLINE_MAX")) lmax = atoi(e);  // (sweeps)
    if (!keystream_possible(g) || lmax < 4) return kOnceNotApplicable;
  }
  SetupTimer timer;
  HIP_TRY(hipSetDevice(g->device));
  const size_t nv1 = (size_t)g->nv + 1;
  PoolScope pool(g);
  ScanTemp tmp;
  if (gm_sweep_env("GM_TC_NO_TRIM")) topo = false;  // (A/B: whole lists streamed on a topologically numbered DAG too)
  DevBuf<unsigned long long> cnt, keys, keyoff;
  DevBuf<int> longs;
  HIP_TRY(cnt.alloc(nv1));
  HIP_TRY(keys.alloc(nv1));
  HIP_TRY(keyoff.alloc(nv1));
  HIP_TRY(longs.alloc(nv1));
  // (few, fat workgroups where a hub window exists: a workgroup's LDS histogram of the hub hosts pays when it sees many rows)
  // The two passes choose their windows independently (a window only says which hosts are aggregated in LDS): the count pass is all
  // atomics and wants the larger one, the place pass waits for its returning atomics and the lists it copies and wants more workgroups
  // per CU.  Measured, window / workgroups per CU, count + place ms: R-MAT-22 4096 / 8: 1.38 + 2.51, 2048 / 16: 1.43 + 2.16;
  // R-MAT-24 4096 / 8: 8.5 + 14.7, 2048 / 16: 10.1 + 13.6.
  int win_count = kHubWin, win_place = 2048, per_cu_count = topo ? 8 : 64, per_cu_place = topo ? 16 : 64;
  if (const char *e = gm_sweep_env("GM_KST_HUB_WIN")) win_count = win_place = std::max(0, std::min(atoi(e), kHubWin));  // (sweeps)
  if (const char *e = gm_sweep_env("GM_KST_WG_PER_CU")) per_cu_count = per_cu_place = std::max(1, atoi(e));
  TaskWalk tw = task_walk_of(g, topo, win_count);  // (the count pass's; the place pass's differs in its window, below)
  int skip_from = (!second && topo && tc_h > 0) ? g->nv - tc_h : 0x7fffffff;
  if (!second && allow_core && !edges) {  // the corner per pair of blocks: the stream leaves out the chosen pairs' edges instead of whole rows
    if (const int rc = tc_pairs_setup(g, ks, tw, skip_from < g->nv ? tc_h : 0)) return rc;
    if (ks.pair_region > 0) {
      tw.region_from = ks.pair_from;
      tw.pair_nb = ks.pair_region / 256;
      tw.pair_bits = ks.pair_bits;
      if (skip_from >= g->nv) skip_from = ks.pair_from;  // (a forced region on a graph without a base corner: gm_tc_core_info names the region)
    }
  }
  tw.skip_from = ks.pair_region > 0 ? 0x7fffffff : skip_from;
  long long core_edges = 0;
  if (skip_from < g->nv) {
    int e0 = 0;
    HIP_TRY(hipMemcpy(&e0, g->d_rp + skip_from, sizeof(int), hipMemcpyDeviceToHost));
    core_edges = g->ne - (long long)e0;
  }
  TaskWalk tw_place = tw;
  tw_place.hub0 = task_walk_of(g, topo, win_place).hub0;
  DevOwn<int> krp_new, trpl_new, tedgel;  // (what this call builds: moved into ks / ke at the end, given back on every other return)
  DevOwn<unsigned> kst;
  DevOwn<int2> tdl, kst_et;
  if (!second) HIP_TRY(krp_new.alloc(sizeof(int) * nv1));
  if (!second) HIP_TRY(trpl_new.alloc(sizeof(int) * nv1));
  int *const krp = second ? first->rp.get() : krp_new.get(), *const trpl = second ? first->trpl.get() : trpl_new.get();
  unsigned long long total = second ? first->n_keys : 0, key_limit = 0x7fffff00ull;
  if (const char *e = gm_opt("GM_KST_MAX_KEYS")) key_limit = std::min<unsigned long long>(key_limit, (unsigned long long)std::max(1ll, atoll(e)));  // (tests)
  int nlong = second ? first->n_long_tasks : 0;
  while (!second) {  // the stream is indexed with 32 bits: halve the limit of a "short" list until it fits
    HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * nv1, 0));
    launch_kst_rows(false, win_count, false, row_walk_grid(g, per_cu_count), tw, lmax, cnt.p, nullptr, nullptr, nullptr, nullptr, KstEdges{nullptr, nullptr});
    hipLaunchKernelGGL(kst_unpack_kernel, grid_1d((long long)nv1), dim3(256), 0, 0, g->nv, cnt.p, keys.p, longs.p);
    HIP_TRY(dev_scan_total(tmp, keys.p, keyoff.p, (size_t)g->nv, &total));
    HIP_TRY(dev_scan_total(tmp, longs.p, trpl, (size_t)g->nv, &nlong));
    if (total < key_limit) break;
    lmax >>= 1;
    if (lmax < 4) {
      ks = KeyStream();
      return kOnceNotApplicable;
    }
  }
  setup_trace("key stream: count pass + scans");
  if (!second) hipLaunchKernelGGL(kst_narrow_kernel, grid_1d((long long)nv1), dim3(256), 0, 0, g->nv, keyoff.p, krp);
  const size_t nk = (size_t)std::max<unsigned long long>(total, 1), nl = (size_t)std::max(nlong, 1);
  HIP_TRY(kst.alloc(sizeof(unsigned) * nk));
  HIP_TRY(tdl.alloc(sizeof(int2) * nl));
  if (edges) HIP_TRY(kst_et.alloc(sizeof(int2) * nk));
  if (edges) HIP_TRY(tedgel.alloc(sizeof(int) * nl));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * nv1, 0));
  launch_kst_rows(true, win_place, edges, row_walk_grid(g, per_cu_place), tw_place, lmax, cnt.p, krp, trpl, kst.get(), tdl.get(), KstEdges{kst_et, tedgel});
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  setup_trace("key stream: place pass");
  if (second) {  // (the first set stays what the triangle count reads)
    ke.kst2 = std::move(kst);
    ke.tdescl2 = std::move(tdl);
    ke.tedgel = std::move(tedgel);
    ke.kst_et = std::move(kst_et);
  } else {
    ks.kst = std::move(kst);
    ks.rp = std::move(krp_new);
    ks.trpl = std::move(trpl_new);
    ks.tdescl = std::move(tdl);
    ks.n_keys = total;
    ks.n_long_tasks = nlong;
    ks.lmax = lmax;
    if (skip_from < g->nv) {
      ks.core_edges = core_edges;
      ks.core_h = g->nv - skip_from;
      ks.skip_from = skip_from;
    }
    if (edges) {
      ks.tedgel = std::move(tedgel);
      ks.kst_et = std::move(kst_et);
    }
  }
  g->setup.table_ms += timer.ms();
  return kOnceBuilt;
}

// the KeyStream of a handle (gm_host.h): GM_OK also when the handle cannot have one (ids beyond 24 bits, keys beyond the 32-bit index space
// at every list limit) -- *built says which.  edges: with the entries the edge supports need: a handle whose stream was built without them
// gets a SECOND set of keys / longer lists with them (KeyEntries) -- same offsets (the counts per host do not depend on the order of
// arrival), its own order
int ensure_keystream(gm_graph *g, bool edges, bool *built, bool allow_core) {
  auto have = [&]() { return g->kst.built() && (!edges || g->kst->kst_et != nullptr || g->kst_entries.built()); };
  *built = have();
  if (*built || g->ne == 0 || (g->kst.known() && !g->kst.built())) return GM_OK;
  // (a stream without the hub corner's rows cannot carry the edge supports: they take the task lists)
  if (edges && g->kst.built() && g->kst->skip_from < g->nv) return GM_OK;
  {
    const int rc = ensure_edesc(g);  // (takes the lock itself)
    if (rc) return rc;
  }
  bool topo = false;
  {
    const int rc = graph_is_topological(g, &topo);  // (takes the lock itself)
    if (rc) return rc;
  }
  if (!g->kst.known()) {
    const int tc_h = (allow_core && !edges) ? tc_core_size(g) : 0;  // (takes the lock itself)
    KeyEntries none;
    const int rc = g->kst.ensure(g->mu, [&](KeyStream &ks) { return build_keystream(g, edges, allow_core, tc_h, topo, nullptr, ks, none); });
    if (rc) return rc;
  }
  if (edges && g->kst.built() && g->kst->kst_et == nullptr && g->kst->skip_from >= g->nv) {  // built without the entries: the second set
    KeyStream none;
    const int rc = g->kst_entries.ensure(g->mu, [&](KeyEntries &ke) { return build_keystream(g, true, false, 0, topo, &*g->kst, none, ke); });
    if (rc) return rc;
  }
  *built = have();
  return GM_OK;
}

int ensure_tasklists(gm_graph *g) {
  // The tasks' own entries (tedge, 4 B per edge: what the edge supports need) are always built with the lists.  Round 3 built them on
  // demand by freeing and rebuilding trp / tdesc -- under a launch of another thread that had already copied those pointers.
  if (g->tasklists.known() || g->ne == 0) return GM_OK;
  {
    const int rc = ensure_edesc(g);  // (takes the lock itself)
    if (rc) return rc;
  }
  // the hub corner (gm_ctc.hip): its edges' supports / triangles come from the matrix cores -- where every row fits the stage (the rows beyond
  // it are the chunked kernel's, run_pattern) and the corner is a whole number of 512-vertex chunks
  const int tl_h = g->max_deg <= kTctStageMax ? tc_core_size(g, "GM_SUP_CORE_H", true) : 0;  // (takes the lock itself)
  bool topo = false;
  {
    const int rc = graph_is_topological(g, &topo);  // (takes the lock itself)
    if (rc) return rc;
    if (gm_sweep_env("GM_TC_NO_TRIM")) topo = false;  // (A/B: whole lists streamed on a topologically numbered DAG too)
  }
  // (the lists, the corner's skip row and the inline copies reach a first caller on another thread together: ADVICE r5)
  return g->tasklists.ensure(g->mu, [&](TaskLists &tl) {
    SetupTimer timer;
    HIP_TRY(hipSetDevice(g->device));
    const size_t ne = (size_t)g->ne, nv1 = (size_t)g->nv + 1;
    PoolScope pool(g);
    DevBuf<int> cnt;
    ScanTemp tmp;
    setup_trace("tasks: sorted / topological check");
    HIP_TRY(cnt.alloc(nv1));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(int) * nv1, 0));
    // (few, fat workgroups: a workgroup's LDS histogram of the hub hosts pays when it sees many rows)
    // (where no hub window exists -- a DAG that is not numbered topologically -- many thin workgroups: power-law LJ-size 30.9 vs 9.8 ms)
    TaskWalk tw = task_walk_of(g, topo, kHubWin);
    const int tl_skip = (topo && tl_h > 0) ? g->nv - tl_h : 0x7fffffff;
    tw.skip_from = tl_skip;
    hipLaunchKernelGGL((task_rows_kernel<false>), row_walk_grid(g, topo ? 8 : 64), dim3(256), 0, 0, tw, cnt.p, nullptr, nullptr, nullptr);
    setup_trace("tasks: count pass");
    HIP_TRY(tl.trp.alloc(sizeof(int) * nv1));
    HIP_TRY(dev_exclusive_sum(tmp, cnt.p, tl.trp.get(), nv1));
    HIP_TRY(tl.tdesc.alloc(sizeof(int2) * ne));
    HIP_TRY(tl.tedge.alloc(sizeof(int) * ne));
    HIP_TRY(hipMemsetAsync(tl.tdesc, 0, sizeof(int2) * ne, 0));  // (the edges of rows beyond the stage are no tasks: empty descriptors at the end)
    HIP_TRY(hipMemsetAsync(tl.tedge, 0, sizeof(int) * ne, 0));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(int) * nv1, 0));
    setup_trace("tasks: scan, allocations, clears");
    hipLaunchKernelGGL((task_rows_kernel<true>), row_walk_grid(g, topo ? 16 : 64), dim3(256), 0, 0, tw, cnt.p, tl.trp.get(), tl.tdesc.get(), tl.tedge.get());  // (the place pass waits for its returning atomics)
    HIP_TRY(hipDeviceSynchronize());
    if (tl_skip < g->nv) {
      tl.skip_from = tl_skip;
      tl.core_h = g->nv - tl_skip;
    }
    setup_trace("tasks: place pass");
    // (a handle that cannot have the key stream: task-major copies of the short lists -- an optimisation that may fail: the handle goes without)
    const HipFailureMark mark;
    if (!keystream_possible(g) && build_inline_copies(g, tl, tmp) != GM_OK) mark.drop();
    setup_trace("tasks: inline copies");
    g->setup.table_ms += timer.ms();
    return kOnceBuilt;
  });
}

// ---- MATCH MASKS of the edge supports (gm_sup.hip, round 5).  An IN-EDGE task -- the target v = s_i of u -> v hosts, the tail
// N+(u)[i + 1 ..) is streamed -- finds triangles (u, s_i, s_j) whose "streamed" edge (u, s_j) is an entry of row u BEHIND the task's own
// entry: instead of one memory-side atomic per match the task stores WHICH keys matched -- bit k of its mask = the k-th key of the tail --
// with plain stores, and a second pass sums the masks of a row by column.  87 % of the triangles of an R-MAT graph are found by in-edge
// tasks, two thirds of them by tasks with tails of >= 32 keys.  Here: the size of every entry's mask (64-bit words; 0 = no mask: an
// out-edge task, a tail below `lmin`, a row beyond the stage), their offsets by one scan, and the offsets again in task order.
__global__ __launch_bounds__(256) void sup_mask_size_kernel(const TaskWalk w, const int lmin, unsigned long long *__restrict__ sz) {
  task_walk(w, [&](const bool act, const int, const int, const int e, const int, const int, const int2, const int tail, const bool u_hosts) {
    // (a LONG list -- streamed one task at a time, gm_hset.h -- looks all the tiles of its last group up: kSupTiles - 1 spare words)
    if (act && !u_hosts && tail >= lmin) sz[e] = (unsigned long long)(((tail + 63) >> 6) + (tail >= kLongList ? kSupMaskSpare : 0));
  });
}
__global__ __launch_bounds__(256) void sup_mask_off_kernel(const long long ne, const unsigned long long *__restrict__ off, unsigned *__restrict__ emoff) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (long long)gridDim.x * blockDim.x)
    emoff[e] = off[e + 1] != off[e] ? (unsigned)off[e] : kNoMask;
}
__global__ __launch_bounds__(256) void sup_mask_task_kernel(const long long nt, const int2 *__restrict__ tdesc, const int *__restrict__ tedge,
                                                            const unsigned *__restrict__ emoff, unsigned *__restrict__ tmoff) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += (long long)gridDim.x * blockDim.x) {
    const int2 d = tdesc[t];
    const int e = tedge[t];
    // (an in-edge task streams the entries right behind its own: start == own entry + 1; an out-edge task of the same entry has no mask)
    tmoff[t] = (d.y > 0 && d.x == e + 1) ? emoff[e] : kNoMask;
  }
}

// the rows with tails of more than 64 keys (a second mask word: sup_far_kernel), widest ids first: flag, scan, scatter
__global__ __launch_bounds__(256) void sup_far_flag_kernel(const int nv, const int *__restrict__ rp, const int lmin, const int stage_max, const int skip_from,
                                                           int *__restrict__ flag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;  // position k = vertex nv - 1 - k
  if (k >= nv) return;
  const int v = nv - 1 - k, d = rp[v + 1] - rp[v];
  flag[k] = (v < skip_from && d <= stage_max && d - 1 > GM_WAVE && d - 1 >= lmin) ? 1 : 0;
}
__global__ __launch_bounds__(256) void sup_far_list_kernel(const int nv, const int *__restrict__ flag, const int *__restrict__ pos, int *__restrict__ rows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nv && flag[k]) rows[pos[k]] = nv - 1 - k;
}

// SupCorner: the symmetric bit matrix of the hub corner the task lists leave out, and the positions the supports' epilogue needs
int ensure_sup_corner(gm_graph *g) {
  const TaskLists &tl = *g->tasklists;
  if (tl.skip_from >= g->nv) return GM_OK;
  return g->sup_corner.ensure(g->mu, [&](SupCorner &sc) {
    SetupTimer timer;
    HIP_TRY(hipSetDevice(g->device));
    const int h = tl.core_h, words = h / 32;
    const size_t cells = (size_t)h * (size_t)words;
    HIP_TRY(sc.csym.alloc(cells * sizeof(unsigned)));
    HIP_TRY(sc.cfirst.alloc(cells * sizeof(unsigned short)));
    HIP_TRY(hipMemsetAsync(sc.csym, 0, cells * sizeof(unsigned), 0));
    HIP_TRY(hipMemsetAsync(sc.cfirst, 0, cells * sizeof(unsigned short), 0));
    int e0 = 0;
    HIP_TRY(hipMemcpy(&e0, g->d_rp + tl.skip_from, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(launch_core_sym_fill(g->nv, tl.skip_from, words, (long long)e0, g->ne, g->d_rp, g->d_col, sc.csym, sc.cfirst, g->cu_count, 0));
    HIP_TRY(hipDeviceSynchronize());
    setup_trace("supports: symmetric corner");
    g->setup.table_ms += timer.ms();
    return kOnceBuilt;
  });
}

// the shortest tail that gets a mask on this handle: kSupMaskMinTail, or the option GM_SUP_MASK_MIN as it stood when the handle's masks
// were laid out (ensure_sup_masks) -- the kernels must use the value the offsets were built with
int sup_mask_min_tail(const gm_graph *g) { return g->sup_masks->min_tail > 0 ? g->sup_masks->min_tail : kSupMaskMinTail; }

// the masks of a handle whose mask words were sized and scanned (off[e] .. off[e + 1]: the words of entry e, `total` of them): the rows with
// a second mask word, the offsets per entry and per task, the cleared arena
static int build_sup_masks(gm_graph *g, const TaskLists &tl, SupMasks &sm, const int lmin, const unsigned long long *off, const unsigned long long total, ScanTemp &tmp) {
  const size_t ne = (size_t)g->ne;
  // the rows that have a second mask word, from the top of the id range
  DevBuf<int> fflag, fpos;
  HIP_TRY(fflag.alloc((size_t)g->nv + 1));
  HIP_TRY(fpos.alloc((size_t)g->nv + 1));
  HIP_TRY(hipMemsetAsync(fflag.p, 0, sizeof(int) * ((size_t)g->nv + 1), 0));
  hipLaunchKernelGGL(sup_far_flag_kernel, dim3((unsigned)((g->nv + 255) / 256)), dim3(256), 0, 0, g->nv, g->d_rp, lmin, kTctStageMax, tl.skip_from, fflag.p);
  int nfar = 0;
  HIP_TRY(dev_scan_total(tmp, fflag.p, fpos.p, (size_t)g->nv, &nfar));
  HIP_TRY(sm.emoff.alloc(sizeof(unsigned) * ne));
  HIP_TRY(sm.far_rows.alloc(sizeof(int) * (size_t)std::max(nfar, 1)));
  hipLaunchKernelGGL(sup_far_list_kernel, dim3((unsigned)((g->nv + 255) / 256)), dim3(256), 0, 0, g->nv, fflag.p, fpos.p, sm.far_rows.get());
  HIP_TRY(sm.tmoff.alloc(sizeof(unsigned) * ne));
  HIP_TRY(sm.smask.alloc(sizeof(unsigned long long) * (size_t)total));
  // (every launch rewrites the words of the tasks it runs; a launch that leaves masked tasks out -- a chunk filter, an aborted launch --
  // must find zeros, not what hipMalloc handed over: ADVICE r5)
  HIP_TRY(hipMemsetAsync(sm.smask, 0, sizeof(unsigned long long) * (size_t)total, 0));
  const long long eb = std::min<long long>(((long long)ne + 255) / 256, (long long)g->cu_count * 32);
  hipLaunchKernelGGL(sup_mask_off_kernel, dim3((unsigned)eb), dim3(256), 0, 0, (long long)ne, off, sm.emoff.get());
  hipLaunchKernelGGL(sup_mask_task_kernel, dim3((unsigned)eb), dim3(256), 0, 0, (long long)ne, tl.tdesc.get(), tl.tedge.get(), sm.emoff.get(), sm.tmoff.get());
  HIP_TRY(hipDeviceSynchronize());
  sm.n_far_rows = nfar;
  sm.words = total;
  return GM_OK;
}

int ensure_sup_masks(gm_graph *g) {
  if (g->sup_masks.known()) return GM_OK;
  const TaskLists &tl = *g->tasklists;
  if (!tl.tdesc || !tl.tedge || !*g->edesc) return GM_ERR_INVALID;  // (after ensure_tasklists)
  bool topo = false;
  {
    const int rc = graph_is_topological(g, &topo);  // (takes the lock itself)
    if (rc) return rc;
  }
  return g->sup_masks.ensure(g->mu, [&](SupMasks &sm) {
    if (!topo || gm_sweep_env("GM_TC_NO_TRIM") || gm_opt("GM_SUP_NO_MASKS") || g->ne < 1) return kOnceNotApplicable;  // (tails exist on a topologically numbered DAG only)
    if (const char *e = gm_opt("GM_SUP_MASK_MIN")) sm.min_tail = std::max(1, atoi(e));
    const int lmin = sm.min_tail > 0 ? sm.min_tail : kSupMaskMinTail;
    SetupTimer timer;
    HIP_TRY(hipSetDevice(g->device));
    const size_t ne = (size_t)g->ne;
    PoolScope pool(g);
    DevBuf<unsigned long long> off;
    ScanTemp tmp;
    HIP_TRY(off.alloc(ne + 1));
    HIP_TRY(hipMemsetAsync(off.p, 0, sizeof(unsigned long long) * (ne + 1), 0));
    TaskWalk tw = task_walk_of(g, true, 0);  // (no hub window: the pass aggregates nothing)
    tw.skip_from = tl.skip_from;  // (the corner's rows have no tasks: no masks)
    hipLaunchKernelGGL(sup_mask_size_kernel, row_walk_grid(g, 32), dim3(256), 0, 0, tw, lmin, off.p);
    unsigned long long total = 0;
    HIP_TRY(dev_scan_total(tmp, off.p, off.p, ne, &total));
    setup_trace("support masks: sizes + scan");
    if (total == 0 || total >= (unsigned long long)kNoMask) {
      g->setup.table_ms += timer.ms();
      return kOnceNotApplicable;
    }
    const HipFailureMark mark;
    if (build_sup_masks(g, tl, sm, lmin, off.p, total, tmp) != GM_OK) {  // (an optimisation that did not fit: the atomics stay)
      mark.drop();
      const int min_tail = sm.min_tail;
      sm = SupMasks();
      sm.min_tail = min_tail;
      g->setup.table_ms += timer.ms();
      return kOnceNotApplicable;
    }
    setup_trace("support masks: offsets");
    g->setup.table_ms += timer.ms();
    return kOnceBuilt;
  });
}

// the rows beyond the stage of the task-list kernels: a handful per graph, found on the host copy of the offsets
int ensure_long_rows(gm_graph *g) {
  if (g->long_rows.known()) return GM_OK;
  const std::vector<int> *rp = nullptr;
  int rc = host_rp(g, &rp);  // (takes the lock itself)
  if (rc) return rc;
  return g->long_rows.ensure(g->mu, [&](LongRows &lr) {
    std::vector<int> rows;
    std::vector<long long> prefix(1, 0);
    for (int v = 0; v < g->nv; ++v) {
      const int d = (*rp)[(size_t)v + 1] - (*rp)[(size_t)v];
      if (d > kTctStageMax) {
        rows.push_back(v);
        prefix.push_back(prefix.back() + d);
      }
    }
    if (!rows.empty()) {
      HIP_TRY(hipSetDevice(g->device));
      HIP_TRY(lr.rows.alloc(sizeof(int) * rows.size()));
      HIP_TRY(lr.prefix.alloc(sizeof(long long) * prefix.size()));
      HIP_TRY(copy_to_device(lr.rows, rows.data(), sizeof(int) * rows.size()));
      HIP_TRY(copy_to_device(lr.prefix, prefix.data(), sizeof(long long) * prefix.size()));
    }
    lr.edges = prefix.back();
    lr.n = (int)rows.size();
    return kOnceBuilt;
  });
}

int ensure_edesc(gm_graph *g) {
  if (g->ne == 0) return GM_OK;
  return g->edesc.ensure(g->mu, [&](DevOwn<int2> &d) {
    SetupTimer timer;
    HIP_TRY(d.alloc(sizeof(int2) * (size_t)g->ne));
    const long long nblocks = std::min<long long>((g->ne + 255) / 256, (long long)g->cu_count * 32);
    hipLaunchKernelGGL(edesc_kernel, dim3((unsigned)nblocks), dim3(256), 0, 0, g->ne, g->d_rp, g->d_col, d.get());
    HIP_TRY(hipDeviceSynchronize());
    setup_trace("edge descriptors");
    g->setup.table_ms += timer.ms();
    return kOnceBuilt;
  });
}

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_tasks_kernel() {}
void gm_touch_tasks() { hipLaunchKernelGGL(gm_touch_tasks_kernel, dim3(1), dim3(1), 0, 0); }
