// gm_clique_plan.hip -- k-clique (k = 4): the plan of one rank's share for the re-hosted first level (gm_mine.h, gm_cbuild.hip) with what it
// is built from: the wide vertices, the core bitmap and its blocks, the rounds and their gather index. Everything below runs on
// the device except what is O(wide vertices of the share) or O(chunks).
#include "gm_host.h"
#include "gm_scan.h"
using namespace gm;

#ifndef GM_WIDE_ARENA_MB
#define GM_WIDE_ARENA_MB 16384
#endif
// the vertices of the two-phase path (dev_select_by_degree)
struct WideRow {
  int min_words;
  __device__ bool operator()(int d) const { return clique_is_wide(d, min_words); }
};
// this rank's share of the sorted wide list: slot i = entry first + i * step
__global__ __launch_bounds__(256) void wide_share_kernel(int count, long long first, long long step, const int *__restrict__ wide_sorted,
                                                         const int *__restrict__ rp, int *__restrict__ verts, int *__restrict__ degs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int u = wide_sorted[first + (long long)i * step];
  verts[i] = u;
  degs[i] = rp[u + 1] - rp[u];
}
__device__ __forceinline__ unsigned long long cb_matrix_words(int d) {
  return (d >= kCbMinDeg && d <= kCbMaxDeg) ? (unsigned long long)d * (unsigned long long)((d + 31) / 32) : 0ull;
}
// words of the matrices of every narrow chunk of the share (position i of the share = chunk order[first + i * step])
__global__ __launch_bounds__(256) void cb_chunk_words_kernel(long long count, long long first, long long step, const int *__restrict__ order,
                                                             const ChunkRec *__restrict__ chunks, const int *__restrict__ rp,
                                                             unsigned long long *__restrict__ words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const long long pos = first + i * step;
  const ChunkRec r = chunks[order ? order[pos] : pos];
  unsigned long long w = 0;
  for (int u = r.u_begin; u < r.u_end; ++u) w += cb_matrix_words(rp[u + 1] - rp[u]);
  words[i] = w;
}
// owners of a round: the vertices of its narrow chunks ...
__global__ __launch_bounds__(256) void cb_own_chunks_kernel(long long count, long long first, long long step, const int *__restrict__ order,
                                                            const ChunkRec *__restrict__ chunks, int *__restrict__ own) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const long long pos = first + i * step;
  const ChunkRec r = chunks[order ? order[pos] : pos];
  for (int u = r.u_begin; u < r.u_end; ++u) own[u] = 1;
}
// ... and its wide vertices
__global__ __launch_bounds__(256) void cb_own_verts_kernel(int count, const int *__restrict__ verts, int *__restrict__ own) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) own[verts[i]] = 2;  // (2: a wide vertex -- its rows with a first endpoint in the core are gathered, cb_owner_sizes_kernel)
}
// per vertex: matrix words and task edges of an owner (0 for everybody else; [nv] = 0 so that the scans end with the totals)
// core_base >= 0: a wide owner's rows whose first endpoint is >= core_base come from the core bitmap (gm_cgather.hip): only the
// entries below it -- the first ones of the ascending row -- are tasks of the streamed build
__global__ __launch_bounds__(256) void cb_owner_sizes_kernel(int nv, const int *__restrict__ rp, const int *__restrict__ col, const int *__restrict__ own,
                                                             int core_base, unsigned long long *__restrict__ words, int *__restrict__ tasks) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v > nv) return;
  unsigned long long w = 0;
  int t = 0;
  if (v < nv && own[v]) {
    const int d = rp[v + 1] - rp[v];
    w = cb_matrix_words(d);
    t = w ? d : 0;
    if (t && own[v] == 2 && core_base >= 0) t = lower_bound(col + rp[v], d, core_base);
  }
  words[v] = w;
  tasks[v] = t;
}
// The task records of a round by counting placement (like ensure_tasklists: until round 4 one (host, entry) key per task found by a
// bisection per entry, a radix sort of 109 M key / owner pairs on the com-Orkut stand-in, a record pass).  Eight lanes walk the row of an
// owner u: the first ntask_of[u] entries are its streamed tasks (all of them, or -- a wide vertex beside a core bitmap -- those below the
// core).  The edge u -> v is hosted by the endpoint whose list is NOT streamed: N+(v) whole, or N+(u) -- beyond v under a topological
// numbering -- whichever is shorter (round 3 compared the whole lists: 15 % more keys on R-MAT), when it fits the stage.
// (same-address atomics aggregated like task_rows_kernel's: per 8-lane group for the tasks a row hosts itself, per workgroup in an LDS
// histogram for the in-edge tasks of the last kHubWin hosts of a topologically numbered DAG)
template <bool PLACE>
__global__ __launch_bounds__(256) void cb_task_rows_kernel(int nv, const int *__restrict__ rp, const int *__restrict__ col, const int2 *__restrict__ edesc,
                                                           const int *__restrict__ ntask_of, int topo, int hub0, int *__restrict__ cnt /* PLACE: the cursors */,
                                                           const int *__restrict__ trp, const unsigned long long *__restrict__ base,
                                                           CBuildTask *__restrict__ out) {
  __shared__ int hist[kHubWin];
  for (int h = threadIdx.x; h < kHubWin; h += 256) hist[h] = 0;
  __syncthreads();
  const long long stride = ((long long)gridDim.x * blockDim.x) >> 3;
  const int lane = threadIdx.x & 63, sub = lane & 7, g8 = lane & ~7;
  const long long u0 = ((long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63)) >> 3;
  auto put = [&](const int slot, const int u, const int i, const int ru, const int du, const int2 dv, const bool v_hosts) {
    const int words = (du + 31) / 32;
    const unsigned long long off = base[u] + (unsigned long long)i * (unsigned long long)words;
    CBuildTask T;
    unsigned fl = (unsigned)(off >> 32) & 255u;
    if (!v_hosts) {  // type A: N+(v) is streamed against the staged N+(u)
      T.list = dv.x;
      T.len = dv.y;
    } else {         // type B: N+(u) -- beyond v when the numbering is topological -- is streamed against the staged N+(v)
      const int skip = topo ? i + 1 : 0;
      T.list = ru + skip;
      T.len = du - skip;
      fl |= ((unsigned)skip << 8) | 0x80000000u;
    }
    T.off_lo = (unsigned)off;
    T.off_hi_fl = fl | ((unsigned)words << 20);
    out[slot] = T;
  };
  for (int phase = 0; phase < (PLACE ? 2 : 1); ++phase) {
    for (long long ub = u0; ub < nv; ub += stride) {
      const long long u = ub + (lane >> 3);
      int nt = 0, ru = 0, du = 0;
      if (u < nv) {
        nt = ntask_of[u];  // 0: not an owner of this round, or no matrix (d+ < 3 / > kCbMaxDeg), or every row comes from the core bitmap
        ru = rp[u];
        du = rp[u + 1] - ru;
      }
      const int nmax = wave_max_nonneg(nt);
      for (int i = sub; i - sub < nmax; i += 8) {  // wave-uniform trip count
        const bool act = i < nt;
        const int e = ru + (act ? i : 0);
        const int2 dv = act ? edesc[e] : make_int2(0, 0);  // {rp[v], d+(v)}
        const int tail = topo ? du - i - 1 : du;
        const bool v_hosts = dv.y > tail && dv.y <= kCbMaxDeg;
        if (phase == 0) {
          const unsigned long long mu = __ballot(act && !v_hosts);
          const unsigned gm = (unsigned)(mu >> g8) & 255u;
          int ubase = 0;
          if (gm != 0u && sub == (int)__builtin_ctz(gm)) ubase = atomicAdd(&cnt[u], (int)__builtin_popcount(gm));
          if (PLACE && gm != 0u) {
            ubase = __shfl(ubase, g8 + (int)__builtin_ctz(gm));
            if (act && !v_hosts) put(trp[u] + ubase + (int)__builtin_popcount(gm & ((1u << sub) - 1u)), (int)u, i, ru, du, dv, false);
          }
        }
        if (act && v_hosts) {
          const int host = col[e];
          if (host >= hub0) {
            if (phase == 0) atomicAdd(&hist[host - hub0], 1);
            else put(trp[host] + atomicAdd(&hist[host - hub0], 1), (int)u, i, ru, du, dv, true);
          } else if (phase == 0) {
            if (!PLACE) atomicAdd(&cnt[host], 1);
            else put(trp[host] + atomicAdd(&cnt[host], 1), (int)u, i, ru, du, dv, true);
          }
        }
      }
    }
    if (phase == 0) {
      __syncthreads();
      for (int h = threadIdx.x; h < kHubWin; h += 256) {
        const int c = hist[h];
        if (c) {
          const int b = atomicAdd(&cnt[hub0 + h], c);  // pass 1: the count; pass 2: this workgroup's range among the hub's tasks
          if (PLACE) hist[h] = b;  // (the ranks inside the range are taken from the same word)
        }
      }
      __syncthreads();
    }
  }
}
__global__ __launch_bounds__(256) void cb_slot_base_kernel(int w0, int w1, const int *__restrict__ verts, const unsigned long long *__restrict__ base,
                                                           unsigned long long *__restrict__ slot_base) {
  const int s = w0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (s < w1) slot_base[s] = base[verts[s]];
}

// ---- core bitmap: dense adjacency of the last core_h vertices of a topologically numbered DAG (gm_host.h; gathered by gm_cgather.hip) ----
__global__ __launch_bounds__(256) void core_fill_kernel(int nv, int base, int words, long long e0, long long e1, const int *__restrict__ rp,
                                                         const int *__restrict__ col, unsigned *__restrict__ bits) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = e0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
    int lo = base, hi = nv - 1;  // the row of entry e
    while (lo < hi) {
      const int mid = (int)(((long long)lo + hi + 1) >> 1);
      if (rp[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int w = col[e] - base;  // (topological: w > lo - base >= 0)
    atomicOr(&bits[(size_t)(lo - base) * (size_t)words + (size_t)(w >> 5)], 1u << (w & 31));
  }
}
int ensure_core_bitmap(gm_graph *g) {
  if (g->core.known()) return GM_OK;
  bool topo = false;
  int rc = graph_is_topological(g, &topo);  // (takes the lock itself)
  if (rc) return rc;
  return g->core.ensure(g->mu, [&](HubCore &c) {
    long long want = kCoreHDefault;
    if (const char *e = gm_opt("GM_CORE_H")) want = atoll(e);  // (tests, sweeps: the core's base inside a planted row; 0 switches the gathered build off)
    if (!topo || g->d_rp == nullptr || g->nv < 64 || want < 64) return kOnceNotApplicable;
    SetupTimer timer;
    HIP_TRY(hipSetDevice(g->device));
    const int h = (int)std::min<long long>((long long)g->nv, want);
    const int base = g->nv - h;
    const int words = (h + 31) / 32;
    const size_t bytes = (size_t)h * (size_t)words * 4;
    if (c.bits.alloc(bytes) != hipSuccess) {  // no room: the streamed build does everything
      (void)hipGetLastError();
      return kOnceNotApplicable;
    }
    HIP_TRY(hipMemsetAsync(c.bits, 0, bytes, 0));
    int e01[2] = {0, 0};
    HIP_TRY(hipMemcpy(&e01[0], g->d_rp + base, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&e01[1], g->d_rp + g->nv, sizeof(int), hipMemcpyDeviceToHost));
    const long long n = (long long)e01[1] - e01[0];
    if (n > 0) {
      const long long blocks = std::min<long long>((n + 255) / 256, (long long)g->cu_count * 32);
      hipLaunchKernelGGL(core_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, 0, g->nv, base, words, (long long)e01[0], (long long)e01[1], g->d_rp, g->d_col, c.bits.get());
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    c.h = h;
    c.base = base;
    setup_trace("clique: core bitmap");
    g->setup.table_ms += timer.ms();
    return kOnceBuilt;
  });
}

// ---- the core bitmap cut into blocks of rows for the blocked gather (gm_mine.h CGatherBParams; gm_cgather.hip cgatherb_kernel) ----------
// A block = consecutive core rows whose stored words (row p keeps the words from cgb_first_word(p) on: the columns right of its diagonal)
// fit kCgbWords, at most kCgbMaxRows of them: 16 rows of 4 KB at the bottom of a 32 K core, ~1000 rows of a few words at its top -- where
// the rows that most vertices hold are.
// (bit positions are taken relative to the core's base rounded DOWN to a multiple of 32 -- `delta` = core_base & 31 phantom columns in front --
// so that the word of a column is (vertex id >> 5) minus a constant whatever the graph's size: the kernel folds the constant into the rows'
// LDS offsets and never subtracts the base from a column)
__global__ __launch_bounds__(256) void core_tri_fill_kernel(int nv, int base, long long e0, long long e1, const int *__restrict__ rp, const int *__restrict__ col,
                                                             const int *__restrict__ bid, const int *__restrict__ rowbase, const int4 *__restrict__ blk,
                                                             unsigned *__restrict__ tri) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int base32 = base & ~31;
  for (long long e = e0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
    int lo = base, hi = nv - 1;  // the row of entry e
    while (lo < hi) {
      const int mid = (int)(((long long)lo + hi + 1) >> 1);
      if (rp[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int p = lo - base, q = col[e] - base32;  // (topological: col[e] > lo)
    atomicOr(&tri[(long long)blk[bid[p]].z + rowbase[p] + (q >> 5)], 1u << (q & 31));
  }
}
// the blocks' images and tables on the device, into cb (a failure leaves the handle without them: ensure_core_tri drops the code)
static int build_core_tri(gm_graph *g, const long long total, const std::vector<int> &bid, const std::vector<int> &rowbase, const std::vector<int4> &blk, CoreBlocks &cb) {
  const int h = g->core->h, core_base = g->core->base;
  int e01[2] = {0, 0};
  HIP_TRY(cb.tri.alloc(sizeof(unsigned) * (size_t)std::max<long long>(total, 4)));
  HIP_TRY(cb.bid.alloc(sizeof(int) * (size_t)h));
  HIP_TRY(cb.rowbase.alloc(sizeof(int) * (size_t)h));
  HIP_TRY(cb.blk.alloc(sizeof(int4) * blk.size()));
  HIP_TRY(hipMemsetAsync(cb.tri, 0, sizeof(unsigned) * (size_t)std::max<long long>(total, 4), 0));
  HIP_TRY(copy_to_device(cb.bid, bid.data(), sizeof(int) * (size_t)h));
  HIP_TRY(copy_to_device(cb.rowbase, rowbase.data(), sizeof(int) * (size_t)h));
  HIP_TRY(copy_to_device(cb.blk, blk.data(), sizeof(int4) * blk.size()));
  HIP_TRY(hipMemcpy(&e01[0], g->d_rp + core_base, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&e01[1], g->d_rp + g->nv, sizeof(int), hipMemcpyDeviceToHost));
  const long long n = (long long)e01[1] - e01[0];
  if (n > 0)
    hipLaunchKernelGGL(core_tri_fill_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, (long long)g->cu_count * 32)), dim3(256), 0, 0, g->nv, core_base,
                       (long long)e01[0], (long long)e01[1], g->d_rp, g->d_col, cb.bid, cb.rowbase, cb.blk, cb.tri);
  HIP_TRY(hipDeviceSynchronize());
  cb.n = (int)blk.size();
  return GM_OK;
}
int ensure_core_tri(gm_graph *g) {
  if (g->core_blocks.known()) return GM_OK;
  {
    const int rc = ensure_core_bitmap(g);  // (takes the lock itself)
    if (rc) return rc;
  }
  return g->core_blocks.ensure(g->mu, [&](CoreBlocks &cb) {
    if (!g->core.built() || g->core->h < 64) return kOnceNotApplicable;
    SetupTimer timer;
    HIP_TRY(hipSetDevice(g->device));
    const int h = g->core->h, core_base = g->core->base, delta = core_base & 31, words = cgb_words(h, delta);
    std::vector<int> bid((size_t)h), rowbase((size_t)h);
    std::vector<int4> blk;
    long long total = 0;
    {
      int p0 = 0, used = 0;
      for (int p = 0; p <= h; ++p) {
        const int span = p < h ? words - cgb_first_word(p, delta) : 0;
        if (p == h || used + span > kCgbWords || p - p0 >= kCgbMaxRows) {  // close the block [p0, p)
          if (p > p0) {
            blk.push_back(make_int4(p0, p - p0, (int)total, used));
            total += (used + 3) & ~3;  // (images start at multiples of four words: 16-byte copies)
          }
          p0 = p;
          used = 0;
          if (p == h) break;
        }
        bid[(size_t)p] = (int)blk.size();
        rowbase[(size_t)p] = used - cgb_first_word(p, delta);
        used += span;
      }
    }
    if (total >= (1ll << 31) || blk.size() >= 65536) return kOnceNotApplicable;
    const HipFailureMark mark;
    if (build_core_tri(g, total, bid, rowbase, blk, cb) != GM_OK) {  // (no room: the row-major gather does the work)
      mark.drop();
      cb = CoreBlocks();
      return kOnceNotApplicable;
    }
    setup_trace("clique: core blocks");
    g->setup.table_ms += timer.ms();
    return kOnceBuilt;
  });
}

__global__ __launch_bounds__(256) void iota_u32_kernel(long long n, unsigned *__restrict__ out) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = (unsigned)k;
}
// The units of a round's wide slots.  One wave per slot walks the core part of the vertex's row: a unit starts where the block of the
// row's core position changes.  EMIT = false: units per slot;  EMIT = true: the records {start of the vertex's column table, matrix offset, d | first row << 16, rows}
// + the block as sort key, at the slot's offset.
template <bool EMIT>
__global__ __launch_bounds__(256) void cgb_units_kernel(int w0, int nslots, const int *__restrict__ verts, const int *__restrict__ rp, const int *__restrict__ col,
                                                         const unsigned long long *__restrict__ slot_base, int core_base, const int *__restrict__ bid,
                                                         int *__restrict__ cnt, const int *__restrict__ uoff, const unsigned *__restrict__ poff,
                                                         unsigned *__restrict__ keys, uint4 *__restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const int s = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (s >= nslots) return;  // (wave-uniform)
  const int u = verts[w0 + s];
  const int ru = rp[u], d = rp[u + 1] - ru;
  const int k0 = lower_bound(col + ru, d, core_base);
  int n = 0;
  const int out0 = EMIT ? uoff[s] : 0;
  const unsigned mbase = EMIT ? (unsigned)slot_base[w0 + s] : 0u;
  for (int jb = k0; jb < d; jb += 64) {
    const int j = jb + lane;
    const int b = j < d ? bid[col[ru + j] - core_base] : -1;
    const int bp = (j > k0 && j < d) ? bid[col[ru + j - 1] - core_base] : -2;
    const bool start = j < d && b != bp;
    const unsigned long long m = __ballot(start);
    if (EMIT && start) {
      // rows of the unit: up to the next start in this tile, else scan ahead (units are short: a few rows)
      int e = j + 1;
      while (e < d && bid[col[ru + e] - core_base] == b) ++e;
      const int k = out0 + n + (int)__popcll(m & ((1ull << lane) - 1ull));
      keys[k] = (unsigned)b;
      recs[k] = make_uint4(poff[s], mbase, (unsigned)d | ((unsigned)j << 16), (unsigned)(e - j));
    }
    n += (int)__popcll(m);
  }
  if (!EMIT && lane == 0) cnt[s] = n;
}
// The COLUMN TABLES the blocked gather reads instead of col: per wide slot, the positions of N+(u) as 16-bit numbers q = id - (core_base & ~31)
// (0: a neighbour below the core, or padding), swizzled so that ONE dword load per lane fetches two column tiles -- dword 64 T + l of a vertex
// = q(128 T + l) | q(128 T + 64 + l) << 16: half the bytes of col and half the loads.
__global__ __launch_bounds__(256) void cgb_table_size_kernel(int w0, int nslots, const int *__restrict__ verts, const int *__restrict__ rp, unsigned *__restrict__ sz) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nslots) return;
  unsigned v = 0u;
  if (s < nslots) {
    const int u = verts[w0 + s];
    const int d = rp[u + 1] - rp[u];
    v = 64u * (unsigned)(((d + 63) / 64 + 1) / 2);
  }
  sz[s] = v;
}
__global__ __launch_bounds__(256) void cgb_table_fill_kernel(int w0, int nslots, const int *__restrict__ verts, const int *__restrict__ rp, const int *__restrict__ col,
                                                              int core_base, const unsigned *__restrict__ poff, unsigned *__restrict__ tab) {
  const int lane = threadIdx.x & 63;
  const int s = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (s >= nslots) return;  // (wave-uniform)
  const int u = verts[w0 + s];
  const int ru = rp[u], d = rp[u + 1] - ru, base32 = core_base & ~31;
  unsigned *__restrict__ out = tab + poff[s];
  const int npairs = ((d + 63) / 64 + 1) / 2;
  for (int t = 0; t < npairs; ++t) {
    const int j0 = 128 * t + lane, j1 = j0 + 64;
    const int c0 = j0 < d ? col[ru + j0] : 0, c1 = j1 < d ? col[ru + j1] : 0;
    const unsigned q0 = c0 >= core_base ? (unsigned)(c0 - base32) : 0u, q1 = c1 >= core_base ? (unsigned)(c1 - base32) : 0u;
    out[64 * t + lane] = q0 | (q1 << 16);
  }
}
// sorted order: record k = recs[idx[k]]; its probes = sum over its rows i of (d - 1 - i)
__global__ __launch_bounds__(256) void cgb_gather_kernel(long long n, const unsigned *__restrict__ idx, const uint4 *__restrict__ recs, uint4 *__restrict__ out,
                                                          unsigned long long *__restrict__ cost, unsigned long long *__restrict__ tbytes) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint4 r = recs[idx[k]];
  out[k] = r;
  const long long d = r.z & 0xffffu, i0 = r.z >> 16, rows = r.w;
  cost[k] = (unsigned long long)(rows * (d - 1 - i0) - rows * (rows - 1) / 2 + 64 * rows + 256);  // (+ per row and per unit overheads, in probes)
  // what the unit reads by construction: its record, its rows' positions, the table dwords of the tile pairs from its first row's on
  const long long npairs = ((d + 63) / 64 + 1) / 2, t0 = (i0 + 1) >> 7;
  tbytes[k] = (unsigned long long)(16 + 4 * rows + 256 * (npairs > t0 ? npairs - t0 : 0));
}
__global__ __launch_bounds__(256) void cgb_item_flag_kernel(long long n, const unsigned *__restrict__ keys, const unsigned long long *__restrict__ cum,
                                                             unsigned long long target, int *__restrict__ flag) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  flag[k] = (k == 0 || keys[k] != keys[k - 1] || cum[k] / target != cum[k - 1] / target) ? 1 : 0;
}
__global__ __launch_bounds__(256) void cgb_item_place_kernel(long long n, const unsigned *__restrict__ keys, const int *__restrict__ flag, const int *__restrict__ pos,
                                                              int2 *__restrict__ items, int n_items) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) items[n_items] = make_int2((int)n, -1);
  if (k >= n) return;
  if (flag[k]) items[pos[k]] = make_int2((int)k, (int)keys[k]);
}
#ifndef GM_CGB_ITEM_COST
#define GM_CGB_ITEM_COST (1ull << 20)
#endif
constexpr unsigned long long kCgbItemCost = GM_CGB_ITEM_COST;  // probes (+ overheads) of a work item: ~80 us of one workgroup
static int build_gather_index(gm_graph *g, CliquePlan &pl, CliqueRound &rd, ScanTemp &tmp) {
  const int nslots = (int)(rd.w1 - rd.w0);
  if (nslots <= 0 || pl.core_base < 0 || !g->core_blocks.built() || rd.words >= (1ull << 32)) return GM_OK;  // (no index: the row-major gather)
  DevBuf<int> cnt, uoff;
  HIP_TRY(cnt.alloc((size_t)nslots + 1));
  HIP_TRY(uoff.alloc((size_t)nslots + 1));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(int) * ((size_t)nslots + 1), 0));
  const dim3 wgrid((unsigned)(((long long)nslots + 3) / 4));
  hipLaunchKernelGGL((cgb_units_kernel<false>), wgrid, dim3(256), 0, 0, (int)rd.w0, nslots, pl.d_verts, g->d_rp, g->d_col, pl.d_slot_base, pl.core_base, g->core_blocks->bid.get(),
                     cnt.p, nullptr, nullptr, nullptr, nullptr);
  int nu = 0;
  HIP_TRY(dev_scan_total(tmp, cnt.p, uoff.p, (size_t)nslots, &nu));
  if (nu <= 0) return GM_OK;
  // the column tables of the round's slots
  DevBuf<unsigned> tsz, poff;
  HIP_TRY(tsz.alloc((size_t)nslots + 1));
  HIP_TRY(poff.alloc((size_t)nslots + 1));
  hipLaunchKernelGGL(cgb_table_size_kernel, grid_1d((long long)nslots + 1), dim3(256), 0, 0, (int)rd.w0, nslots, pl.d_verts, g->d_rp, tsz.p);
  unsigned tab_words = 0;
  HIP_TRY(dev_scan_total(tmp, tsz.p, poff.p, (size_t)nslots, &tab_words));
  DevOwn<unsigned> tab;  // (the round's once the index is complete)
  // (+ nine tile pairs of slack: the kernel requests nine pairs from a unit's first one on without looking at the table's end -- what lies
  // beyond belongs to tiles the vertex does not have and is never used; byte offsets are 32 bits)
  if ((unsigned long long)tab_words * 4ull + 4096ull >= (1ull << 32)) return GM_OK;  // (no index: the row-major gather)
  HIP_TRY(tab.alloc(sizeof(unsigned) * ((size_t)std::max(tab_words, 64u) + 9 * 64)));
  hipLaunchKernelGGL(cgb_table_fill_kernel, wgrid, dim3(256), 0, 0, (int)rd.w0, nslots, pl.d_verts, g->d_rp, g->d_col, pl.core_base, poff.p, tab);
  DevBuf<unsigned> keys, keys_s, idx, idx_s;
  DevBuf<uint4> recs;
  DevBuf<unsigned long long> cost, cum;
  DevBuf<int> flag, pos;
  HIP_TRY(keys.alloc((size_t)nu));
  HIP_TRY(keys_s.alloc((size_t)nu));
  HIP_TRY(idx.alloc((size_t)nu));
  HIP_TRY(idx_s.alloc((size_t)nu));
  HIP_TRY(recs.alloc((size_t)nu));
  hipLaunchKernelGGL((cgb_units_kernel<true>), wgrid, dim3(256), 0, 0, (int)rd.w0, nslots, pl.d_verts, g->d_rp, g->d_col, pl.d_slot_base, pl.core_base, g->core_blocks->bid.get(),
                     nullptr, uoff.p, poff.p, keys.p, recs.p);
  hipLaunchKernelGGL(iota_u32_kernel, grid_1d(nu), dim3(256), 0, 0, (long long)nu, idx.p);
  int bits = 1;
  while ((1 << bits) < g->core_blocks->n) ++bits;
  HIP_TRY(dev_sort_pairs<false>(tmp, keys.p, keys_s.p, idx.p, idx_s.p, (size_t)nu, 0, bits));  // (stable: a block's units stay in slot order)
  DevOwn<uint4> units;
  HIP_TRY(units.alloc(sizeof(uint4) * (size_t)nu));
  HIP_TRY(cost.alloc((size_t)nu + 1));
  HIP_TRY(cum.alloc((size_t)nu + 1));
  HIP_TRY(flag.alloc((size_t)nu + 1));
  HIP_TRY(pos.alloc((size_t)nu + 1));
  hipLaunchKernelGGL(cgb_gather_kernel, grid_1d(nu), dim3(256), 0, 0, (long long)nu, idx_s.p, recs.p, units, cost.p, cum.p);
  // (cum holds the units' table bytes for a moment: their sum is the kernel's own bytes, gm_clique4_gather_info)
  HIP_TRY(dev_sum(tmp, cum.p, (size_t)nu, &rd.gather_table_bytes));
  HIP_TRY(dev_exclusive_sum(tmp, cost.p, cum.p, (size_t)nu));
  HIP_TRY(hipMemsetAsync(flag.p + nu, 0, sizeof(int), 0));
  hipLaunchKernelGGL(cgb_item_flag_kernel, grid_1d(nu), dim3(256), 0, 0, (long long)nu, keys_s.p, cum.p, kCgbItemCost, flag.p);
  int ni = 0;
  HIP_TRY(dev_scan_total(tmp, flag.p, pos.p, (size_t)nu, &ni));
  DevOwn<int2> items;
  HIP_TRY(items.alloc(sizeof(int2) * ((size_t)ni + 1)));
  hipLaunchKernelGGL(cgb_item_place_kernel, grid_1d(nu), dim3(256), 0, 0, (long long)nu, keys_s.p, flag.p, pos.p, items, ni);
  HIP_TRY(hipDeviceSynchronize());
  rd.d_gunits = std::move(units);
  rd.d_gtab = std::move(tab);
  rd.d_gitems = std::move(items);
  rd.n_gunits = (size_t)nu;
  rd.n_gitems = (size_t)ni;
  return GM_OK;
}

int clique_wide_min_words() {
  static const int v = [] {
    const char *e = gm_sweep_env("GM_WIDE_MIN_WORDS");  // (sweeps; read once: tables and plans are cached per graph)
    return e ? std::max(64, std::min(atoi(e), kBitWords)) : kWideMinWordsDefault;
  }();
  return v;
}

__global__ __launch_bounds__(256) void mcls_rec_kernel(int n, const int *__restrict__ slots, const int *__restrict__ verts, const int *__restrict__ rp,
                                                       const unsigned long long *__restrict__ slot_base, int4 *__restrict__ rec) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int slot = slots[k], u = verts[slot];
  const unsigned long long b = slot_base[slot];
  rec[k] = make_int4(rp[u + 1] - rp[u], (int)(unsigned)b, (int)(unsigned)(b >> 32), 0);
}

// one round: owners -> offsets -> task lists -> host-chunk table
static int build_clique_round(gm_graph *g, CliquePlan &pl, CliqueRound &rd, ScanTemp &tmp) {
  const int nv = g->nv;
  const size_t nv1 = (size_t)nv + 1;
  DevBuf<int> own, ntask_of, tpos, cnt;
  DevBuf<unsigned long long> words;
  HIP_TRY(own.alloc(nv1));
  HIP_TRY(ntask_of.alloc(nv1));
  HIP_TRY(tpos.alloc(nv1));
  HIP_TRY(words.alloc(nv1));
  HIP_TRY(hipMemsetAsync(own.p, 0, sizeof(int) * nv1, 0));
  if (rd.n_count > 0)
    hipLaunchKernelGGL(cb_own_chunks_kernel, grid_1d(rd.n_count), dim3(256), 0, 0, rd.n_count, pl.n_first + rd.n_pos0 * pl.n_step, pl.n_step, pl.d_order, pl.tabN->d, own.p);
  if (rd.w1 > rd.w0)
    hipLaunchKernelGGL(cb_own_verts_kernel, grid_1d((long long)(rd.w1 - rd.w0)), dim3(256), 0, 0, (int)(rd.w1 - rd.w0), pl.d_verts + rd.w0, own.p);
  hipLaunchKernelGGL(cb_owner_sizes_kernel, grid_1d((long long)nv1), dim3(256), 0, 0, nv, g->d_rp, g->d_col, own.p, pl.core_base, words.p, ntask_of.p);
  HIP_TRY(rd.d_base.alloc(sizeof(unsigned long long) * nv1));
  int nt = 0;
  HIP_TRY(dev_scan_total(tmp, words.p, rd.d_base.get(), (size_t)nv, &rd.words));
  HIP_TRY(dev_scan_total(tmp, ntask_of.p, tpos.p, (size_t)nv, &nt));
  rd.n_tasks = (size_t)nt;
  HIP_TRY(rd.d_trp.alloc(sizeof(int) * nv1));
  if (rd.w1 > rd.w0)  // (before the early return: a round whose wide rows all come from the core bitmap has no streamed task at all)
    hipLaunchKernelGGL(cb_slot_base_kernel, grid_1d((long long)(rd.w1 - rd.w0)), dim3(256), 0, 0, (int)rd.w0, (int)rd.w1, pl.d_verts, rd.d_base, pl.d_slot_base);
  if (nt == 0) {
    HIP_TRY(hipMemset(rd.d_trp, 0, sizeof(int) * nv1));
    HIP_TRY(hipDeviceSynchronize());
    return GM_OK;
  }
  HIP_TRY(cnt.alloc(nv1));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(int) * nv1, 0));
  const dim3 kgrid = row_walk_grid(g, pl.topo ? 8 : 64);
  const int hub0 = pl.topo ? std::max(0, nv - kHubWin) : nv;
  hipLaunchKernelGGL((cb_task_rows_kernel<false>), kgrid, dim3(256), 0, 0, nv, g->d_rp, g->d_col, g->edesc->get(), ntask_of.p, pl.topo ? 1 : 0, hub0,
                     cnt.p, nullptr, nullptr, nullptr);
  HIP_TRY(dev_exclusive_sum(tmp, cnt.p, rd.d_trp.get(), nv1));
  HIP_TRY(rd.d_tasks.alloc(sizeof(CBuildTask) * (size_t)nt));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(int) * nv1, 0));
  hipLaunchKernelGGL((cb_task_rows_kernel<true>), kgrid, dim3(256), 0, 0, nv, g->d_rp, g->d_col, g->edesc->get(), ntask_of.p, pl.topo ? 1 : 0, hub0,
                     cnt.p, rd.d_trp, rd.d_base, rd.d_tasks);
  HIP_TRY(hipGetLastError());
  // host chunks: runs of consecutive vertices whose DAG rows fit the stage (longer rows host nothing), costs from the task lists,
  // heavy chunks cut into parts like gm_tch.hip's (a hub hosts 10^5 in-edges)
  ChunkTable &t = rd.host_tab;
  t.target = std::max(64, std::min(pl.target, pl.stage));
  t.allow_split = true;
  t.bit_words = 0;
  t.part_cap = task_part_cap(g, pl.world);
  t.stage_cap = pl.stage;
  t.rf.tct = 1;
  t.rf.skip_lo = pl.stage;
  t.rf.skip_hi = 0x7fffffff;
  t.bitmap_min_deg = 0x7fffffff;
  double bm_ms = 0;
  int rc = build_table_device(g, t, false, bm_ms, rd.d_trp, &rd.d_tasks[0].len, (int)(sizeof(CBuildTask) / sizeof(int)));
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return GM_OK;
}

int get_clique_plan(gm_graph *g, int rank, int world, int policy, int target, unsigned long long part_cap, CliquePlan **out) {
  {
    std::lock_guard<std::mutex> lk(g->mu);
    for (auto &pl : g->clique_plans)
      if (pl.rank == rank && pl.world == world && pl.policy == policy && pl.target == target) { *out = &pl; return GM_OK; }
  }
  // (built outside the lock: the solvers have ONE caller per handle; get_table below takes the lock itself)
  HIP_TRY(hipSetDevice(g->device));
  CliquePlan pl;
  pl.rank = rank; pl.world = world; pl.policy = policy; pl.target = target;
  pl.stage = g->max_deg <= kStageCapClique ? kStageCapClique : kCbMaxDeg;
  // narrow chunk table (whole rows, matrices of a chunk <= kBitWords words together; the wide and the huge rows left out)
  {
    RowFilter rf;
    rf.skip_clique_wide = clique_wide_min_words();
    rf.only_hi = kCbMaxDeg;  // rows beyond the stage of the build kernel: mine_kernel's arena path (run_pattern)
    const int rc = get_table(g, target, false, kBitWords, part_cap, kStageCapClique, &pl.tabN, rf, kBitmapMinDeg);
    if (rc) return rc;
  }
  {
    const int rc = ensure_edesc(g);  // (the task records read the targets' {start, length} from the edge descriptors)
    if (rc) return rc;
    setup_trace("clique: narrow table + edge descriptors");
  }
  SetupTimer timer;
  PoolScope pool(g);  // (the per-vertex arrays of the rounds)
  ScanTemp tmp;
  // once per graph: the wide vertices, longest rows first (select + stable radix sort by row length)
  if (const int rc_w = g->wide.ensure(g->mu, [&](WideVerts &wv) {
    DevBuf<int> sel, degs, keyo;
    int m = 0;
    if (const int rc = dev_select_by_degree(tmp, g->nv, g->d_rp, WideRow{clique_wide_min_words()}, sel, degs, &m)) return rc;
    wv.n = (size_t)m;
    if (m > 0) {
      HIP_TRY(keyo.alloc((size_t)m));
      HIP_TRY(wv.sorted.alloc(sizeof(int) * (size_t)m));
      HIP_TRY(dev_sort_pairs<true>(tmp, degs.p, keyo.p, sel.p, wv.sorted.get(), (size_t)m));
    }
    return kOnceBuilt;
  })) return rc_w;
  {  // topological numbering? (decides whether the in-edge tasks stream only the part of N+(u) beyond v)
    bool topo = false;
    const int rc = graph_is_topological(g, &topo);
    if (rc) return rc;
    pl.topo = topo && !gm_sweep_env("GM_CLIQUE_NO_TOPO");  // (GM_CLIQUE_NO_TOPO: A/B, whole lists streamed)
    if (pl.topo) {  // the dense hub core: rows of the wide vertices' matrices are gathered from it (gm_cgather.hip)
      const int rc2 = ensure_core_bitmap(g);
      if (rc2) return rc2;
      if (g->core.built()) pl.core_base = g->core->base;
    }
  }
  {  // this rank's share of the narrow table: every world-th chunk of the cost-ordered dequeue list, a contiguous range, or the
     // chunks of a vertex range
    ChunkTable *tb = pl.tabN;
    const long long n = (long long)tb->n;
    long long first = 0, step = 1, count = 0;
    if (policy == GM_PART_VERTEX) {
      const int rc = table_host_views(g, tb);
      if (rc) return rc;
      chunk_range_of_vertex_share(tb, g->nv, rank, world, &first, &count);
    } else {
      gm_partition((int64_t)n, rank, world, policy, (int64_t *)&first, (int64_t *)&step, (int64_t *)&count);
    }
    pl.n_first = first; pl.n_step = step; pl.n_count = count;
    pl.d_order = (policy == GM_PART_ROUND_ROBIN) ? tb->d_order[pl.order_which] : nullptr;
  }
  // this rank's share of the wide list
  int64_t wfirst = 0, wstep = 1, wcount = 0;
  gm_partition((int64_t)g->wide->n, rank, world, policy == GM_PART_VERTEX ? GM_PART_RANGE : policy, &wfirst, &wstep, &wcount);
  std::vector<int> hd((size_t)wcount);
  if (wcount > 0) {
    DevBuf<int> degs;
    HIP_TRY(pl.d_verts.alloc(sizeof(int) * (size_t)wcount));
    HIP_TRY(pl.d_slot_base.alloc(sizeof(unsigned long long) * (size_t)wcount));
    HIP_TRY(degs.alloc((size_t)wcount));
    hipLaunchKernelGGL(wide_share_kernel, grid_1d(wcount), dim3(256), 0, 0, (int)wcount, (long long)wfirst, (long long)wstep, g->wide->sorted.get(), g->d_rp, pl.d_verts, degs.p);
    pl.verts.resize((size_t)wcount);
    HIP_TRY(copy_to_host(pl.verts.data(), pl.d_verts, sizeof(int) * (size_t)wcount));
    HIP_TRY(copy_to_host(hd.data(), degs.p, sizeof(int) * (size_t)wcount));
  }
  setup_trace("clique: wide share to the host");
  // rounds within the arena budget: the narrow chunks first (in dequeue order), then the wide vertices (longest rows first)
  unsigned long long arena_mb = GM_WIDE_ARENA_MB;
  if (const char *e = gm_opt("GM_WIDE_ARENA_MB")) arena_mb = std::max(1ll, atoll(e));  // (tests: force several rounds)
  const unsigned long long budget_words = (arena_mb << 20) / 4ull;
  // (the per-chunk words come to the host only when the narrow chunks alone overflow the arena: one round needs their sum)
  std::vector<unsigned long long> cw;
  unsigned long long cw_total = 0;
  if (pl.n_count > 0) {
    DevBuf<unsigned long long> dcw;
    HIP_TRY(dcw.alloc((size_t)pl.n_count));
    hipLaunchKernelGGL(cb_chunk_words_kernel, grid_1d(pl.n_count), dim3(256), 0, 0, pl.n_count, pl.n_first, pl.n_step, pl.d_order, pl.tabN->d, g->d_rp, dcw.p);
    HIP_TRY(dev_sum(tmp, dcw.p, (size_t)pl.n_count, &cw_total));
    if (cw_total > budget_words) {
      cw.resize((size_t)pl.n_count);
      HIP_TRY(copy_to_host(cw.data(), dcw.p, sizeof(unsigned long long) * (size_t)pl.n_count));
    }
  }
  setup_trace("clique: words of the narrow chunks to the host");
  std::vector<int> cls_slots, mcls_slots;
  {
    long long c0 = 0;
    size_t s0 = 0;
    while (c0 < pl.n_count || s0 < (size_t)wcount || pl.rounds.empty()) {
      CliqueRound rd;
      unsigned long long words = 0;
      long long c1 = c0;
      if (cw.empty()) {  // every narrow chunk fits one round: the first
        if (c0 < pl.n_count) words = cw_total;
        c1 = pl.n_count;
      } else {
        for (; c1 < pl.n_count; ++c1) {
          if ((c1 > c0) && words + cw[(size_t)c1] > budget_words) break;
          words += cw[(size_t)c1];
        }
      }
      size_t s1 = s0;
      std::vector<int> by_mcls[3];
      if (c1 == pl.n_count) {  // (wide vertices only once the narrow chunks are placed)
        for (; s1 < (size_t)wcount; ++s1) {
          const int d = hd[s1];
          const unsigned long long w = (unsigned long long)d * (unsigned long long)((d + 31) / 32);
          if ((s1 > s0 || c1 > c0) && words + w > budget_words) break;
          words += w;
          pl.wide_edges += (unsigned long long)d;
          by_mcls[clique_mma_class(d)].push_back((int)s1);
        }
      }
      rd.n_pos0 = c0; rd.n_count = c1 - c0;
      rd.w0 = s0; rd.w1 = s1;
      for (int c = 0; c < 3; ++c) {
        rd.mcls_begin[c] = mcls_slots.size();
        mcls_slots.insert(mcls_slots.end(), by_mcls[c].begin(), by_mcls[c].end());
      }
      rd.mcls_begin[3] = mcls_slots.size();
      pl.rounds.push_back(std::move(rd));
      c0 = c1;
      s0 = s1;
      if (c0 >= pl.n_count && s0 >= (size_t)wcount) break;
    }
  }
  setup_trace("clique: rounds (host loop)");
  HIP_TRY(pl.d_mcls_slots.alloc(sizeof(int) * std::max<size_t>(mcls_slots.size(), 1)));
  if (!mcls_slots.empty()) HIP_TRY(copy_to_device(pl.d_mcls_slots, mcls_slots.data(), sizeof(int) * mcls_slots.size()));
  setup_trace("clique: wide list, classes, rounds (host)");
  unsigned long long need_words = 0;
  for (size_t r = 0; r < pl.rounds.size(); ++r) {
    const int rc = build_clique_round(g, pl, pl.rounds[r], tmp);
    if (rc) return rc;  // (the half-built plan goes back with `pl`)
    if (pl.core_base >= 0) {
      int rc2 = ensure_core_tri(g);
      if (rc2 == GM_OK) rc2 = build_gather_index(g, pl, pl.rounds[r], tmp);
      if (rc2) return rc2;
    }
    need_words = std::max(need_words, pl.rounds[r].words);
  }
  if (!mcls_slots.empty()) {  // (the slot offsets are known now: the records the count kernels read behind their dequeue)
    HIP_TRY(pl.d_mcls_rec.alloc(sizeof(int4) * mcls_slots.size()));
    hipLaunchKernelGGL(mcls_rec_kernel, grid_1d((long long)mcls_slots.size()), dim3(256), 0, 0, (int)mcls_slots.size(), pl.d_mcls_slots, pl.d_verts, g->d_rp,
                       pl.d_slot_base, pl.d_mcls_rec);
  }
  setup_trace("clique: rounds built");
  const size_t need = (size_t)need_words * 4;
  if (need > g->arena.mat_bytes) {
    g->arena.mat_bytes = 0;
    HIP_TRY(g->arena.mat.alloc(std::max<size_t>(need, 16)));
    g->arena.mat_bytes = need;
  }
  if (!g->arena.queue) HIP_TRY(g->arena.queue.alloc(65536));
  setup_trace("clique: arena");
  HIP_TRY(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(g->mu);
  g->clique_plans.push_back(std::move(pl));
  *out = &g->clique_plans.back();
  g->setup.table_ms += timer.ms();
  return GM_OK;
}

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_clique_plan_kernel() {}
void gm_touch_clique_plan() { hipLaunchKernelGGL(gm_touch_clique_plan_kernel, dim3(1), dim3(1), 0, 0); }
