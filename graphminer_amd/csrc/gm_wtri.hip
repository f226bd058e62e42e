// gm_wtri.hip -- the raw sums behind the six 5-vertex patterns of the reference's sgl solver that need no enumeration of 5-tuples
// (src/sgl/omp_base.cc:29-45: 5path, semihouse, closedhouse, hourglass, taileddiamond, taileddiamond2; DESIGN.md "SgL, 5-vertex closed forms").
// With t(e) the support of an edge (gm_sup.hip), x(e) = t(e) - 1, d(v) the symmetric degree, T_v the triangles at v:
//   wtri_kernel        A = sum_tri [x(bc)(d(a)-2) + x(ac)(d(b)-2) + x(ab)(d(c)-2)],  B = sum_tri [x(ab)x(ac) + x(ab)x(bc) + x(ac)x(bc)]
//                      -- a SECOND pass over the triangles of the oriented copy, on the task lists of the edge supports (trp / tdesc / tedge): the
//                      host row as a hashed set in LDS (gm_hset.h), a match knows its three DAG entries like sup_kernel's -- the task's own,
//                      host row start + position, the index of the streamed key -- reads their supports and adds the two terms to
//                      lane-private 64-bit sums.  It only reads: no per-match atomics, one atomic per workgroup and sum.
//   wtri_edge_kernel   the same terms for the out-edges no task list holds (rows beyond the 2048-entry stage, or the rows of the hub corner
//                      the supports take on the matrix cores): one wave per edge, the longer list bisected in global memory.
//   wtri_entry_kernel  per DAG entry: ed(e) = d(u) + d(v), 2 T_v by scatter, and the sums  sum t,  sum C(t,2)  (D),  sum C(t,2)(d(u)+d(v)-6)  (W)
//   wtri_vertex_kernel H = sum_v C(T_v, 2),  S = sum_v T_v d(v)
//   path5_kernel       P = sum_v (e1(v)^2 - p2(v)) / 2 on the symmetric graph
//   chouse_kernel      Q = sum_e (t(e) - 2) sum_{c in S_e} |S_e ^ N(c)| on the symmetric graph (closedhouse.h with its two inner loops folded)
// The degree opposite an edge of a triangle {a, b, c} is d(a) + d(b) + d(c) - ed(e): the pass needs no vertex of the triangle but the key.
// Everything is uint64 arithmetic modulo 2^64; the halvings act on exact per-item values.
#include "gm_hset.h"

namespace gm {

constexpr int kWtriWaves = 4;
constexpr int kWtriTiles = 2;

template <int STAGE>
struct alignas(16) WtriLds {
  HsTable<STAGE> set;
  int trpl[kMaxChunkVerts + 1];  // row offsets of the chunk's task lists
  HsWave<STAGE> w[kWtriWaves];   // (while the set is built: the fill counters of its buckets)
  unsigned long long part[kWtriWaves][2];
  int next_batch;
  unsigned queue_pos;
  int pad_[2];
};

// the A and B terms of one triangle from its three DAG entries (eo: the task's own edge; eh, es: the host's and the streamed list's edge to the key)
struct WtriAcc {
  const unsigned *__restrict__ sup;
  const unsigned *__restrict__ ed;
  const int *__restrict__ deg;
  const int *__restrict__ col;
  unsigned long long a = 0, b = 0;
  __device__ __forceinline__ void add(const int eo, const int eh, const int es) {
    const unsigned long long x0 = (unsigned long long)sup[eo] - 1ull, x1 = (unsigned long long)sup[eh] - 1ull, x2 = (unsigned long long)sup[es] - 1ull;
    const unsigned long long f0 = ed[eo], f1 = ed[eh], f2 = ed[es];
    const unsigned long long ds = f0 + (unsigned long long)(unsigned)deg[col[es]] - 2ull;  // d(a) + d(b) + d(c) - 2
    a += x0 * (ds - f0) + x1 * (ds - f1) + x2 * (ds - f2);
    b += x0 * x1 + x0 * x2 + x1 * x2;
  }
};

template <int STAGE>
__global__ __launch_bounds__((kWtriWaves * GM_WAVE), 2)
void wtri_kernel(const MineParams p, const WtriParams wp) {
  __shared__ WtriLds<STAGE> B;
  using H = HsHash<STAGE>;
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const int wave = threadIdx.x >> 6;
  const int tid = threadIdx.x;
  constexpr int nthreads = kWtriWaves * GM_WAVE;
  const int *__restrict__ rp = p.g.rp;
  const int *__restrict__ col = p.g.col;
  const int *__restrict__ trp = p.g.trp;
  const int2 *__restrict__ tdesc = p.g.tdesc;
  const int *__restrict__ tedge = p.g.tedge;
  HsWave<STAGE> &L = B.w[wave];
  WtriAcc acc{wp.sup, wp.ed, wp.deg, col};
  for (;;) {
    if (tid == 0) B.queue_pos = atomicAdd(p.queue, (unsigned)p.grab);
    __syncthreads();
    const unsigned q = B.queue_pos;
    if (q >= (unsigned)p.count) break;
    const unsigned qe = min(q + (unsigned)p.grab, (unsigned)p.count);
    for (unsigned ci = q; ci < qe; ++ci) {
      const size_t pos = (size_t)p.first + (size_t)ci * (size_t)p.step;
      const size_t cid = p.order ? (size_t)p.order[pos] : pos;
      const ChunkRec r = p.chunks[cid];
      const int ub = r.u_begin, nvl = r.u_end - r.u_begin;
      const int eb = r.e_begin, nel = r.e_end - r.e_begin;
      for (int i = tid; i <= nvl; i += nthreads) B.trpl[i] = trp[ub + i];
      if (tid == 0) B.next_batch = 0;
      const bool fallback = hs_build<STAGE, nthreads>(B.set, reinterpret_cast<unsigned *>(&B.w[0]), rp, col, ub, nvl, eb, nel,
                                                       (p.flags & (1 << 22)) != 0, tid);  // (ends with a barrier)
      const int tb = B.trpl[0], ntask = B.trpl[nvl] - tb;
      for (;;) {
        int bi = 0;
        if (lane == 0) bi = atomicAdd(&B.next_batch, 1);
        bi = readfirst(bi) * r.nparts + r.part;
        const int t0 = bi * GM_WAVE;
        if (t0 >= ntask) break;
        const bool valid = t0 + lane < ntask;
        const int te = tb + min(t0 + lane, ntask - 1);
        const int2 d = tdesc[te];                      // {start, length} of the list to stream
        const int own_e = tedge[te];                   // the task's own DAG entry
        const int lo = hs_local_row(B.trpl, nvl, te);  // the host row of this task
        const int ru = B.set.rpl[lo], a = B.set.rpl[lo + 1] - ru;
        const bool act = valid && d.y > 0 && a > 0;
        wave_sync();
        // the two per-task words handed back with a match: word = the DAG entry the host's row starts at, word2 = the task's own entry
        auto hit = [&](const unsigned long long hm, const int word, const int word2, const unsigned at, const int kidx, const bool) {
          if (hm == 0ull) return;  // wave-uniform
          if (__builtin_amdgcn_inverse_ballot_w64(hm)) acc.add(word2, word + (int)at, kidx);
        };
        auto hit1 = [&](const int word, const int word2, const int at, const int kidx) {  // one key found through the surplus list (wave-uniform)
          if (lane == 0) acc.add(word2, word + at, kidx);
        };
        hs_pass<STAGE, kWtriTiles>(B.set, L, col, fallback, lane, act ? d.y : 0, d.x, H::salt(lo), ru - eb, a, ru, own_e, hit, hit1);
        wave_sync();
      }
      __syncthreads();  // every wave is done with the chunk: the set is rewritten by the next one
    }
  }
  const unsigned long long sa = wave_sum_u64(acc.a), sb = wave_sum_u64(acc.b);
  if (lane == 0) {
    B.part[wave][0] = sa;
    B.part[wave][1] = sb;
  }
  __syncthreads();
  if (tid < 2) {
    unsigned long long t = 0;
    for (int w = 0; w < kWtriWaves; ++w) t += B.part[w][tid];
    if (t) atomicAdd(&p.counters[tid], t);
  }
}

// One wave per out-edge u -> v of the rows no task list holds: `rows` / `prefix` name them (the rows beyond the stage), or -- rows == nullptr --
// they are the rows from `v0` on (the hub corner; total: an upper bound for the grid).  The shorter of N+(u) -- beyond v under a topological
// numbering -- and N+(v) is streamed by the lanes, the longer one bisected in global memory.
__global__ __launch_bounds__(256) void wtri_edge_kernel(const WtriEdgeParams p, const WtriParams wp) {
  __shared__ unsigned long long part[4][2];
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  WtriAcc acc{wp.sup, wp.ed, wp.deg, p.col};
  const long long e0 = p.rows ? 0ll : (long long)p.rp[p.v0];
  const long long total = p.rows ? p.total : p.ne - e0;
  for (long long t = wave0; t < total; t += nwaves) {
    int u, e;
    if (p.rows) {
      int lo = 0, hi = p.nrows - 1;  // the row of edge t: largest r with prefix[r] <= t (wave-uniform)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.prefix[mid] <= t) lo = mid; else hi = mid - 1;
      }
      u = p.rows[lo];
      e = p.rp[u] + (int)(t - p.prefix[lo]);
    } else {
      e = (int)(e0 + t);
      int lo = p.v0, hi = p.nv - 1;  // largest v with rp[v] <= e
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.rp[mid] <= e) lo = mid; else hi = mid - 1;
      }
      u = lo;
    }
    const int ru = p.rp[u], du = p.rp[u + 1] - ru, i = e - ru, v = p.col[e];
    const int rv = p.rp[v], dv = p.rp[v + 1] - rv;
    const int skip = p.topo ? i + 1 : 0;
    const int abase = ru + skip, a = du - skip;
    const bool a_short = a <= dv;
    const int sbase = a_short ? abase : rv, sn = a_short ? a : dv, lbase = a_short ? rv : abase, ln = a_short ? dv : a;
    for (int k = lane; k < sn; k += GM_WAVE) {
      const int key = p.col[sbase + k];
      const int pos = lower_bound(p.col + lbase, ln, key);
      if (pos < ln && p.col[lbase + pos] == key) acc.add(e, lbase + pos, sbase + k);
    }
  }
  const unsigned long long sa = wave_sum_u64(acc.a), sb = wave_sum_u64(acc.b);
  if (lane == 0) {
    part[threadIdx.x >> 6][0] = sa;
    part[threadIdx.x >> 6][1] = sb;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned long long t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (t) atomicAdd(&p.counters[threadIdx.x], t);
  }
}

// block-wide sums of n lane-private 64-bit values -> one atomic per workgroup and sum (256 threads)
template <int N>
__device__ __forceinline__ void block_add_u64(const unsigned long long (&v)[N], unsigned long long *__restrict__ out) {
  __shared__ unsigned long long part[4][N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long s = wave_sum_u64(v[k]);
    if ((threadIdx.x & (GM_WAVE - 1)) == 0) part[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const unsigned long long t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (t) atomicAdd(&out[threadIdx.x], t);
  }
}

__device__ __forceinline__ unsigned long long choose2_u64(const unsigned long long x) {  // C(x, 2) mod 2^64: the even factor is halved first
  if (x < 2ull) return 0ull;
  return (x & 1ull) ? x * ((x - 1ull) >> 1) : (x >> 1) * (x - 1ull);
}

// symmetric degrees of a DAG: out-degree, then one increment per entry at its target
__global__ __launch_bounds__(256) void wtri_outdeg_kernel(int nv, const int *__restrict__ rp, int *__restrict__ deg) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) deg[v] = rp[v + 1] - rp[v];
}
__global__ __launch_bounds__(256) void wtri_indeg_kernel(long long ne, const int *__restrict__ col, int *__restrict__ deg) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += stride) atomicAdd(&deg[col[e]], 1);
}

// per DAG entry: ed, the scatter of the supports into 2 T_v, and out[0] += t, out[1] += C(t, 2), out[2] += C(t, 2) (d(u) + d(v) - 6)
__global__ __launch_bounds__(256) void wtri_entry_kernel(const WtriEntryParams p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s[3] = {0ull, 0ull, 0ull};
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < p.ne; e += stride) {
    int lo = 0, hi = p.nv - 1;  // largest u with rp[u] <= e
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((long long)p.rp[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int u = lo, v = p.col[e];
    const unsigned long long t = p.sup[e];
    const unsigned long long dd = (unsigned long long)(unsigned)p.deg[u] + (unsigned long long)(unsigned)p.deg[v];
    p.ed[e] = (unsigned)dd;
    if (t) {
      atomicAdd(&p.tv2[u], t);
      atomicAdd(&p.tv2[v], t);
    }
    const unsigned long long c2 = t * (t - (t ? 1ull : 0ull)) / 2ull;  // (t < 2^32: exact)
    s[0] += t;
    s[1] += c2;
    s[2] += c2 * (dd - 6ull);  // (c2 != 0 implies d(u), d(v) >= 3)
  }
  block_add_u64<3>(s, p.out);
}

// per vertex: out[3] += C(T_v, 2), out[4] += T_v d(v)
__global__ __launch_bounds__(256) void wtri_vertex_kernel(int nv, const unsigned long long *__restrict__ tv2, const int *__restrict__ deg,
                                                          unsigned long long *__restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s[2] = {0ull, 0ull};
  for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const unsigned long long tv = tv2[v] >> 1;
    s[0] += choose2_u64(tv);
    s[1] += tv * (unsigned long long)(unsigned)deg[v];
  }
  block_add_u64<2>(s, out + 3);
}

// P: one wave per row of the symmetric graph, e1 = sum (d(a) - 1) < 2^31, p2 = sum (d(a) - 1)^2; (e1^2 - p2) / 2 is exact per row
__global__ __launch_bounds__(256) void path5_kernel(int nv, const int *__restrict__ rp, const int *__restrict__ col, unsigned long long *__restrict__ out) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  unsigned long long s[1] = {0ull};
  for (long long v = wave0; v < nv; v += nwaves) {
    const int r0 = rp[v], r1 = rp[v + 1];
    unsigned long long e1 = 0, p2 = 0;
    for (int j = r0 + lane; j < r1; j += GM_WAVE) {
      const int a = col[j];
      const unsigned long long x = (unsigned long long)(unsigned)(rp[a + 1] - rp[a] - 1);
      e1 += x;
      p2 += x * x;
    }
    e1 = wave_sum_u64(e1);
    p2 = wave_sum_u64(p2);
    if (lane == 0) s[0] += (e1 * e1 - p2) >> 1;
  }
  block_add_u64<1>(s, out);
}

// Q: one wave per undirected edge {u, v}, v < u, of the symmetric graph: S = N(u) ^ N(v) materialised (LDS up to kChouseCap keys of the
// shorter list, else the wave's slot of the global scratch), then for every member c the keys of S ^ N(c) -- the shorter streamed, the
// longer bisected (gm_setops.h) -- times (|S| - 2).
__global__ __launch_bounds__(256) void chouse_kernel(const ChouseParams p) {
  __shared__ int sets[4][kChouseCap];
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  int *gS = p.scratch + (size_t)wave0 * (size_t)p.max_deg;
  unsigned long long s[1] = {0ull};
  for (long long e = wave0; e < p.ne; e += nwaves) {
    int lo = 0, hi = p.nv - 1;  // largest u with rp[u] <= e (wave-uniform)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((long long)p.rp[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int u = lo, v = p.col[e];
    if (v >= u) continue;
    const int ru = p.rp[u], a = p.rp[u + 1] - ru, rv = p.rp[v], b = p.rp[v + 1] - rv;
    if (min(a, b) < 3) continue;  // |S| <= 2: no term
    int *S = min(a, b) <= kChouseCap ? sets[threadIdx.x >> 6] : gS;
    wave_sync();
    const int n = wave_intersect_set(p.col + ru, a, p.col + rv, b, S);
    wave_sync();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    if (n >= 3) {
      unsigned long long cnt = 0;
      for (int k = 0; k < n; ++k) {
        const int c = S[k];
        const int rc = p.rp[c];
        cnt += wave_intersect_num(S, n, p.col + rc, p.rp[c + 1] - rc);
      }
      s[0] += cnt * (unsigned long long)(n - 2);
    }
    wave_sync();
  }
  block_add_u64<1>(s, p.out);
}

int wtri_per_cu(int stage) {
  const size_t lds = stage <= 1024 ? sizeof(WtriLds<1024>) : sizeof(WtriLds<kTctStageMax>);
  return (int)std::max<size_t>(1, std::min<size_t>(163840 / lds, 2048 / (kWtriWaves * GM_WAVE)));
}
hipError_t launch_wtri(const MineParams &p, const WtriParams &wp, int stage, int grid_blocks, hipStream_t stream) {
  static_assert(sizeof(WtriLds<kTctStageMax>) <= 65536, "a statically sized LDS block");
  static_assert(sizeof(HsWave<kTctStageMax>) * kWtriWaves >= (size_t)kTctStageMax * 2, "fill counters alias the wave scratch");
  if (!p.g.trp || !p.g.tdesc || !p.g.tedge || !wp.sup || !wp.ed || !wp.deg) return hipErrorInvalidValue;
  const dim3 grid((unsigned)grid_blocks), block(kWtriWaves * GM_WAVE);
  if (stage <= 1024) hipLaunchKernelGGL((wtri_kernel<1024>), grid, block, 0, stream, p, wp);
  else hipLaunchKernelGGL((wtri_kernel<kTctStageMax>), grid, block, 0, stream, p, wp);
  return hipGetLastError();
}
hipError_t launch_wtri_edges(const WtriEdgeParams &p, const WtriParams &wp, int cu_count, hipStream_t stream) {
  if (p.total <= 0) return hipSuccess;
  const long long blocks = std::min<long long>((p.total + 3) / 4, (long long)cu_count * 8);
  hipLaunchKernelGGL(wtri_edge_kernel, dim3((unsigned)std::max<long long>(1, blocks)), dim3(256), 0, stream, p, wp);
  return hipGetLastError();
}
hipError_t launch_wtri_degrees(int nv, long long ne, const int *rp, const int *col, int *deg, int cu_count, hipStream_t stream) {
  const long long cap = (long long)cu_count * 8;
  hipLaunchKernelGGL(wtri_outdeg_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(((long long)nv + 255) / 256, cap))), dim3(256), 0, stream, nv, rp, deg);
  if (ne > 0) hipLaunchKernelGGL(wtri_indeg_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>((ne + 255) / 256, cap))), dim3(256), 0, stream, ne, col, deg);
  return hipGetLastError();
}
hipError_t launch_wtri_entries(const WtriEntryParams &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(wtri_entry_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>((p.ne + 255) / 256, (long long)cu_count * 8))), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_wtri_vertices(int nv, const unsigned long long *tv2, const int *deg, unsigned long long *out, int cu_count, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  hipLaunchKernelGGL(wtri_vertex_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(((long long)nv + 255) / 256, (long long)cu_count * 8))), dim3(256), 0, stream, nv, tv2, deg, out);
  return hipGetLastError();
}
hipError_t launch_path5(int nv, const int *rp, const int *col, unsigned long long *out, int cu_count, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  hipLaunchKernelGGL(path5_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(((long long)nv + 3) / 4, (long long)cu_count * 8))), dim3(256), 0, stream, nv, rp, col, out);
  return hipGetLastError();
}
int chouse_grid(long long ne, int cu_count) { return (int)std::max<long long>(1, std::min<long long>((ne + 3) / 4, (long long)cu_count * 8)); }
hipError_t launch_chouse(const ChouseParams &p, int grid_blocks, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!p.scratch || p.max_deg <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(chouse_kernel, dim3((unsigned)grid_blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_wtri_kernel() {}
void gm_touch_wtri() { hipLaunchKernelGGL(gm_touch_wtri_kernel, dim3(1), dim3(1), 0, 0); }
