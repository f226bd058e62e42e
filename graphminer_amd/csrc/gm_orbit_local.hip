// gm_orbit_local.hip -- the kernels of gm_motif_local's own (DESIGN.md "Local motif counts"): the graphlet-degree orbits of every vertex.
// Everything else the call needs -- t(e), T_v, R_v, K_v -- comes from the three local counts (gm_local.hip, gm_rect_local.hip,
// gm_kcl_local.hip).  With x(e) = t(e) - 1:
//   credit_kernel       the DIAMOND-RIM credits W(e) = sum over the triangles of e of the x of their other two edges: a second pass over
//                       the triangles of the oriented copy, wtri_kernel's walk (gm_wtri.hip) -- the task lists of the edge supports, the host
//                       row as a hashed set in LDS, a match knows its three DAG entries eo (the task's own), eh (host row start +
//                       position), es (the index of the streamed key) -- that adds instead of summing:
//                         W[eh] += x(eo) + x(es),  W[es] += x(eo) + x(eh)   one 64-bit atomic each, result unused
//                         W[eo] += x(eh) + x(es)                            gathered per batch lane in LDS, ONE atomic per task
//   credit_edge_kernel  the same credits for the out-edges no task list holds (rows beyond the 2048-entry stage, or the rows of the hub
//                       corner): one wave per edge, the longer list bisected in global memory; the own edge's credit summed over the wave
//   orbit_e1_kernel     on the CALLER's symmetric CSR: e1(v) = sum_{a in N(v)} (d(a) - 1)
//   orbit_finish_kernel the neighbour sums of row v, the non-induced counts N[0 .. 14], gm_orbits_from_noninduced (gm_orbit.h: the one
//                       coefficient table), the orbit-major writes, and the column sums the motif counts need (one atomic per workgroup
//                       and sum); K4 = false: orbits 0 .. 3 from e1 and T_v alone, in one gather
// The two row kernels take 64 consecutive rows per wave: a lane sums its own short row, a row of more than kOrbitWaveRow entries is summed
// by the whole wave (local_vertex_kernel's split).  uint64 arithmetic modulo 2^64; plain HIP atomics and vector stores only.
#include "gm_hset.h"
#include "gm_orbit.h"

namespace gm {

constexpr int kCreditWaves = 4;
constexpr int kCreditTiles = 2;

template <int STAGE>
struct alignas(16) CreditLds {
  HsTable<STAGE> set;
  int trpl[kMaxChunkVerts + 1];   // row offsets of the chunk's task lists
  HsWave<STAGE> w[kCreditWaves];  // (while the set is built: the fill counters of its buckets)
  unsigned long long own[kCreditWaves][GM_WAVE];  // per batch lane: the credit its task's own entry has gathered
  unsigned xo[kCreditWaves][GM_WAVE];             // per batch lane: x of its task's own entry
  int next_batch;
  unsigned queue_pos;
  int pad_[2];
};

template <int STAGE>
__global__ __launch_bounds__((kCreditWaves * GM_WAVE), 2)
void credit_kernel(const MineParams p, const CreditParams cp) {
  __shared__ CreditLds<STAGE> B;
  using H = HsHash<STAGE>;
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const int wave = threadIdx.x >> 6;
  const int tid = threadIdx.x;
  constexpr int nthreads = kCreditWaves * GM_WAVE;
  const int *__restrict__ rp = p.g.rp;
  const int *__restrict__ col = p.g.col;
  const int *__restrict__ trp = p.g.trp;
  const int2 *__restrict__ tdesc = p.g.tdesc;
  const int *__restrict__ tedge = p.g.tedge;
  const unsigned *__restrict__ sup = cp.sup;
  unsigned long long *__restrict__ W = cp.w;
  HsWave<STAGE> &L = B.w[wave];
  unsigned long long *own = B.own[wave];
  unsigned *xo = B.xo[wave];
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
        own[lane] = 0ull;
        xo[lane] = act ? sup[own_e] - 1u : 0u;  // (a task with a match has t >= 1)
        wave_sync();
        // the two per-task words handed back with a match: word = the DAG entry the host's row starts at, word2 = the task's batch lane
        auto hit = [&](const unsigned long long hm, const int word, const int word2, const unsigned at, const int kidx, const bool uniform) {
          if (hm == 0ull) return;  // wave-uniform
          const bool mine = __builtin_amdgcn_inverse_ballot_w64(hm);
          unsigned long long c = 0ull;
          if (mine) {
            const int eh = word + (int)at, es = kidx;
            const unsigned long long x0 = xo[word2], xh = (unsigned long long)sup[eh] - 1ull, xs = (unsigned long long)sup[es] - 1ull;
            atomicAdd(&W[eh], x0 + xs);
            atomicAdd(&W[es], x0 + xh);
            c = xh + xs;
          }
          if (uniform) {  // a tile of ONE task (long lists): its own credit summed over the wave
            c = wave_sum_u64(c);
            if (lane == 0 && c) atomicAdd(&own[word2], c);
          } else if (mine) {
            atomicAdd(&own[word2], c);
          }
        };
        auto hit1 = [&](const int word, const int word2, const int at, const int kidx) {  // one key found through the surplus list (wave-uniform)
          if (lane == 0) {
            const int eh = word + at, es = kidx;
            const unsigned long long x0 = xo[word2], xh = (unsigned long long)sup[eh] - 1ull, xs = (unsigned long long)sup[es] - 1ull;
            atomicAdd(&W[eh], x0 + xs);
            atomicAdd(&W[es], x0 + xh);
            atomicAdd(&own[word2], xh + xs);
          }
        };
        hs_pass<STAGE, kCreditTiles>(B.set, L, col, fallback, lane, act ? d.y : 0, d.x, H::salt(lo), ru - eb, a, ru, lane, hit, hit1);
        wave_sync();
        const unsigned long long c = own[lane];
        if (valid && c) atomicAdd(&W[own_e], c);  // the own edge's credit: once per task
        wave_sync();
      }
      __syncthreads();  // every wave is done with the chunk: the set is rewritten by the next one
    }
  }
}

// One wave per out-edge u -> v of the rows no task list holds (wtri_edge_kernel's walk): `rows` / `prefix` name them (the rows beyond the
// stage), or -- rows == nullptr -- they are the rows from `v0` on (the hub corner; total: an upper bound for the grid).
__global__ __launch_bounds__(256) void credit_edge_kernel(const WtriEdgeParams p, const CreditParams cp) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const unsigned *__restrict__ sup = cp.sup;
  unsigned long long *__restrict__ W = cp.w;
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
    const unsigned long long x0 = (unsigned long long)sup[e] - 1ull;  // (used only with a match: t >= 1 then)
    unsigned long long c = 0ull;
    for (int k = lane; k < sn; k += GM_WAVE) {
      const int key = p.col[sbase + k];
      const int pos = lower_bound(p.col + lbase, ln, key);
      if (pos < ln && p.col[lbase + pos] == key) {
        const int e1 = lbase + pos, e2 = sbase + k;
        const unsigned long long x1 = (unsigned long long)sup[e1] - 1ull, x2 = (unsigned long long)sup[e2] - 1ull;
        atomicAdd(&W[e1], x0 + x2);
        atomicAdd(&W[e2], x0 + x1);
        c += x1 + x2;
      }
    }
    c = wave_sum_u64(c);
    if (lane == 0 && c) atomicAdd(&W[e], c);
  }
}

// ---- the row kernels on the caller's symmetric CSR ------------------------------------------------------------------------------------------
// block-wide sums of n lane-private 64-bit values -> one atomic per workgroup and sum (256 threads, every lane active)
template <int N>
__device__ __forceinline__ void orbit_block_add(const unsigned long long (&v)[N], unsigned long long *__restrict__ out) {
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

__device__ __forceinline__ unsigned long long orbit_choose2(const unsigned long long x) {  // C(x, 2) mod 2^64: the even factor is halved first
  if (x < 2ull) return 0ull;
  return (x & 1ull) ? x * ((x - 1ull) >> 1) : (x >> 1) * (x - 1ull);
}
__device__ __forceinline__ unsigned long long orbit_choose3(const unsigned long long x) {  // C(x, 3) mod 2^64: the factors are divided before the product
  if (x < 3ull) return 0ull;
  unsigned long long f[3] = {x, x - 1ull, x - 2ull};
  if (f[0] & 1ull) f[1] >>= 1; else f[0] >>= 1;  // (x - 1 is even when x is odd)
  const int r = (int)(x % 3ull);                 // x - r is the multiple of 3
  f[r] /= 3ull;
  return f[0] * f[1] * f[2];
}

// The sums of NS terms over every row of a wave's 64 consecutive rows: term(j, t) adds entry j's NS terms to t.  Lane l returns the sums of
// row base + l (zeros beyond nv).  Wave-uniform control flow: every lane of the wave calls it.
template <int NS, class Term>
__device__ __forceinline__ void orbit_row_sums(const int r0, const int r1, const int lane, Term term, unsigned long long (&s)[NS]) {
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0ull;
  if (r1 - r0 <= kOrbitWaveRow)
    for (int j = r0; j < r1; ++j) term(j, s);
  unsigned long long longs = __ballot(r1 - r0 > kOrbitWaveRow);
  while (longs) {  // wave-uniform
    const int l = readfirst((int)__builtin_ctzll(longs));
    longs &= longs - 1ull;
    const int b = readlane(r0, l), e = readlane(r1, l);
    unsigned long long part[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) part[k] = 0ull;
    for (int j = b + lane; j < e; j += GM_WAVE) term(j, part);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const unsigned long long t = wave_sum_u64(part[k]);
      if (lane == l) s[k] = t;
    }
  }
}

__global__ __launch_bounds__(256) void orbit_e1_kernel(int nv, const int *__restrict__ rp, const int *__restrict__ col, unsigned long long *__restrict__ e1) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long base = wave0 * GM_WAVE; base < nv; base += nwaves * GM_WAVE) {
    const long long v = base + lane;
    const int r0 = v < nv ? rp[v] : 0, r1 = v < nv ? rp[v + 1] : 0;
    unsigned long long s[1];
    orbit_row_sums<1>(r0, r1, lane, [&](const int j, unsigned long long (&t)[1]) {
      const int a = col[j];
      t[0] += (unsigned long long)(unsigned)(rp[a + 1] - rp[a]) - 1ull;
    }, s);
    if (v < nv) e1[v] = s[0];
  }
}

template <bool K4>
__global__ __launch_bounds__(256) void orbit_finish_kernel(const OrbitFinishParams p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  const int *__restrict__ rp = p.rp;
  const int *__restrict__ col = p.col;
  constexpr int NC = K4 ? 6 : 2;
  unsigned long long cs[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) cs[k] = 0ull;
  const size_t nv = (size_t)p.nv;
  for (long long base = wave0 * GM_WAVE; base < p.nv; base += nwaves * GM_WAVE) {
    const long long v = base + lane;
    const bool in = v < p.nv;
    const int r0 = in ? rp[v] : 0, r1 = in ? rp[v + 1] : 0;
    const unsigned long long d = (unsigned long long)(unsigned)(r1 - r0);
    const unsigned long long tv = in ? p.tv[v] : 0ull;
    if constexpr (!K4) {
      unsigned long long s[1];
      orbit_row_sums<1>(r0, r1, lane, [&](const int j, unsigned long long (&t)[1]) {
        const int a = col[j];
        t[0] += (unsigned long long)(unsigned)(rp[a + 1] - rp[a]) - 1ull;
      }, s);
      if (in) {
        const unsigned long long o1 = s[0] - 2ull * tv, o2 = orbit_choose2(d) - tv;
        if (p.orbits) {
          p.orbits[v] = d;
          p.orbits[nv + v] = o1;
          p.orbits[2 * nv + v] = o2;
          p.orbits[3 * nv + v] = tv;
        }
        cs[0] += o2;
        cs[1] += tv;
      }
    } else {
      unsigned long long s[5];  // sum e1(a), sum C(d(a) - 1, 2), sum T_a, sum t(va) (d(a) - 2), sum C(t(va), 2)
      orbit_row_sums<5>(r0, r1, lane, [&](const int j, unsigned long long (&t)[5]) {
        const int a = col[j];
        const unsigned long long da = (unsigned long long)(unsigned)(rp[a + 1] - rp[a]), te = p.ent[j];
        t[0] += p.e1[a];
        t[1] += orbit_choose2(da - 1ull);
        t[2] += p.tv[a];
        t[3] += te * (da - 2ull);  // (t > 0 implies d(a) >= 2; else the product is 0 modulo 2^64)
        t[4] += orbit_choose2(te);
      }, s);
      if (in) {
        const unsigned long long e1 = p.e1[v];
        uint64_t N[kOrbits4], o[kOrbits4];
        N[0] = d;
        N[1] = e1 - 2ull * tv;
        N[2] = orbit_choose2(d) - tv;
        N[3] = tv;
        N[4] = s[0] - d * (d - 1ull) - 2ull * tv;
        N[5] = (d - 1ull) * e1 - 2ull * tv;
        N[6] = s[1];
        N[7] = orbit_choose3(d);
        N[8] = p.rv[v];
        N[9] = s[2] - 2ull * tv;
        N[10] = s[3];
        N[11] = tv * (d - 2ull);
        N[13] = s[4];
        N[12] = p.w2[v] - N[13];  // (w2: half the row sum of the rim credits)
        N[14] = p.kv[v];
        gm_orbits_from_noninduced(N, o);
        if (p.orbits) {
#pragma unroll
          for (int k = 0; k < kOrbits4; ++k) p.orbits[(size_t)k * nv + v] = o[k];
        }
        cs[0] += o[7];
        cs[1] += o[4];
        cs[2] += o[9];
        cs[3] += o[8];
        cs[4] += o[13];
        cs[5] += o[14];
      }
    }
  }
  orbit_block_add<NC>(cs, p.sums);
}

int credit_per_cu(int stage) {
  const size_t lds = stage <= 1024 ? sizeof(CreditLds<1024>) : sizeof(CreditLds<kTctStageMax>);
  return (int)std::max<size_t>(1, std::min<size_t>(163840 / lds, 2048 / (kCreditWaves * GM_WAVE)));
}
hipError_t launch_credit(const MineParams &p, const CreditParams &cp, int stage, int grid_blocks, hipStream_t stream) {
  static_assert(sizeof(CreditLds<kTctStageMax>) <= 65536, "a statically sized LDS block");
  static_assert(sizeof(HsWave<kTctStageMax>) * kCreditWaves >= (size_t)kTctStageMax * 2, "fill counters alias the wave scratch");
  if (!p.g.trp || !p.g.tdesc || !p.g.tedge || !cp.sup || !cp.w) return hipErrorInvalidValue;
  const dim3 grid((unsigned)grid_blocks), block(kCreditWaves * GM_WAVE);
  if (stage <= 1024) hipLaunchKernelGGL((credit_kernel<1024>), grid, block, 0, stream, p, cp);
  else hipLaunchKernelGGL((credit_kernel<kTctStageMax>), grid, block, 0, stream, p, cp);
  return hipGetLastError();
}
hipError_t launch_credit_edges(const WtriEdgeParams &p, const CreditParams &cp, int cu_count, hipStream_t stream) {
  if (p.total <= 0) return hipSuccess;
  if (!cp.sup || !cp.w) return hipErrorInvalidValue;
  const long long blocks = std::min<long long>((p.total + 3) / 4, (long long)cu_count * 8);
  hipLaunchKernelGGL(credit_edge_kernel, dim3((unsigned)std::max<long long>(1, blocks)), dim3(256), 0, stream, p, cp);
  return hipGetLastError();
}
static inline dim3 orbit_grid(long long nv, int cu_count) {
  return dim3((unsigned)std::max<long long>(1, std::min<long long>((nv + 255) / 256, (long long)cu_count * 8)));
}
hipError_t launch_orbit_e1(int nv, const int *rp, const int *col, unsigned long long *e1, int cu_count, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  if (!e1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(orbit_e1_kernel, orbit_grid(nv, cu_count), dim3(256), 0, stream, nv, rp, col, e1);
  return hipGetLastError();
}
hipError_t launch_orbit_finish(const OrbitFinishParams &p, int k, int cu_count, hipStream_t stream) {
  if (p.nv <= 0) return hipSuccess;
  if (!p.tv || !p.sums || (k == 4 && (!p.ent || !p.e1 || !p.rv || !p.kv || !p.w2))) return hipErrorInvalidValue;
  if (k == 4) hipLaunchKernelGGL((orbit_finish_kernel<true>), orbit_grid(p.nv, cu_count), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((orbit_finish_kernel<false>), orbit_grid(p.nv, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_orbit_local_kernel() {}
void gm_touch_orbit_local() { hipLaunchKernelGGL(gm_touch_orbit_local_kernel, dim3(1), dim3(1), 0, 0); }
