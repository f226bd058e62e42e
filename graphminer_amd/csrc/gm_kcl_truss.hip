// gm_kcl_truss.hip -- k-clique trusses (gm_clique_ktruss / gm_clique_truss_decompose; DESIGN.md "k-clique trusses"): the per-edge k-clique
// counts K_e of gm_clique_local, peeled in whole-frontier rounds on the caller's SYMMETRIC graph.  The state of an undirected edge sits at
// its canonical entry min(e, rev[e]), the one in the row of its smaller end (gm_local.hip).
//   ktr_init_kernel           the marks (canonical entries alive, the others removed for good); the smallest count of the graph
//   ktr_mark_kernel           a round, steps 1 + 2 (local_mark_kernel over 64-bit counts): last round's frontier becomes removed, the alive
//                             edges below the threshold become the frontier -- appended to a list through one atomic per wave, their
//                             theta and round written -- and the smallest count that stays is kept
//   ktr_peel_kernel<K>        step 3.  An edge is BLOCKED for frontier edge e when it is removed, or in the frontier at a canonical entry
//                             below e's.  e = (u, v) gathers S_e = the common neighbours w with neither (u, w) nor (v, w) blocked (the shorter
//                             row streamed, the longer bisected), builds Msym of S_e WITHOUT the blocked pairs and, with
//                             c_i = C_{K-3}(Msym_i) = the (K-2)-cliques of that graph that hold S_e[i], subtracts c_i from (u, w_i) and
//                             (v, w_i), c_ij = C_{K-4}(Msym_i & Msym_j) from (w_i, w_j) for every set pair -- each only outside the
//                             frontier -- and adds sum_i c_i / (K - 2) to the destroyed total.  The pairs are found by walking the rows of
//                             the survivors a second time, as the matrix was built: the walk has the entry at hand.  The path follows
//                             |S_e|: up to kKclLocalRegs2Row a wave per edge, up to kKclLocalLdsRow the workgroup, beyond that the list of
//   ktr_peel_wide_kernel<K>   which takes S_e, Msym and the waves' candidate sets out of the workgroup's slot of a global scratch
//                             (a wave per position, KclAny).  Slow and exact.
//   ktr_out_kernel            both directions of every edge: K_e inside the truss or GM_CORE_REMOVED, or theta and round mirrored from the
//                             canonical entry; the surviving edges and the sum of their counts
// The marks do not change while a peel kernel runs: every workgroup sees the state the round began with.  Two 64-bit atomics per member of
// S_e, one per adjacent pair of members, one per frontier edge; nothing per clique.  Plain vector loads and stores, atomicOr on the matrices.
#include "gm_kcl.h"

namespace gm {

constexpr int kKtrGrab = 4;  // frontier edges per dequeue of ktr_peel_kernel: one per wave on the wave path
constexpr unsigned long long kKtrNone = ~0ull;

__device__ __forceinline__ unsigned *ktr_queue(const KclTrussParams &p, const int w) { return reinterpret_cast<unsigned *>(p.words + 4) + w; }

// the smallest of one lane-private count per lane -> one atomic per workgroup (256 threads, every lane active): ~0 - m, so that 0 = none
__device__ __forceinline__ void ktr_block_least(unsigned long long least, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long part[4];
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)least, o, 64);
    least = other < least ? other : least;
  }
  if ((threadIdx.x & (GM_WAVE - 1)) == 0) part[threadIdx.x >> 6] = least;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = part[0];
    for (int w = 1; w < 4; ++w) m = part[w] < m ? part[w] : m;
    if (m != kKtrNone) atomicMax(out, kKtrNone - m);
  }
}

__global__ __launch_bounds__(256) void ktr_init_kernel(const KclTrussParams p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long least = kKtrNone;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < p.ne; e += stride) {
    const bool canonical = (long long)p.rev[e] > e;
    p.mark[e] = canonical ? LM_ALIVE : LM_REMOVED;
    if (canonical) {
      const unsigned long long c = p.cnt[e];
      least = c < least ? c : least;
    }
  }
  ktr_block_least(least, p.words + CW_LEAST);
}

__global__ __launch_bounds__(256) void ktr_mark_kernel(const KclTrussParams p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long least = kKtrNone;
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < p.ne; base += stride) {  // wave-uniform
    const long long c = base + lane;
    bool enters = false;
    if (c < p.ne && (long long)p.rev[c] > c) {  // a canonical entry
      const unsigned char m = p.mark[c];
      if (m == LM_FRONTIER) {
        p.mark[c] = LM_REMOVED;
      } else if (m == LM_ALIVE) {
        const unsigned long long s = p.cnt[c];
        enters = s < p.thr;
        if (enters) {
          p.mark[c] = LM_FRONTIER;
          if (p.theta) p.theta[c] = p.level;
          if (p.round) p.round[c] = p.round_no;
        } else {
          least = s < least ? s : least;
        }
      }
    }
    const unsigned long long bm = __ballot(enters);
    if (bm) {  // one atomic per wave: the leader reserves the slots of the list
      const int leader = readfirst((int)__builtin_ctzll(bm));
      int at = 0;
      if (lane == leader) at = (int)atomicAdd(&p.words[CW_FRONT], (unsigned long long)__popcll(bm));
      at = readlane(at, leader);
      if (enters) p.front[at + rank_below(bm)] = (int)c;
    }
  }
  ktr_block_least(least, p.words + CW_LEAST);
}

// canonical entry x is blocked for the frontier edge of canonical entry c
__device__ __forceinline__ bool ktr_blocked(const KclTrussParams &p, const int x, const int c) {
  const unsigned char m = p.mark[x];
  return m == LM_REMOVED || (m == LM_FRONTIER && x < c);
}
// the canonical entry of the edge (a, b), which exists: a bisection of the row of the smaller end
__device__ __forceinline__ int ktr_entry(const KclTrussParams &p, const int a, const int b) {
  const int x = min(a, b), r0 = p.rp[x];
  int pos = 0;
  contains(p.col + r0, p.rp[x + 1] - r0, max(a, b), &pos);
  return r0 + pos;
}

// the two rows of a frontier edge: the shorter one is streamed, the longer one bisected
struct KtrEdge {
  int c, sb, sn, lb, ln;
};
__device__ __forceinline__ KtrEdge ktr_edge(const KclTrussParams &p, const int c) {
  const int u = local_row_of(p.rp, p.nv, c), v = p.col[c];
  const int ru = p.rp[u], du = p.rp[u + 1] - ru, rv = p.rp[v], dv = p.rp[v + 1] - rv;
  const bool u_short = du <= dv;
  return KtrEdge{c, u_short ? ru : rv, u_short ? du : dv, u_short ? rv : ru, u_short ? dv : du};
}

// The members of S_e among the entries [r0, r1) of the shorter row, one wave, ascending: L[at0 + 0 ..] = w, E1 / E2 (may be nullptr) = the
// canonical entries of the edges from the two ends to w, as far as `cap` reaches (cap = 0: counted only).  Returns how many there are.
// Wave-uniform arguments, every lane active.
__device__ __forceinline__ int ktr_gather(const KclTrussParams &p, const KtrEdge &ed, const int r0, const int r1, int *L, int *E1, int *E2, const int at0,
                                          const int cap, const int lane) {
  int n = 0;
  for (int b = r0; b < r1; b += GM_WAVE) {
    const int es = b + lane;
    bool keep = false;
    int w = 0, cs = 0, cl = 0;
    if (es < r1) {
      w = p.col[es];
      int pos = 0;
      if (contains(p.col + ed.lb, ed.ln, w, &pos)) {
        const int el = ed.lb + pos;
        cs = min(es, p.rev[es]);
        cl = min(el, p.rev[el]);
        keep = !ktr_blocked(p, cs, ed.c) && !ktr_blocked(p, cl, ed.c);
      }
    }
    const unsigned long long bm = __ballot(keep);
    const int at = at0 + n + rank_below(bm);
    if (keep && at < cap) {
      L[at] = w;
      if (E1) {
        E1[at] = cs;
        E2[at] = cl;
      }
    }
    n += (int)__popcll(bm);
  }
  return n;
}
// ... of the whole shorter row by the four waves of a workgroup, a contiguous quarter each: counted, then written behind the quarters
// before it.  `part`: four ints in LDS.  Ends with a barrier; returns |S_e| (what lies beyond `cap` is not written).
__device__ __forceinline__ int ktr_gather_block(const KclTrussParams &p, const KtrEdge &ed, int *L, int *E1, int *E2, const int cap, int *part, const int wave,
                                                const int lane) {
  const int q = (ed.sn + 3) >> 2;
  const int r0 = ed.sb + min(wave * q, ed.sn), r1 = ed.sb + min((wave + 1) * q, ed.sn);
  const int mine = ktr_gather(p, ed, r0, r1, L, E1, E2, 0, 0, lane);
  if (lane == 0) part[wave] = mine;
  __syncthreads();
  int at0 = 0, d = 0;
  for (int w = 0; w < 4; ++w) {
    at0 += w < wave ? part[w] : 0;
    d += part[w];
  }
  if (d <= cap) ktr_gather(p, ed, r0, r1, L, E1, E2, at0, cap, lane);
  __syncthreads();
  return d;
}

// The adjacent pairs i < j of S_e (L: ascending, d members, in LDS) with the canonical entry x of (L[i], L[j]), the positions i = first,
// first + step, ... by one wave: the row of L[i] is streamed against L or, when it is much the longer list, L against it (kcl_build_msym_lds).
// L[i] < L[j], so the entry met in the row of L[i] is the canonical one.  f(i, j, x) runs in the lane that met the pair.
template <class F>
__device__ __forceinline__ void ktr_walk_pairs(const KclTrussParams &p, const int *__restrict__ L, const int d, const int first, const int step, const int lane,
                                               F f) {
  for (int i = first; i < d; i += step) {
    const int v = L[i], rv = p.rp[v], b = p.rp[v + 1] - rv;
    const bool stream_row = b <= 4 * d;
    const int n = stream_row ? b : d - (i + 1);
    for (int t = lane; t < n; t += GM_WAVE) {
      int pos = 0, x;
      bool hit;
      if (stream_row) {
        x = rv + t;
        hit = contains(L, d, p.col[x], &pos) && pos > i;
      } else {
        int at = 0;
        pos = i + 1 + t;
        hit = contains(p.col + rv, b, L[pos], &at);
        x = rv + at;
      }
      if (hit) f(i, pos, x);
    }
  }
}

// C_M(Msym_i): the (M + 1)-cliques of the matrix's graph that hold position i, the candidate set in KW registers
template <int M, int KW>
__device__ __forceinline__ unsigned long long ktr_value(const unsigned *__restrict__ msym, const int i, const int stride) {
  unsigned T[KW];
#pragma unroll
  for (int w2 = 0; w2 < KW; ++w2) T[w2] = (w2 < stride) ? msym[i * stride + w2] : 0u;
  return KclSmall<M, KW>::run(T, msym, stride);
}
// C_M(Msym_i & Msym_j): the (M + 2)-cliques that hold the positions i and j
template <int M, int KW>
__device__ __forceinline__ unsigned long long ktr_pair_value(const unsigned *__restrict__ msym, const int i, const int j, const int stride) {
  unsigned T[KW];
#pragma unroll
  for (int w2 = 0; w2 < KW; ++w2) T[w2] = (w2 < stride) ? (msym[i * stride + w2] & msym[j * stride + w2]) : 0u;
  return KclSmall<M, KW>::run(T, msym, stride);
}

// the matrix without the blocked pairs (zeroed; the caller puts a barrier behind it)
__device__ __forceinline__ void ktr_build_msym(const KclTrussParams &p, const int c, const int *__restrict__ L, const int d, const int stride,
                                               unsigned *__restrict__ msym, const int first, const int step, const int lane) {
  ktr_walk_pairs(p, L, d, first, step, lane, [&](const int i, const int j, const int x) {
    if (ktr_blocked(p, x, c)) return;
    atomicOr(&msym[i * stride + (j >> 5)], 1u << (j & 31));
    atomicOr(&msym[j * stride + (i >> 5)], 1u << (i & 31));
  });
}
// the pairs' decrements, K >= 4: every set pair whose edge is outside the frontier loses the cliques that hold both of its ends
template <int K, int KW>
__device__ __forceinline__ void ktr_pair_decrements(const KclTrussParams &p, const int *__restrict__ L, const int d, const int stride,
                                                    const unsigned *__restrict__ msym, const int first, const int step, const int lane) {
  if constexpr (K >= 4) {
    ktr_walk_pairs(p, L, d, first, step, lane, [&](const int i, const int j, const int x) {
      if (!((msym[i * stride + (j >> 5)] >> (j & 31)) & 1u) || p.mark[x] != LM_ALIVE) return;
      const unsigned long long val = ktr_pair_value<K - 4, KW>(msym, i, j, stride);
      if (val) atomicSub(&p.cnt[x], val);
    });
  }
}

// a frontier edge of up to kKclLocalRegs2Row survivors (L, E1, E2: n of them), one wave: msym = kKclLocalRegs2Row rows of two words
template <int K>
__device__ __forceinline__ void ktr_edge_wave(const KclTrussParams &p, const int c, const int *__restrict__ L, const int *__restrict__ E1,
                                              const int *__restrict__ E2, const int n, unsigned *__restrict__ msym, const int lane) {
  constexpr int KW = kKclLocalRegs2Row / 32;
  const int stride = (n + 31) >> 5;
  if (K >= 4) {
    for (int i = lane; i < n * stride; i += GM_WAVE) msym[i] = 0u;
    wave_sync();
    ktr_build_msym(p, c, L, n, stride, msym, 0, 1, lane);
    wave_sync();
  }
  unsigned long long val = 0;
  if (lane < n) {
    val = K >= 4 ? ktr_value<(K >= 4 ? K - 3 : 1), KW>(msym, lane, stride) : 1ull;  // (K = 3: every survivor closes one triangle, no matrix)
    if (val) {
      const int e1 = E1[lane], e2 = E2[lane];
      if (p.mark[e1] == LM_ALIVE) atomicSub(&p.cnt[e1], val);
      if (p.mark[e2] == LM_ALIVE) atomicSub(&p.cnt[e2], val);
    }
  }
  const unsigned long long sum = wave_sum_u64(val);
  if (lane == 0 && sum) atomicAdd(&p.words[CW_DESTROYED], sum / (unsigned long long)(K - 2));
  ktr_pair_decrements<K, KW>(p, L, n, stride, msym, 0, 1, lane);
  wave_sync();  // (the next edge rewrites the wave's share)
}

// a frontier edge of up to kKclLocalLdsRow survivors, the workgroup: S_e is gathered again by all four waves
template <int K>
__device__ __forceinline__ void ktr_edge_lds(const KclTrussParams &p, const KtrEdge &ed, unsigned *__restrict__ msym, int *__restrict__ L, int *__restrict__ E1,
                                             int *__restrict__ E2, int *__restrict__ part, int *__restrict__ next_pos, unsigned long long *__restrict__ total) {
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = tid >> 6;
  const int d = ktr_gather_block(p, ed, L, E1, E2, kKclLocalLdsRow, part, wave, lane);
  if (d > kKclLocalLdsRow) {  // (cannot happen: the marks do not change, the wave that counted S_e saw the same)
    if (tid == 0) atomicAdd(&p.words[CW_ERR], 1ull);
    return;
  }
  const int stride = (d + 31) >> 5;
  if (K >= 4)
    for (int i = tid; i < d * stride; i += 256) msym[i] = 0u;
  if (tid == 0) {
    *next_pos = 0;
    *total = 0ull;
  }
  __syncthreads();
  if (K >= 4) {
    ktr_build_msym(p, ed.c, L, d, stride, msym, wave, 4, lane);
    __syncthreads();
  }
  unsigned long long mine = 0;
  if (K >= 4) {
    constexpr int M = K >= 4 ? K - 3 : 1;
    for (;;) {  // a lane per position, taken off a counter: the descents differ in length
      const int i = atomicAdd(next_pos, 1);
      if (i >= d) break;
      // (workgroup-uniform: the registers a set takes follow |S_e| -- kKclLocalRegs8Row, kKclLocalRegs12Row)
      const unsigned long long val = stride <= kKclLocalRegs8Row / 32    ? ktr_value<M, kKclLocalRegs8Row / 32>(msym, i, stride)
                                     : stride <= kKclLocalRegs12Row / 32 ? ktr_value<M, kKclLocalRegs12Row / 32>(msym, i, stride)
                                                                         : ktr_value<M, kKclWords>(msym, i, stride);
      if (val == 0ull) continue;
      mine += val;
      const int e1 = E1[i], e2 = E2[i];
      if (p.mark[e1] == LM_ALIVE) atomicSub(&p.cnt[e1], val);
      if (p.mark[e2] == LM_ALIVE) atomicSub(&p.cnt[e2], val);
    }
  } else {
    for (int i = tid; i < d; i += 256) {
      mine += 1ull;
      const int e1 = E1[i], e2 = E2[i];
      if (p.mark[e1] == LM_ALIVE) atomicSub(&p.cnt[e1], 1ull);
      if (p.mark[e2] == LM_ALIVE) atomicSub(&p.cnt[e2], 1ull);
    }
  }
  const unsigned long long sum = wave_sum_u64(mine);
  if (lane == 0 && sum) atomicAdd(total, sum);
  if (stride <= kKclLocalRegs8Row / 32) ktr_pair_decrements<K, kKclLocalRegs8Row / 32>(p, L, d, stride, msym, wave, 4, lane);
  else if (stride <= kKclLocalRegs12Row / 32) ktr_pair_decrements<K, kKclLocalRegs12Row / 32>(p, L, d, stride, msym, wave, 4, lane);
  else ktr_pair_decrements<K, kKclWords>(p, L, d, stride, msym, wave, 4, lane);
  __syncthreads();
  if (tid == 0 && *total) atomicAdd(&p.words[CW_DESTROYED], *total / (unsigned long long)(K - 2));
  __syncthreads();  // (the next edge rewrites the LDS)
}

template <int K>
__global__ __launch_bounds__(256) void ktr_peel_kernel(const KclTrussParams p, const unsigned n_front) {
  __shared__ unsigned msym[kKclLocalLdsRow * kKclWords];  // the workgroup path's matrix; the wave path: wave w's at w * 2 * kKclLocalRegs2Row
  __shared__ int Ls[kKclLocalLdsRow];                     // S_e; the wave path: wave w's at w * kKclLocalRegs2Row
  __shared__ int E1s[kKclLocalLdsRow], E2s[kKclLocalLdsRow];  // the canonical entries of the edges from the two ends to S_e, shared the same way
  __shared__ unsigned long long total;
  __shared__ unsigned slot;
  __shared__ int next_pos, part[4], survivors[kKtrGrab];
  static_assert(kKtrGrab == 4 && 4 * kKclLocalRegs2Row <= kKclLocalLdsRow, "a wave per dequeued edge, its share inside the workgroup's arrays");
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = tid >> 6;
  for (;;) {
    if (tid == 0) slot = atomicAdd(ktr_queue(p, CQ_MAIN), (unsigned)kKtrGrab);
    __syncthreads();
    const unsigned q = slot;
    if (q >= n_front) break;
    {  // every wave its own edge: S_e is counted, and kept as far as the wave path reaches
      int n = 0;
      const int o = wave * kKclLocalRegs2Row;
      if (q + (unsigned)wave < n_front) {
        const KtrEdge ed = ktr_edge(p, p.front[q + wave]);
        n = ktr_gather(p, ed, ed.sb, ed.sb + ed.sn, Ls + o, E1s + o, E2s + o, 0, kKclLocalRegs2Row, lane);
        wave_sync();
        if (n >= K - 2 && n <= kKclLocalRegs2Row) ktr_edge_wave<K>(p, ed.c, Ls + o, E1s + o, E2s + o, n, msym + wave * 2 * kKclLocalRegs2Row, lane);
      }
      if (lane == 0) survivors[wave] = n;
    }
    __syncthreads();
    for (int j = 0; j < kKtrGrab; ++j) {  // workgroup-uniform: the edges of this dequeue beyond the wave path
      const int n = survivors[j];
      if (n <= kKclLocalRegs2Row) continue;
      const int c = p.front[q + j];
      if (n > kKclLocalLdsRow) {
        if (tid == 0) {
          const unsigned at = atomicAdd(ktr_queue(p, CQ_HEAVY), 1u);
          if (at < p.heavy_cap && p.scratch) p.heavy[at] = c;
          else atomicAdd(&p.words[CW_ERR], 1ull);  // (cannot happen: the list holds every edge, and a handle with a row this long has the
                                                   // wide kernel's scratch)
        }
        continue;
      }
      ktr_edge_lds<K>(p, ktr_edge(p, c), msym, Ls, E1s, E2s, part, &next_pos, &total);
    }
    __syncthreads();  // (the next dequeue rewrites `slot` and `survivors`)
  }
}

template <int K>
__global__ __launch_bounds__(256) void ktr_peel_wide_kernel(const KclTrussParams p) {
  static_assert(K - 3 <= kKclMaxLevels, "a set per level of the descent");
  __shared__ unsigned long long total;
  __shared__ unsigned slot;
  __shared__ int next_row, part[4];
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = tid >> 6;
  // the slot (kcl_local_scratch_words): 2 max_deg words -- S_e in the first max_deg of them --, the matrix, the four waves' set stacks
  unsigned *base = p.scratch + (size_t)blockIdx.x * p.scratch_words;
  int *L = reinterpret_cast<int *>(base);
  unsigned *msym = base + 2 * (size_t)p.max_deg;
  const unsigned n_heavy = min(*ktr_queue(p, CQ_HEAVY), p.heavy_cap);  // (complete: ktr_peel_kernel ran before this launch)
  for (;;) {
    if (tid == 0) {
      slot = atomicAdd(ktr_queue(p, CQ_WIDE), 1u);
      next_row = 0;
      total = 0ull;
    }
    __syncthreads();
    const unsigned q = slot;
    if (q >= n_heavy) break;
    const KtrEdge ed = ktr_edge(p, p.heavy[q]);
    const int u = local_row_of(p.rp, p.nv, ed.c), v = p.col[ed.c];
    const int d = ktr_gather_block(p, ed, L, nullptr, nullptr, p.max_deg, part, wave, lane);
    if (d > p.max_deg) {  // (cannot happen: the slot is sized by the handle's longest row)
      if (tid == 0) atomicAdd(&p.words[CW_ERR], 1ull);
      __syncthreads();
      continue;
    }
    const int stride = (d + 31) >> 5;
    unsigned *stk = msym + (size_t)d * stride + (size_t)wave * kKclMaxLevels * stride;
    for (size_t i = tid; i < (size_t)d * stride; i += 256) msym[i] = 0u;
    __threadfence();
    __syncthreads();
    for (int i = wave; i < d; i += 4) {  // the matrix without the blocked pairs: the row of L[i] against L, the pairs above i
      const int w = L[i], rw = p.rp[w], b = p.rp[w + 1] - rw;
      for (int t = lane; t < b; t += GM_WAVE) {
        int pos = 0;
        if (contains(L, d, p.col[rw + t], &pos) && pos > i && !ktr_blocked(p, rw + t, ed.c)) {
          atomicOr(&msym[(size_t)i * stride + (pos >> 5)], 1u << (pos & 31));
          atomicOr(&msym[(size_t)pos * stride + (i >> 5)], 1u << (i & 31));
        }
      }
    }
    __threadfence();
    __syncthreads();
    unsigned long long mine = 0;
    for (;;) {  // a wave per position, taken dynamically
      int i = 0;
      if (lane == 0) i = atomicAdd(&next_row, 1);
      i = readfirst(i);
      if (i >= d) break;
      const unsigned *Mi = msym + (size_t)i * stride;
      const unsigned long long val = wave_sum_u64(KclAny<K - 3>::run(Mi, stk, msym, stride, lane));
      if (val == 0ull) continue;
      mine += val;
      const int w = readfirst(L[i]);
      if (lane < 2) {  // (u, w) and (v, w)
        const int x = ktr_entry(p, lane == 0 ? u : v, w);
        if (p.mark[x] == LM_ALIVE) atomicSub(&p.cnt[x], val);
      }
      if constexpr (K >= 4) {  // the set pairs (i, j), j > i, one after the other
        for (int w0 = (i >> 5) & ~(GM_WAVE - 1); w0 < stride; w0 += GM_WAVE) {
          const int wi = w0 + lane;
          unsigned bits = wi < stride ? Mi[wi] : 0u;
          if (wi == (i >> 5)) bits &= 0xFFFFFFFEu << (i & 31);
          if (wi < (i >> 5)) bits = 0u;
          unsigned long long nz = __ballot(bits != 0u);
          while (nz) {  // wave-uniform
            const int ww = readfirst((int)__builtin_ctzll(nz));
            nz &= nz - 1ull;
            unsigned x = (unsigned)readlane((int)bits, ww);
            while (x) {
              const int j = (w0 + ww) * 32 + __ffs((int)x) - 1;
              x &= x - 1u;
              const int en = ktr_entry(p, w, readfirst(L[j]));
              if (p.mark[en] != LM_ALIVE) continue;
              const unsigned *Mj = msym + (size_t)j * stride;
              for (int w2 = lane; w2 < stride; w2 += GM_WAVE) stk[w2] = Mi[w2] & Mj[w2];
              const unsigned long long pv = wave_sum_u64(KclAny<(K >= 4 ? K - 4 : 0)>::run(stk, stk + stride, msym, stride, lane));
              if (lane == 0 && pv) atomicSub(&p.cnt[en], pv);
            }
          }
        }
      }
    }
    if (lane == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0 && total) atomicAdd(&p.words[CW_DESTROYED], total / (unsigned long long)(K - 2));
    __syncthreads();  // (the next edge rewrites the slot and the counters)
  }
}

__global__ __launch_bounds__(256) void ktr_out_kernel(const KclTrussParams p, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long part[2][4];
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long alive = 0, sum = 0;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < p.ne; e += stride) {
    const long long r = p.rev[e], c = min(e, r);
    if (p.theta) {  // the decomposition: the mark kernel wrote the canonical entries, the others take theirs
      if (r <= e) {
        p.theta[e] = r == e ? 0ull : p.theta[c];
        if (p.round) p.round[e] = r == e ? 0u : p.round[c];
      }
      continue;
    }
    const bool in = r != e && p.mark[c] == LM_ALIVE;
    const unsigned long long k = in ? p.cnt[c] : kKtrNone;
    if (out) out[e] = k;
    alive += (in && c == e) ? 1ull : 0ull;
    sum += (in && c == e) ? k : 0ull;
  }
  alive = wave_sum_u64(alive);
  sum = wave_sum_u64(sum);
  if ((threadIdx.x & (GM_WAVE - 1)) == 0) {
    part[0][threadIdx.x >> 6] = alive;
    part[1][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned long long t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
    if (t) atomicAdd(&p.words[threadIdx.x == 0 ? CW_ALIVE : CW_SUM], t);
  }
}

static inline dim3 ktr_grid(long long n, long long per_block, long long per_cu, int cu_count) {
  return dim3((unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, (long long)cu_count * per_cu)));
}
static bool ktr_params_ok(const KclTrussParams &p) {
  return p.rp && p.col && p.rev && p.cnt && p.mark && p.front && p.words && p.k >= 3 && p.k <= 8 && p.ne < (1ll << 31);
}

hipError_t launch_ktr_init(const KclTrussParams &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!ktr_params_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ktr_init_kernel, ktr_grid(p.ne, 256, 8, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_ktr_mark(const KclTrussParams &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!ktr_params_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ktr_mark_kernel, ktr_grid(p.ne, 256, 8, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}
template <int K>
static hipError_t launch_ktr_k(const KclTrussParams &p, bool wide, unsigned n_front, dim3 grid, hipStream_t stream) {
  if (wide) hipLaunchKernelGGL(ktr_peel_wide_kernel<K>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(ktr_peel_kernel<K>, grid, dim3(256), 0, stream, p, n_front);
  return hipGetLastError();
}
static hipError_t launch_ktr_any(const KclTrussParams &p, bool wide, unsigned n_front, dim3 grid, hipStream_t stream) {
  switch (p.k) {
    case 3: return launch_ktr_k<3>(p, wide, n_front, grid, stream);
    case 4: return launch_ktr_k<4>(p, wide, n_front, grid, stream);
    case 5: return launch_ktr_k<5>(p, wide, n_front, grid, stream);
    case 6: return launch_ktr_k<6>(p, wide, n_front, grid, stream);
    case 7: return launch_ktr_k<7>(p, wide, n_front, grid, stream);
    case 8: return launch_ktr_k<8>(p, wide, n_front, grid, stream);
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_ktr_peel(const KclTrussParams &p, unsigned n_front, int cu_count, hipStream_t stream) {
  if (n_front == 0) return hipSuccess;
  if (!ktr_params_ok(p) || !p.heavy || (long long)n_front > p.ne / 2) return hipErrorInvalidValue;
  return launch_ktr_any(p, false, n_front, ktr_grid(n_front, kKtrGrab, 4, cu_count), stream);
}
hipError_t launch_ktr_peel_wide(const KclTrussParams &p, int grid_blocks, hipStream_t stream) {
  if (grid_blocks < 1) return hipSuccess;
  if (!ktr_params_ok(p) || !p.heavy || !p.scratch || (p.scratch_words & 1ull)) return hipErrorInvalidValue;
  return launch_ktr_any(p, true, 0u, dim3((unsigned)grid_blocks), stream);
}
hipError_t launch_ktr_out(const KclTrussParams &p, unsigned long long *out, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!ktr_params_ok(p)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ktr_out_kernel, ktr_grid(p.ne, 256, 8, cu_count), dim3(256), 0, stream, p, out);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_kcl_truss_kernel() {}
void gm_touch_kcl_truss() { hipLaunchKernelGGL(gm_touch_kcl_truss_kernel, dim3(1), dim3(1), 0, 0); }
