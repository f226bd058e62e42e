// gm_clique_list.hip -- k-clique LISTING (gm_clique_list; DESIGN.md "k-clique listing"): every k-clique of a symmetric graph once, as k ids
// of the caller's numbering ascending, in an order that is fixed for (handle, k), windowed.  The walk is the local counts' (gm_kcl.h): per
// root u of the oriented copy the symmetric adjacency matrix Msym of L = N+(u), and over it the descent that picks the other k - 1 members
// as ascending positions i < l < j < ... of L.  The order: ascending root, then lexicographic on those positions.
//   kcl_list_count_kernel<K, WIDE>  COUNT: per entry (u, L[i]) the value c = C_{k-2}(Msym_i & {above i}) = sum over its pairs l of
//                                   v(i, l) = C_{k-3}(Msym_i & Msym_l & {above l}); an exclusive scan (hipCUB) over the entries turns the
//                                   values into every entry's first slot
//   kcl_list_fill_kernel<K, WIDE>   FILL: a root, then an entry, then a pair whose slots miss the window is skipped (a root before its matrix
//                                   is built).  A wave per entry: the pair values of 64 positions l at a time are scanned across the lanes,
//                                   a pair that meets the window is walked wave-uniformly down to its last level, whose members are
//                                   consecutive slots: slot = the pair's first slot + the rows before + rank_below of the ballot
// WIDE = false: rows of up to kKclLocalLdsRow entries, the matrix in LDS, a pair value by one lane out of registers (KclSmall).  WIDE = true:
// longer rows, any length, matrix and sets in the workgroup's slot of a global scratch, a pair value by the whole wave (KclAny).  The sets
// of the fill's walk lie in memory (LDS / the slot) and lane t owns the words t, t + 64, ... of each, as in KclAny.  Rows are queued in LDS (a
// ring of 128 rows per wave) and leave 64 at a time: 256 k contiguous bytes, k dword stores whose lanes cover neighbouring addresses,
// clipped to the window per int.  No atomic cursor, no global atomic on a count.  Plain HIP, vector stores only.
#include "gm_kcl.h"
#include "gm_scan.h"

namespace gm {

constexpr int kKclListGrab = 8;             // roots per dequeue of the LDS kernels
constexpr int kKclListRing = 2 * GM_WAVE;   // rows of a wave's ring

__device__ __forceinline__ unsigned long long kcl_readlane_u64(const unsigned long long v, const int l) {
  return ((unsigned long long)(unsigned)readlane((int)(unsigned)(v >> 32), l) << 32) | (unsigned)readlane((int)(unsigned)v, l);
}
// inclusive prefix sum of 64-bit values across the 64 lanes (all lanes active)
__device__ __forceinline__ unsigned long long kcl_wave_incl_scan_u64(unsigned long long v, const int lane) {
#pragma unroll
  for (int o = 1; o < GM_WAVE; o <<= 1) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, o, GM_WAVE), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), o, GM_WAVE);
    if (lane >= o) v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// the set of the pair (i, l): word w2 of Msym_i & Msym_l & {positions above l}
__device__ __forceinline__ unsigned kcl_list_pair_word(const unsigned *Mi, const unsigned *Ml, const int l, const int w2) {
  unsigned t = (w2 >= (l >> 5)) ? (Mi[w2] & Ml[w2]) : 0u;
  if (w2 == (l >> 5)) t &= 0xFFFFFFFEu << (l & 31);
  return t;
}
// v(i, l) by one lane, the set in KW registers (the matrix in LDS)
template <int M, int KW>
__device__ __forceinline__ unsigned long long kcl_list_pair_small(const unsigned *__restrict__ msym, const int i, const int l, const int stride) {
  unsigned T[KW];
#pragma unroll
  for (int w2 = 0; w2 < KW; ++w2) T[w2] = (w2 < stride) ? kcl_list_pair_word(msym + i * stride, msym + l * stride, l, w2) : 0u;
  return KclSmall<M, KW>::run(T, msym, stride);
}
// (workgroup-uniform: the registers a set takes follow the row's length -- kKclListRegs2Row, kKclListRegs8Row)
template <int M>
__device__ __forceinline__ unsigned long long kcl_list_pair_lane(const unsigned *__restrict__ msym, const int i, const int l, const int stride) {
  return stride <= kKclListRegs2Row / 32   ? kcl_list_pair_small<M, kKclListRegs2Row / 32>(msym, i, l, stride)
         : stride <= kKclListRegs8Row / 32 ? kcl_list_pair_small<M, kKclListRegs8Row / 32>(msym, i, l, stride)
                                           : kcl_list_pair_small<M, kKclWords>(msym, i, l, stride);
}
// v(i, l) by the whole wave, the set formed in stk (stride words; the levels below behind it).  The wave's sum.
template <int M>
__device__ __forceinline__ unsigned long long kcl_list_pair_any(const unsigned *msym, unsigned *stk, const int i, const int l, const int stride, const int lane) {
  const unsigned *Mi = msym + (size_t)i * stride, *Ml = msym + (size_t)l * stride;
  for (int w2 = lane; w2 < stride; w2 += GM_WAVE) stk[w2] = kcl_list_pair_word(Mi, Ml, l, w2);
  return wave_sum_u64(KclAny<M>::run(stk, stk + stride, msym, stride, lane));
}

// ---- COUNT --------------------------------------------------------------------------------------------------------------------------------
// One root with its matrix in LDS: the lanes take the words of the upper triangle from a counter in LDS, the pairs of a word add up in a
// register and then in the entry's sum in LDS; every entry gets one plain store.
template <int K>
__device__ __forceinline__ void kcl_list_count_root(const KclListParams &p, const int u, unsigned *__restrict__ msym, unsigned long long *__restrict__ acc,
                                                    int *__restrict__ Ls, int *__restrict__ next_word) {
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = tid >> 6;
  const int ru = p.rp[u], d = p.rp[u + 1] - ru;
  const int stride = (d + 31) >> 5;
  for (int i = tid; i < d * stride; i += 256) msym[i] = 0u;
  for (int i = tid; i < d; i += 256) {
    Ls[i] = p.col[ru + i];
    acc[i] = 0ull;
  }
  if (tid == 0) *next_word = 0;
  __syncthreads();
  kcl_build_msym_lds(p.rp, p.col, Ls, d, stride, msym, wave, lane);
  __syncthreads();
  const int nwords = d * stride;
  for (;;) {
    const int word = atomicAdd(next_word, 1);
    if (word >= nwords) break;
    const int i = word / stride, w = word - i * stride;
    if (w < (i >> 5)) continue;  // (below the diagonal)
    unsigned x = msym[word];
    if (w == (i >> 5)) x &= 0xFFFFFFFEu << (i & 31);  // the positions above i
    unsigned long long sum = 0;
    while (x) {
      const int l = w * 32 + (__ffs((int)x) - 1);
      x &= x - 1u;
      sum += kcl_list_pair_lane<K - 3>(msym, i, l, stride);
    }
    if (sum) atomicAdd(&acc[i], sum);  // (LDS)
  }
  __syncthreads();
  for (int i = tid; i < d; i += 256) p.cnt[ru + i] = acc[i];
  __syncthreads();  // (the next root rewrites the LDS)
}

// The roots a workgroup of a WIDE kernel takes from 256 consecutive vertices: those beyond the LDS matrix that `want` keeps, into list[]
template <class Want>
__device__ __forceinline__ int kcl_list_wide_roots(const KclListParams &p, const unsigned q, const int k, int *list, int *n_list, Want want) {
  const int tid = threadIdx.x;
  if (tid == 0) *n_list = 0;
  __syncthreads();
  const long long u = (long long)q + tid;
  if (u < p.nv) {
    const int d = p.rp[u + 1] - p.rp[u];
    if (d > kKclLocalLdsRow && d >= k - 1 && d <= p.max_deg && want((int)u, d)) list[atomicAdd(n_list, 1)] = (int)u;
  }
  __syncthreads();
  return *n_list;
}

template <int K, bool WIDE>
__global__ __launch_bounds__(256) void kcl_list_count_kernel(const KclListParams p) {
  __shared__ unsigned msym_s[WIDE ? 1 : kKclLocalLdsRow * kKclWords];
  __shared__ unsigned long long acc_s[WIDE ? 1 : kKclLocalLdsRow];
  __shared__ int Ls_s[WIDE ? 256 : kKclLocalLdsRow];  // WIDE: the roots of the dequeue
  __shared__ unsigned slot;
  __shared__ int next;
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = readfirst(tid >> 6);
  for (;;) {
    if (tid == 0) slot = atomicAdd(WIDE ? p.queue_wide : p.queue, WIDE ? 256u : (unsigned)kKclListGrab);
    __syncthreads();
    const unsigned q = slot;
    __syncthreads();  // (a dequeue whose roots are all skipped has no other barrier before the next one)
    if (q >= (unsigned)p.nv) break;
    if constexpr (!WIDE) {
      const int qe = (int)min(q + (unsigned)kKclListGrab, (unsigned)p.nv);
      for (int u = (int)q; u < qe; ++u) {
        const int d = p.rp[u + 1] - p.rp[u];
        if (d < K - 1 || d > kKclLocalLdsRow) continue;  // (workgroup-uniform: no k-clique is rooted here / the WIDE kernel's; cnt is zeroed)
        kcl_list_count_root<K>(p, u, msym_s, acc_s, Ls_s, &next);
      }
    } else {
      const int nr = kcl_list_wide_roots(p, q, K, Ls_s, &next, [](int, int) { return true; });
      unsigned *base = p.scratch + (size_t)blockIdx.x * p.scratch_words;
      unsigned *msym = base + 2 * (size_t)p.max_deg;  // (the slot's layout is the local counts': kcl_local_scratch_words)
      for (int r = 0; r < nr; ++r) {
        const int u = Ls_s[r];
        const int ru = p.rp[u], d = p.rp[u + 1] - ru;
        const int stride = (d + 31) >> 5;
        const int *L = p.col + ru;
        unsigned *stk = msym + (size_t)d * stride + (size_t)wave * kKclMaxLevels * stride;
        __syncthreads();  // (every wave has left the root before)
        for (size_t i = tid; i < (size_t)d * stride; i += 256) msym[i] = 0u;
        __threadfence();
        __syncthreads();
        kcl_build_msym_wide(p.rp, p.col, L, d, stride, msym, wave, lane);
        __threadfence();
        __syncthreads();
        // a wave per row i, dealt round robin.  NOT dequeued by lane 0 and broadcast: with a lane-0 store at the loop's end the compiler
        // threaded the two lane-0 branches across the back edge and left lanes 1 .. 63 in a loop of their own that never ends.
        for (int i = wave; i < d; i += 4) {
          const unsigned *Mi = msym + (size_t)i * stride;
          unsigned long long row_sum = 0;
          for (int w = i >> 5; w < stride; ++w) {
            unsigned x = (unsigned)readfirst((int)Mi[w]);  // (every lane reads the same word)
            if (w == (i >> 5)) x &= 0xFFFFFFFEu << (i & 31);
            while (x) {
              const int l = w * 32 + (__ffs((int)x) - 1);
              x &= x - 1u;
              row_sum += kcl_list_pair_any<K - 3>(msym, stk, i, l, stride, lane);
            }
          }
          p.cnt[ru + i] = row_sum;  // (every lane the same value to the same address: one store instruction, no lane-0 branch)
        }
      }
      __syncthreads();  // (the next dequeue rewrites the list)
    }
  }
}

// ---- FILL ---------------------------------------------------------------------------------------------------------------------------------
// A wave's queue of rows on their way out.  Everything but q's contents is wave-uniform.
template <int K>
struct KclListRing {
  int *q;                                // kKclListRing rows of K ints (LDS, the wave's own)
  int *out;
  unsigned long long first, end, slot0;  // the window [first, end); slot0: the slot of the ring's head
  int qn, qhead, lane, u;                // queued rows, the head (0 or 64), the root's id
  int pre[K - 2];                        // the ids of the members picked above the last level
  __device__ __forceinline__ bool past() const { return slot0 + (unsigned long long)qn >= end; }
  // rows [qhead, qhead + n) of the ring -> slots [slot0, slot0 + n): ints j, j + 64, ... of the run, clipped to the window
  __device__ __forceinline__ void flush(const int n) {
    const long long d0 = (long long)K * ((long long)slot0 - (long long)first), lim = (long long)K * (long long)(end - first);
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const int j = r * GM_WAVE + lane;
      const long long d = d0 + j;
      if (j < K * n && d >= 0 && d < lim) out[d] = q[K * qhead + j];
    }
  }
  __device__ __forceinline__ void finish() {
    wave_sync();
    flush(qn);
    wave_sync();
    qn = 0;
  }
  // the next row is slot b (rows were skipped: what is queued leaves first)
  __device__ __forceinline__ void seek(const unsigned long long b) {
    if (slot0 + (unsigned long long)qn != b) {
      finish();
      slot0 = b;
    }
  }
  // the lanes of m (a ballot; ascending lane = ascending slot) each add the row pre[] + last, the root's id inserted where it sorts
  __device__ __forceinline__ void emit(const unsigned long long m, const int last) {
    const int n = __popcll(m);
    if (n == 0) return;
    if (slot0 + (unsigned long long)(qn + n) <= first) {  // (all of it lies before the window)
      slot0 += (unsigned long long)(qn + n);
      qn = 0;
      return;
    }
    if ((m >> lane) & 1ull) {
      int at = K * ((qhead + qn + rank_below(m)) & (kKclListRing - 1));
      bool placed = false;
#pragma unroll
      for (int t = 0; t < K - 1; ++t) {
        const int id = t < K - 2 ? pre[t < K - 2 ? t : 0] : last;
        if (!placed && u < id) {
          q[at++] = u;
          placed = true;
        }
        q[at++] = id;
      }
      if (!placed) q[at] = u;
    }
    qn += n;
    if (qn >= GM_WAVE) {
      wave_sync();
      flush(GM_WAVE);
      wave_sync();
      qhead ^= GM_WAVE;
      qn -= GM_WAVE;
      slot0 += GM_WAVE;
    }
  }
};

// The last level: the members of a set are consecutive slots.  word(w): the lane's own word w of the set; 64 positions at a time the two
// words come back through readlane -- they ARE the ballot of the positions' lanes.
template <int K, class Word>
__device__ __forceinline__ void kcl_list_last(KclListRing<K> &ring, const int stride, const int *L, const int lane, Word word) {
  for (int w0 = 0; w0 < stride; w0 += GM_WAVE) {
    const unsigned mine = (w0 + lane < stride) ? word(w0 + lane) : 0u;
    if (__ballot(mine != 0u) == 0ull) continue;  // wave-uniform
    const int nw2 = min(GM_WAVE, stride - w0);
    for (int ww = 0; ww < nw2; ww += 2) {
      const unsigned long long set = ((unsigned long long)(unsigned)readlane((int)mine, ww + 1) << 32) | (unsigned)readlane((int)mine, ww);
      if (set == 0ull) continue;
      if (ring.past()) return;
      const bool found = (set >> lane) & 1ull;
      const unsigned long long m = __ballot(found);
      ring.emit(m, found ? L[(w0 + ww) * 32 + lane] : 0);
    }
  }
}

// The levels above it, wave-uniform: S picks member K - 1 - M of the row (M members are still to pick); the set below a member is formed in
// stk by the lanes that own its words.
template <int M, int K>
struct KclListWalk {
  static __device__ __forceinline__ void run(const unsigned *S, unsigned *stk, const unsigned *msym, const int stride, const int *L, const int lane,
                                             KclListRing<K> &ring) {
    for (int w0 = 0; w0 < stride; w0 += GM_WAVE) {
      const unsigned mine = (w0 + lane < stride) ? S[w0 + lane] : 0u;
      unsigned long long nz = __ballot(mine != 0u);
      while (nz) {  // wave-uniform
        const int ww = readfirst((int)__builtin_ctzll(nz));
        nz &= nz - 1ull;
        const int w = w0 + ww;
        unsigned x = (unsigned)readlane((int)mine, ww);
        while (x) {
          const int bit = __ffs((int)x) - 1;
          x &= x - 1u;
          if (ring.past()) return;
          const int j = w * 32 + bit;
          const unsigned *Mj = msym + (size_t)j * stride;
          for (int w2 = lane; w2 < stride; w2 += GM_WAVE) {
            unsigned t = (w2 >= w) ? (S[w2] & Mj[w2]) : 0u;
            if (w2 == w) t &= 0xFFFFFFFEu << bit;
            stk[w2] = t;
          }
          ring.pre[K - 1 - M] = readfirst(L[j]);
          KclListWalk<M - 1, K>::run(stk, stk + stride, msym, stride, L, lane, ring);
        }
      }
    }
  }
};
template <int K>
struct KclListWalk<1, K> {
  static __device__ __forceinline__ void run(const unsigned *S, unsigned *, const unsigned *, const int stride, const int *L, const int lane,
                                             KclListRing<K> &ring) {
    kcl_list_last<K>(ring, stride, L, lane, [&](const int w) { return S[w]; });
  }
};

// The entries of one root whose matrix is built (msym: LDS or the slot; L: the row, in LDS or in the CSR; stk: the wave's kKclMaxLevels
// sets): a wave per entry i, dealt round robin (wave-uniform).
template <int K, bool WIDE>
__device__ __forceinline__ void kcl_list_fill_entries(const KclListParams &p, const int u, const int ru, const int d, const int stride, const unsigned *msym,
                                                      const int *L, unsigned *stk, int *ringq, const int wave, const int lane) {
  KclListRing<K> ring;
  ring.q = ringq; ring.out = p.out; ring.first = p.first; ring.end = p.first + p.nw; ring.slot0 = 0;
  ring.qn = 0; ring.qhead = 0; ring.lane = lane; ring.u = u;
  const unsigned long long first = p.first, end = p.first + p.nw;
  for (int i = wave; i < d; i += 4) {
    const unsigned long long elo = p.off[ru + i], ehi = p.off[ru + i + 1];
    if (ehi <= first || elo >= end || elo == ehi) continue;  // (the entry misses the window, or holds nothing)
    ring.slot0 = elo;
    ring.pre[0] = readfirst(L[i]);
    const unsigned *Mi = msym + (size_t)i * stride;
    if constexpr (K == 3) {  // the entry's own set is the last level
      kcl_list_last<K>(ring, stride, L, lane, [&](const int w) {
        unsigned t = (w >= (i >> 5)) ? Mi[w] : 0u;
        if (w == (i >> 5)) t &= 0xFFFFFFFEu << (i & 31);
        return t;
      });
    } else {
      unsigned long long carried = elo;  // the first slot of the chunk's first pair
      for (int c = i >> 6; c * GM_WAVE < d && carried < end; ++c) {
        const int l = c * GM_WAVE + lane;
        const bool member = l < d && l > i && ((Mi[l >> 5] >> (l & 31)) & 1u);
        const unsigned long long members = __ballot(member);
        if (members == 0ull) continue;
        unsigned long long v = 0;
        if constexpr (!WIDE) {
          if (member) v = kcl_list_pair_lane<K - 3>(msym, i, l, stride);
        } else {
          for (unsigned long long mm = members; mm;) {  // wave-uniform
            const int src = readfirst((int)__builtin_ctzll(mm));
            mm &= mm - 1ull;
            const unsigned long long val = kcl_list_pair_any<K - 3>(msym, stk, i, c * GM_WAVE + src, stride, lane);
            if (lane == src) v = val;
          }
        }
        const unsigned long long incl = kcl_wave_incl_scan_u64(v, lane);
        const unsigned long long base = carried + (incl - v);  // exclusive: the pair's first slot
        unsigned long long need = __ballot(v != 0ull && base < end && base + v > first);
        while (need) {  // wave-uniform: the pairs that meet the window, ascending
          const int src = readfirst((int)__builtin_ctzll(need));
          need &= need - 1ull;
          const int l2 = c * GM_WAVE + src;
          ring.seek(kcl_readlane_u64(base, src));
          ring.pre[1 < K - 2 ? 1 : 0] = readfirst(L[l2]);
          const unsigned *Ml = msym + (size_t)l2 * stride;
          for (int w2 = lane; w2 < stride; w2 += GM_WAVE) stk[w2] = kcl_list_pair_word(Mi, Ml, l2, w2);
          KclListWalk<K - 3, K>::run(stk, stk + stride, msym, stride, L, lane, ring);
        }
        carried += kcl_readlane_u64(incl, GM_WAVE - 1);
      }
    }
    ring.finish();
  }
}

template <int K, bool WIDE>
__global__ __launch_bounds__(256) void kcl_list_fill_kernel(const KclListParams p) {
  constexpr int kLevels = K >= 4 ? K - 3 : 1;  // the pair's own set and the sets of the walk's levels
  static_assert(kLevels <= kKclMaxLevels, "a set per level of the walk");
  __shared__ unsigned msym_s[WIDE ? 1 : kKclLocalLdsRow * kKclWords];
  __shared__ int Ls_s[WIDE ? 256 : kKclLocalLdsRow];  // WIDE: the roots of the dequeue
  __shared__ unsigned stk_s[WIDE ? 1 : 4 * kLevels * kKclWords];
  __shared__ int ring_s[4 * kKclListRing * K];
  __shared__ unsigned slot;
  __shared__ int next;
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = readfirst(tid >> 6);
  const unsigned long long first = p.first, end = p.first + p.nw;
  int *ringq = ring_s + wave * kKclListRing * K;
  for (;;) {
    if (tid == 0) slot = atomicAdd(WIDE ? p.queue_wide : p.queue, WIDE ? 256u : (unsigned)kKclListGrab);
    __syncthreads();
    const unsigned q = slot;
    __syncthreads();  // (a dequeue whose roots are all skipped has no other barrier before the next one)
    if (q >= (unsigned)p.nv) break;
    if constexpr (!WIDE) {
      const int qe = (int)min(q + (unsigned)kKclListGrab, (unsigned)p.nv);
      for (int u = (int)q; u < qe; ++u) {
        const int ru = p.rp[u], d = p.rp[u + 1] - ru;
        if (d < K - 1 || d > kKclLocalLdsRow) continue;  // (workgroup-uniform)
        const unsigned long long lo = p.off[ru], hi = p.off[ru + d];
        if (hi <= first || lo >= end || lo == hi) continue;  // (the root misses the window: its matrix is not built)
        const int stride = (d + 31) >> 5;
        for (int i = tid; i < d * stride; i += 256) msym_s[i] = 0u;
        for (int i = tid; i < d; i += 256) Ls_s[i] = p.col[ru + i];
        __syncthreads();
        kcl_build_msym_lds(p.rp, p.col, Ls_s, d, stride, msym_s, wave, lane);
        __syncthreads();
        kcl_list_fill_entries<K, false>(p, u, ru, d, stride, msym_s, Ls_s, stk_s + wave * kLevels * kKclWords, ringq, wave, lane);
        __syncthreads();  // (the next root rewrites the LDS)
      }
    } else {
      const int nr = kcl_list_wide_roots(p, q, K, Ls_s, &next, [&](const int u, const int d) {
        const unsigned long long lo = p.off[p.rp[u]], hi = p.off[p.rp[u] + d];
        return !(hi <= first || lo >= end || lo == hi);
      });
      unsigned *base = p.scratch + (size_t)blockIdx.x * p.scratch_words;
      unsigned *msym = base + 2 * (size_t)p.max_deg;
      for (int r = 0; r < nr; ++r) {
        const int u = Ls_s[r];
        const int ru = p.rp[u], d = p.rp[u + 1] - ru;
        const int stride = (d + 31) >> 5;
        const int *L = p.col + ru;
        unsigned *stk = msym + (size_t)d * stride + (size_t)wave * kKclMaxLevels * stride;
        __syncthreads();  // (every wave has left the root before)
        for (size_t i = tid; i < (size_t)d * stride; i += 256) msym[i] = 0u;
        __threadfence();
        __syncthreads();
        kcl_build_msym_wide(p.rp, p.col, L, d, stride, msym, wave, lane);
        __threadfence();
        __syncthreads();
        kcl_list_fill_entries<K, true>(p, u, ru, d, stride, msym, L, stk, ringq, wave, lane);
      }
      __syncthreads();  // (the next dequeue rewrites the list)
    }
  }
}

template <int K>
static hipError_t launch_kcl_list_k(const KclListParams &p, bool fill, int grid, int grid_wide, hipStream_t stream) {
  if (!fill) {
    hipLaunchKernelGGL((kcl_list_count_kernel<K, false>), dim3(grid), dim3(256), 0, stream, p);
    if (grid_wide > 0) hipLaunchKernelGGL((kcl_list_count_kernel<K, true>), dim3(grid_wide), dim3(256), 0, stream, p);
  } else {
    hipLaunchKernelGGL((kcl_list_fill_kernel<K, false>), dim3(grid), dim3(256), 0, stream, p);
    if (grid_wide > 0) hipLaunchKernelGGL((kcl_list_fill_kernel<K, true>), dim3(grid_wide), dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}
static hipError_t launch_kcl_list(const KclListParams &p, bool fill, int grid, int grid_wide, hipStream_t stream) {
  if (p.nv <= 0 || p.ne <= 0) return hipSuccess;
  if (grid < 1 || grid_wide < 0 || !p.rp || !p.col || !p.queue || !p.queue_wide || (fill ? (!p.off || !p.out) : !p.cnt) ||
      (grid_wide > 0 && (!p.scratch || (p.scratch_words & 1ull))))
    return hipErrorInvalidValue;
  switch (p.k) {
    case 3: return launch_kcl_list_k<3>(p, fill, grid, grid_wide, stream);
    case 4: return launch_kcl_list_k<4>(p, fill, grid, grid_wide, stream);
    case 5: return launch_kcl_list_k<5>(p, fill, grid, grid_wide, stream);
    case 6: return launch_kcl_list_k<6>(p, fill, grid, grid_wide, stream);
    case 7: return launch_kcl_list_k<7>(p, fill, grid, grid_wide, stream);
    case 8: return launch_kcl_list_k<8>(p, fill, grid, grid_wide, stream);
    default: return hipErrorInvalidValue;
  }
}

hipError_t kcl_list_count_scan(const KclListParams &p, unsigned long long *off, int grid, int grid_wide, hipStream_t stream) {
  if (p.ne <= 0 || !off) return hipErrorInvalidValue;
  DevBuf<unsigned long long> cnt;
  ScanTemp tmp;
  hipError_t e = cnt.alloc((size_t)p.ne + 1);
  if (e != hipSuccess) return e;
  // (the entries of the roots no kernel takes -- fewer than k - 1 out-neighbours -- and the value behind the last entry)
  if ((e = hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * ((size_t)p.ne + 1), stream)) != hipSuccess) return e;
  KclListParams q = p;
  q.cnt = cnt.p;
  if ((e = launch_kcl_list(q, false, grid, grid_wide, stream)) != hipSuccess) return e;
  if ((e = dev_exclusive_sum(tmp, cnt.p, off, (size_t)p.ne + 1, stream)) != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

hipError_t launch_kcl_list_fill(const KclListParams &p, int grid, int grid_wide, hipStream_t stream) {
  if (p.nw == 0) return hipSuccess;
  return launch_kcl_list(p, true, grid, grid_wide, stream);
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_clique_list_kernel() {}
void gm_touch_clique_list() { hipLaunchKernelGGL(gm_touch_clique_list_kernel, dim3(1), dim3(1), 0, 0); }
