// gm_kcl_local.hip -- local k-clique counts (gm_clique_local; DESIGN.md "Local k-clique counts"): the number of k-cliques on every entry
// of the DAG the call runs on, one uint64 per entry.  Cliques are ATTRIBUTED, not summed: for a root u with out-list L = N+(u), Msym is
// the symmetric adjacency of L inside L (a bit-matrix, row i = the positions of L adjacent to L[i]), and with
//   C_0 = 1,  C_1(S) = |S|,  C_m(S) = sum_{j in S} C_{m-1}(S & Msym_j & {positions above j})
// every k-clique whose lowest vertex (in the DAG's order) is u is counted
//   on the inner edge (L[i], L[l]) of every adjacent pair i < l -- every DAG triangle (u, i, l) once -- by C_{k-3}(Msym_i & Msym_l),
//   on the spoke (u, L[i]) by C_{k-2}(Msym_i) = (sum of the inner values of the pairs that hold i) / (k - 2): a (k-1)-clique of L that
//   holds i has k - 2 other members, so the spokes cost a sum, not a second descent.
// One 64-bit atomicAdd per DAG triangle and one per (root, spoke); nothing per clique.  All integer.
//   kcl_local_kernel<K, false> rows of up to kKclLocalLdsRow entries: a workgroup per root, Msym and the spoke sums in LDS, the lanes take the
//                             pairs one at a time off the words of the upper triangle, the candidate set of a descent in 2, 8, 12 or 16
//                             registers per level (rows of up to 64, 256, 384, 512 entries).  Rows beyond the LDS matrix are appended to
//                             the wide kernel's list, and for k >= 5 the rows beyond kKclLocalSplitRow entries -- few, and the descents
//                             below them long -- to the list of
//   kcl_local_kernel<K, true>  which gives each of them to kKclParts workgroups and each pair to a whole wave (the members of the pair's
//                             set dealt to the lanes)
//   kcl_local_fold_kernel     the spoke sums arrive undivided in an array of their own (the shares of a root add up first): + sum / (k - 2)
//   kcl_local_wide_kernel<K>  the rows of that list, any length: Msym, the spoke sums and the waves' candidate sets in the workgroup's
//                             slot of a global scratch; a wave per row i, every lane owns the words w = lane (mod 64) of a set, so a lane
//                             reads back only what it wrote itself.  Slow and exact.
// Plain vector loads and stores, atomicOr on the matrices, atomicAdd(unsigned long long) on the counts.
#include "gm_kcl.h"

namespace gm {

constexpr int kKclGrab = 8;                      // roots per dequeue of kcl_local_kernel
constexpr int kKclParts = 16;                    // workgroups per split root

// the DAG entry of the edge {a, b}: in the row of one of its ends (-1: not an edge -- cannot happen for an adjacent pair)
__device__ __forceinline__ int kcl_entry(const int *__restrict__ rp, const int *__restrict__ col, const int a, const int b) {
  int r0 = rp[a], pos = 0;
  if (contains(col + r0, rp[a + 1] - r0, b, &pos)) return r0 + pos;
  r0 = rp[b];
  if (contains(col + r0, rp[b + 1] - r0, a, &pos)) return r0 + pos;
  return -1;
}

// the position of `key` in the ascending list col[r0 .. r0 + n), searched by the whole wave: 64 probes narrow the list to a 64th, a list
// of at most 64 keys is read once (-1: not there).  Wave-uniform arguments, every lane active.
__device__ __forceinline__ int kcl_wave_find(const int *__restrict__ col, const int r0, const int n, const int key, const int lane) {
  int lo = 0, hi = n;  // the key, if present, lies in [lo, hi)
  while (hi - lo > GM_WAVE) {
    const int step = (hi - lo + GM_WAVE - 1) / GM_WAVE;
    const int at = lo + lane * step;
    const bool le = at < hi && col[r0 + at] <= key;
    const int c = __popcll(__ballot(le));  // (ascending: the lanes with col <= key are a prefix)
    if (c == 0) return -1;
    const int nlo = lo + (c - 1) * step;
    hi = min(hi, nlo + step);
    lo = nlo;
  }
  const bool eq = lo + lane < hi && col[r0 + lo + lane] == key;
  const unsigned long long m = __ballot(eq);
  return m ? lo + (int)__builtin_ctzll(m) : -1;
}
// the DAG entry of the edge {a, b}, the whole wave searching
__device__ __forceinline__ int kcl_wave_entry(const int *__restrict__ rp, const int *__restrict__ col, const int a, const int b, const int lane) {
  int r0 = rp[a];
  int pos = kcl_wave_find(col, r0, rp[a + 1] - r0, b, lane);
  if (pos >= 0) return r0 + pos;
  r0 = rp[b];
  pos = kcl_wave_find(col, r0, rp[b + 1] - r0, a, lane);
  return pos >= 0 ? r0 + pos : -1;
}

// the value of the pair (i, l) by a whole WAVE, M >= 2: every lane holds the pair's set, the members j are dealt to the lanes 64 at a time
// and every lane descends below its own -- C_{M-1}(S & Msym_j & {positions above j}) -- at the same time as the others.  The wave's sum.
template <int M, int KW>
__device__ __forceinline__ unsigned long long kcl_pair_wave(const unsigned *__restrict__ msym, const int i, const int l, const int stride, const int lane) {
  unsigned S[KW], R[KW];
#pragma unroll
  for (int w2 = 0; w2 < KW; ++w2) R[w2] = S[w2] = (w2 < stride) ? (msym[i * stride + w2] & msym[l * stride + w2]) : 0u;
  unsigned long long c = 0;
  int rank = 0, mine = -1;
  for (;;) {  // wave-uniform: every lane walks the same members
    int w = -1;
    unsigned x = 0;
#pragma unroll
    for (int ww = KW - 1; ww >= 0; --ww)
      if (R[ww]) { w = ww; x = R[ww]; }
    if (w >= 0) {
#pragma unroll
      for (int w2 = 0; w2 < KW; ++w2)
        if (w2 == w) R[w2] = x & (x - 1u);
      if ((rank & (GM_WAVE - 1)) == lane) mine = w * 32 + (__ffs((int)x) - 1);
      ++rank;
    }
    if (w < 0 || (rank & (GM_WAVE - 1)) == 0) {  // the deal is complete
      if (mine >= 0) {
        const int wj = mine >> 5;
        const unsigned *Mj = msym + mine * stride;
        unsigned T[KW];
#pragma unroll
        for (int w2 = 0; w2 < KW; ++w2) {
          unsigned t = (w2 >= wj && w2 < stride) ? (S[w2] & Mj[w2]) : 0u;
          if (w2 == wj) t &= 0xFFFFFFFEu << (mine & 31);
          T[w2] = t;
        }
        c += KclSmall<M - 1, KW>::run(T, msym, stride);
        mine = -1;
      }
      if (w < 0) break;
    }
  }
  return wave_sum_u64(c);
}
// the value of the pair (i, l): C_M(Msym_i & Msym_l), the set in KW registers
template <int M, int KW>
__device__ __forceinline__ unsigned long long kcl_pair_small(const unsigned *__restrict__ msym, const int i, const int l, const int stride) {
  unsigned T[KW];
#pragma unroll
  for (int w2 = 0; w2 < KW; ++w2) T[w2] = (w2 < stride) ? (msym[i * stride + w2] & msym[l * stride + w2]) : 0u;
  return KclSmall<M, KW>::run(T, msym, stride);
}

// One root, or one of `nparts` shares of it (the grains idx = part (mod nparts) of its matrix; every share builds the matrix for itself).
// WAVE = false: the lanes take grains of the upper triangle from a counter in LDS and ONE pair per trip: every lane of a wave is in a
// descent at the same time, whatever the words hold.  WAVE = true (k >= 5, the split roots): the waves take the grains and a whole wave
// one pair -- the pairs of a long row differ by orders of magnitude in what lies below them.
template <int K, bool WAVE>
__device__ __forceinline__ void kcl_root_lds(const KclLocalParams &p, const int u, const int part, const int nparts, unsigned *__restrict__ msym,
                                             unsigned long long *__restrict__ acc, int *__restrict__ Ls, int *__restrict__ next_word) {
  static_assert(!WAVE || K >= 5, "a wave per pair deals the first level of the descent");
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
  kcl_build_msym_lds(p.rp, p.col, Ls, d, stride, msym, wave, lane);  // (gm_kcl.h)
  __syncthreads();
  // a grain: a word of the matrix, or (k >= 5, where a pair is a long descent) 4 bits of one
  constexpr int kSlices = K >= 5 ? 8 : 1;
  const int ngrains = d * stride * kSlices;
  unsigned x = 0u;  // the pairs of the lane's (WAVE: the wave's) grain, of row i and word w, not taken yet
  int i = 0, w = 0;
  for (;;) {
    while (x == 0u) {
      int t = 0;
      if (!WAVE || lane == 0) t = atomicAdd(next_word, 1);
      if (WAVE) t = readfirst(t);
      const int idx = part + t * nparts;
      if (idx >= ngrains) break;
      const int word = idx / kSlices;
      i = word / stride;
      w = word - i * stride;
      if (w < (i >> 5)) continue;  // (below the diagonal)
      x = msym[word];
      if (w == (i >> 5)) x &= 0xFFFFFFFEu << (i & 31);
      if constexpr (kSlices > 1) x &= ((1u << (32 / kSlices)) - 1u) << ((idx % kSlices) * (32 / kSlices));
    }
    if (x == 0u) break;  // (no grain is left)
    const int l = w * 32 + (__ffs((int)x) - 1);
    x &= x - 1u;
    // (workgroup-uniform: the registers a set takes follow the row's length -- kKclLocalRegs2Row, kKclLocalRegs8Row, kKclLocalRegs12Row)
    if constexpr (WAVE) {
      const unsigned long long val = stride <= kKclLocalRegs8Row / 32    ? kcl_pair_wave<K - 3, kKclLocalRegs8Row / 32>(msym, i, l, stride, lane)
                                     : stride <= kKclLocalRegs12Row / 32 ? kcl_pair_wave<K - 3, kKclLocalRegs12Row / 32>(msym, i, l, stride, lane)
                                                                         : kcl_pair_wave<K - 3, kKclWords>(msym, i, l, stride, lane);
      if (val == 0ull) continue;
      const int e = kcl_wave_entry(p.rp, p.col, Ls[i], Ls[l], lane);
      if (lane == 0) {
        if (e >= 0) atomicAdd(&p.cnt[e], val);
        else atomicAdd(p.err, 1ull);
        atomicAdd(&acc[i], val);
        atomicAdd(&acc[l], val);
      }
    } else {
      const unsigned long long val = stride <= kKclLocalRegs2Row / 32    ? kcl_pair_small<K - 3, kKclLocalRegs2Row / 32>(msym, i, l, stride)
                                     : stride <= kKclLocalRegs8Row / 32  ? kcl_pair_small<K - 3, kKclLocalRegs8Row / 32>(msym, i, l, stride)
                                     : stride <= kKclLocalRegs12Row / 32 ? kcl_pair_small<K - 3, kKclLocalRegs12Row / 32>(msym, i, l, stride)
                                                                         : kcl_pair_small<K - 3, kKclWords>(msym, i, l, stride);
      if (val == 0ull) continue;
      const int e = kcl_entry(p.rp, p.col, Ls[i], Ls[l]);
      if (e >= 0) atomicAdd(&p.cnt[e], val);
      else atomicAdd(p.err, 1ull);
      atomicAdd(&acc[i], val);
      atomicAdd(&acc[l], val);
    }
  }
  __syncthreads();
  for (int j = tid; j < d; j += 256)
    if (acc[j]) atomicAdd(&p.spk[ru + j], acc[j]);  // (undivided: the shares of a root add up first -- kcl_local_fold_kernel)
  __syncthreads();  // (the next root rewrites the LDS)
}

// SPLIT = false: the roots as they are numbered, kKclGrab per dequeue -- those of up to kKclLocalLdsRow entries are counted (k >= 5: up
// to kKclLocalSplitRow; the longer ones go to the list of the split roots), those beyond go to the list of the wide kernel.
// SPLIT = true: the split roots, kKclParts workgroups each.
template <int K, bool SPLIT>
__global__ __launch_bounds__(256) void kcl_local_kernel(const KclLocalParams p) {
  __shared__ unsigned msym[kKclLocalLdsRow * kKclWords];
  __shared__ unsigned long long acc[kKclLocalLdsRow];  // per position: the sum of the inner values of its pairs
  __shared__ int Ls[kKclLocalLdsRow];
  __shared__ unsigned slot;
  __shared__ int next_word;
  const int tid = threadIdx.x;
  const unsigned count = SPLIT ? min(*p.n_mid, p.mid_cap) * (unsigned)kKclParts : (unsigned)p.nv;  // (SPLIT: the list is complete)
  for (;;) {
    if (tid == 0) slot = atomicAdd(SPLIT ? p.queue_mid : p.queue, SPLIT ? 1u : (unsigned)kKclGrab);
    __syncthreads();
    const unsigned q = slot;
    __syncthreads();  // (a dequeue whose roots are all skipped has no other barrier before the next one)
    if (q >= count) break;
    if constexpr (SPLIT) {
      kcl_root_lds<K, (K >= 5)>(p, p.mid[q / kKclParts], (int)(q % kKclParts), kKclParts, msym, acc, Ls, &next_word);
    } else {
      const int qe = (int)min(q + (unsigned)kKclGrab, count);
      for (int u = (int)q; u < qe; ++u) {
        const int d = p.rp[u + 1] - p.rp[u];
        if (d < K - 1) continue;  // (workgroup-uniform: a k-clique rooted here needs k - 1 out-neighbours)
        const bool wide = d > kKclLocalLdsRow, split = !wide && K >= 5 && d > kKclLocalSplitRow;
        if (wide || split) {
          if (tid == 0) {
            const unsigned at = atomicAdd(wide ? p.n_heavy : p.n_mid, 1u);
            if (at < (wide ? p.heavy_cap : p.mid_cap)) (wide ? p.heavy : p.mid)[at] = u;
            else atomicAdd(p.err, 1ull);  // (cannot happen: the lists hold every row that can be this long)
          }
          continue;
        }
        kcl_root_lds<K, false>(p, u, 0, 1, msym, acc, Ls, &next_word);
      }
    }
  }
}

// cnt[e] += spk[e] / (k - 2): the spokes, once every share of every root has added its sums
__global__ __launch_bounds__(256) void kcl_local_fold_kernel(const long long ne, const unsigned div, unsigned long long *__restrict__ cnt,
                                                             const unsigned long long *__restrict__ spk) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += stride) {
    const unsigned long long s = spk[e];
    if (s) cnt[e] += s / (unsigned long long)div;
  }
}

// the workgroup's scratch slot: the spoke sums (max_deg uint64), the matrix (max_deg rows), the four waves' set stacks (kKclMaxLevels sets each)
unsigned long long kcl_local_scratch_words(int max_deg) {
  const unsigned long long D = (unsigned long long)std::max(max_deg, 1), S = (D + 31) >> 5;
  return (2ull * D + D * S + 4ull * kKclMaxLevels * S + 1ull) & ~1ull;  // (even: the slots stay 8-byte aligned)
}

template <int K>
__global__ __launch_bounds__(256) void kcl_local_wide_kernel(const KclLocalParams p) {
  static_assert(K - 3 <= kKclMaxLevels, "a set per level of the descent");
  __shared__ unsigned slot;
  __shared__ int next_row;
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = tid >> 6;
  unsigned *base = p.scratch + (size_t)blockIdx.x * p.scratch_words;
  unsigned long long *acc = reinterpret_cast<unsigned long long *>(base);  // (scratch_words is even: 8-byte aligned)
  unsigned *msym = base + 2 * (size_t)p.max_deg;
  const unsigned n_heavy = min(*p.n_heavy, p.heavy_cap);  // (complete: kcl_local_kernel ran before this launch)
  for (;;) {
    if (tid == 0) {
      slot = atomicAdd(p.queue_wide, 1u);
      next_row = 0;
    }
    __syncthreads();
    const unsigned q = slot;
    __syncthreads();
    if (q >= n_heavy) break;
    const int u = p.heavy[q];
    const int ru = p.rp[u], d = p.rp[u + 1] - ru;
    if (d > p.max_deg) {  // (cannot happen: the slot is sized by the handle's longest row)
      if (tid == 0) atomicAdd(p.err, 1ull);
      __syncthreads();
      continue;
    }
    const int stride = (d + 31) >> 5;
    const int *L = p.col + ru;
    unsigned *stk = msym + (size_t)d * stride + (size_t)wave * kKclMaxLevels * stride;
    for (size_t i = tid; i < (size_t)d * stride; i += 256) msym[i] = 0u;
    for (int i = tid; i < d; i += 256) acc[i] = 0ull;
    __threadfence();
    __syncthreads();
    kcl_build_msym_wide(p.rp, p.col, L, d, stride, msym, wave, lane);  // (gm_kcl.h)
    __threadfence();
    __syncthreads();
    for (;;) {  // a wave per row i, taken dynamically: the first rows hold the most pairs
      int i = 0;
      if (lane == 0) i = atomicAdd(&next_row, 1);
      i = readfirst(i);
      if (i >= d) break;
      const unsigned *Mi = msym + (size_t)i * stride;
      unsigned long long row_sum = 0;
      for (int w = i >> 5; w < stride; ++w) {
        unsigned x = (unsigned)readfirst((int)Mi[w]);  // (every lane reads the same word)
        if (w == (i >> 5)) x &= 0xFFFFFFFEu << (i & 31);
        while (x) {
          const int l = w * 32 + (__ffs((int)x) - 1);
          x &= x - 1u;
          const unsigned *Ml = msym + (size_t)l * stride;
          unsigned long long part = 0;
          if constexpr (K == 4) {  // (the pair's own set is all there is: counted as it is formed)
            for (int w2 = lane; w2 < stride; w2 += GM_WAVE) part += (unsigned)__popc(Mi[w2] & Ml[w2]);
          } else {
            for (int w2 = lane; w2 < stride; w2 += GM_WAVE) stk[w2] = Mi[w2] & Ml[w2];
            part = KclAny<K - 3>::run(stk, stk + stride, msym, stride, lane);
          }
          const unsigned long long val = wave_sum_u64(part);
          if (val == 0ull) continue;
          row_sum += val;
          const int e = kcl_wave_entry(p.rp, p.col, readfirst(L[i]), readfirst(L[l]), lane);
          if (lane == 0) {
            if (e >= 0) atomicAdd(&p.cnt[e], val);
            else atomicAdd(p.err, 1ull);
            atomicAdd(&acc[l], val);
          }
        }
      }
      if (lane == 0 && row_sum) atomicAdd(&acc[i], row_sum);
    }
    __threadfence();
    __syncthreads();
    for (int i = tid; i < d; i += 256) {
      const unsigned long long s = __hip_atomic_load(&acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (s) atomicAdd(&p.spk[ru + i], s);  // (undivided, as kcl_root_lds leaves them)
    }
    __syncthreads();  // (the next root rewrites the slot)
  }
}

template <int K>
static hipError_t launch_kcl_k(const KclLocalParams &p, int stage, int grid, hipStream_t stream) {
  if (stage == KCL_STAGE_ROOTS) hipLaunchKernelGGL((kcl_local_kernel<K, false>), dim3(grid), dim3(256), 0, stream, p);
  else if (stage == KCL_STAGE_SPLIT) hipLaunchKernelGGL((kcl_local_kernel<K, true>), dim3(grid), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(kcl_local_wide_kernel<K>, dim3(grid), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_kcl_local(const KclLocalParams &p, int stage, int grid, hipStream_t stream) {
  if (p.nv <= 0 || p.ne <= 0 || grid < 1) return hipSuccess;
  if (!p.cnt || !p.spk || !p.queue || !p.queue_wide || !p.queue_mid || !p.heavy || !p.n_heavy || !p.mid || !p.n_mid || !p.err ||
      (stage == KCL_STAGE_WIDE && (!p.scratch || (p.scratch_words & 1ull))))
    return hipErrorInvalidValue;
  if (stage == KCL_STAGE_FOLD) {
    hipLaunchKernelGGL(kcl_local_fold_kernel, dim3(grid), dim3(256), 0, stream, p.ne, (unsigned)(p.k - 2), p.cnt, p.spk);
    return hipGetLastError();
  }
  switch (p.k) {
    case 3: return launch_kcl_k<3>(p, stage, grid, stream);
    case 4: return launch_kcl_k<4>(p, stage, grid, stream);
    case 5: return launch_kcl_k<5>(p, stage, grid, stream);
    case 6: return launch_kcl_k<6>(p, stage, grid, stream);
    case 7: return launch_kcl_k<7>(p, stage, grid, stream);
    case 8: return launch_kcl_k<8>(p, stage, grid, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_kcl_local_kernel() {}
void gm_touch_kcl_local() { hipLaunchKernelGGL(gm_touch_kcl_local_kernel, dim3(1), dim3(1), 0, 0); }
