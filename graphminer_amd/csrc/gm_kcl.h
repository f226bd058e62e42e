// gm_kcl.h -- what the k-clique kernels over a root's out-list share (gm_kcl_local.hip: the local counts, gm_clique_list.hip: the listing):
// the symmetric adjacency bit-matrix Msym of an out-list L = N+(u) (row i = the positions of L adjacent to L[i]) and the descents over it,
//   C_0 = 1,  C_1(S) = |S|,  C_m(S) = sum_{j in S} C_{m-1}(S & Msym_j & {positions above j}).
// Device code only; included by those two units.
#pragma once
#include "gm_setops.h"
#include "gm_mine.h"

namespace gm {

constexpr int kKclWords = kKclLocalLdsRow / 32;  // words of a row of the LDS matrix
constexpr int kKclMaxLevels = 5;                 // k <= 8: the pair's own set and the sets of C_4 .. C_2

// Msym of a row held in LDS (Ls, d entries, zeroed matrix of `stride` words per row): a wave per position i -- N+(L[i]) is streamed against
// L in LDS, or, when it is much the longer list, L against it.  The caller puts a barrier behind it.
__device__ __forceinline__ void kcl_build_msym_lds(const int *rp, const int *col, const int *__restrict__ Ls, const int d,
                                                   const int stride, unsigned *__restrict__ msym, const int wave, const int lane) {
  for (int i = wave; i < d; i += 4) {
    const int v = Ls[i], rv = rp[v], b = rp[v + 1] - rv;
    const bool stream_row = b <= 4 * d;
    const int n = stream_row ? b : d;
    for (int t = lane; t < n; t += GM_WAVE) {
      int pos = 0;
      bool hit;
      if (stream_row) {
        hit = contains(Ls, d, col[rv + t], &pos);
      } else {
        int at = 0;
        hit = contains(col + rv, b, Ls[t], &at);
        pos = t;
      }
      if (hit) {
        atomicOr(&msym[i * stride + (pos >> 5)], 1u << (pos & 31));
        atomicOr(&msym[pos * stride + (i >> 5)], 1u << (i & 31));
      }
    }
  }
}
// ... of a row of any length, the matrix in global memory (zeroed; L: the row in the CSR).  The caller fences and puts a barrier behind it.
__device__ __forceinline__ void kcl_build_msym_wide(const int *rp, const int *col, const int *L, const int d,
                                                    const int stride, unsigned *msym, const int wave, const int lane) {
  for (int i = wave; i < d; i += 4) {
    const int v = L[i], rv = rp[v], b = rp[v + 1] - rv;
    for (int t = lane; t < b; t += GM_WAVE) {
      int pos = 0;
      if (contains(L, d, col[rv + t], &pos)) {
        atomicOr(&msym[(size_t)i * stride + (pos >> 5)], 1u << (pos & 31));
        atomicOr(&msym[(size_t)pos * stride + (i >> 5)], 1u << (i & 31));
      }
    }
  }
}

// C_M of a set of up to 32 KW positions held in KW registers.  The next member is found with compile-time indices only (the set stays in
// registers) and every level has ONE call site of the level below it: the code grows linearly in M.
template <int M, int KW>
struct KclSmall {
  static __device__ __forceinline__ unsigned long long run(const unsigned (&S)[KW], const unsigned *__restrict__ msym, const int stride) {
    unsigned R[KW];  // the members not visited yet
#pragma unroll
    for (int w = 0; w < KW; ++w) R[w] = S[w];
    unsigned long long c = 0;
    for (;;) {
      int w = -1;
      unsigned x = 0;
#pragma unroll
      for (int ww = KW - 1; ww >= 0; --ww)
        if (R[ww]) { w = ww; x = R[ww]; }
      if (w < 0) break;
      const int bit = __ffs((int)x) - 1;
      const unsigned *Mj = msym + (w * 32 + bit) * stride;
      unsigned T[KW];
#pragma unroll
      for (int w2 = 0; w2 < KW; ++w2) {
        if (w2 == w) R[w2] = x & (x - 1u);
        unsigned t = (w2 >= w && w2 < stride) ? (S[w2] & Mj[w2]) : 0u;
        if (w2 == w) t &= 0xFFFFFFFEu << bit;  // the positions above j
        T[w2] = t;
      }
      c += KclSmall<M - 1, KW>::run(T, msym, stride);
    }
    return c;
  }
};
template <int KW>
struct KclSmall<1, KW> {
  static __device__ __forceinline__ unsigned long long run(const unsigned (&S)[KW], const unsigned *, int) {
    unsigned c = 0;
#pragma unroll
    for (int w = 0; w < KW; ++w) c += (unsigned)__popc(S[w]);
    return c;
  }
};
template <int KW>
struct KclSmall<0, KW> {
  static __device__ __forceinline__ unsigned long long run(const unsigned (&)[KW], const unsigned *, int) { return 1ull; }
};

// C_M of a set of `stride` words in memory, one wave: lane t owns the words t, t + 64, ... of every set (it alone writes and reads them);
// the members are walked wave-uniformly through readlane.  `stk`: the sets of the levels below, `stride` words each.  Per-lane partial.
template <int M>
struct KclAny {
  static __device__ __forceinline__ unsigned long long run(const unsigned *S, unsigned *stk, const unsigned *msym, const int stride, const int lane) {
    unsigned long long c = 0;
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
          const unsigned *Mj = msym + (size_t)(w * 32 + bit) * stride;
          for (int w2 = lane; w2 < stride; w2 += GM_WAVE) {
            unsigned t = (w2 >= w) ? (S[w2] & Mj[w2]) : 0u;
            if (w2 == w) t &= 0xFFFFFFFEu << bit;
            stk[w2] = t;
          }
          c += KclAny<M - 1>::run(stk, stk + stride, msym, stride, lane);
        }
      }
    }
    return c;
  }
};
template <>
struct KclAny<1> {
  static __device__ __forceinline__ unsigned long long run(const unsigned *S, unsigned *, const unsigned *, const int stride, const int lane) {
    unsigned c = 0;
    for (int w = lane; w < stride; w += GM_WAVE) c += (unsigned)__popc(S[w]);
    return c;
  }
};
template <>
struct KclAny<0> {
  static __device__ __forceinline__ unsigned long long run(const unsigned *, unsigned *, const unsigned *, int, const int lane) { return lane == 0 ? 1ull : 0ull; }
};

}  // namespace gm
