// gm_ctc.hip -- triangle count, the triangles of the HUB CORE on the matrix cores.
//
// On a DAG numbered by degree the hubs are the LAST ids, and every out-neighbour of a hub is a hub: the out-edges of the last H vertices
// lie inside the H x H corner of the adjacency matrix.  They are a few per cent of the edges and 30 - 65 % of the keys the streamed
// triangle kernel (gm_tch.hip) moves -- a task costs min(d+(v), tail_u(v)) keys, and those are the longest lists of the graph
// (R-MAT-22: H = 8 K / 16 K / 32 K vertices = 3.7 / 6.0 / 10.8 M of 40.6 M edges = 29 / 42 / 66 % of the 2.98 G streamed keys).
// With M = the corner as a bit matrix (strictly upper triangular under the topological numbering; the 4-clique's core bitmap, gm_host.h
// HubCore) the triangles whose smallest member is a core vertex are
//     sum_{i<j, M_ij} popc(M_i & M_j)  =  sum_{i,j} M_ij (M M^T)_ij                                   (omp_base.cc:15-21 on bit rows)
// -- the masked binary matrix product of the 4-clique's second level (gm_cmma.hip), once, on one H x H matrix: FP4 MFMA with a set bit
// as the E2M1 value 1.0, f32 accumulators (exact: a sum is at most H <= 2^15), a wave per 64 x 64 block of (i, j) with I <= J over the
// column steps K >= J (1/6 of the cube: H = 16 K is 1.1 * 10^7 v_mfma_scale_f32_32x32x64_f8f6f4, ~0.2 ms of the chip), a block whose mask
// is empty skipped.  The key stream and the task lists of the triangle count leave the rows >= nv - H out (TaskWalk::skip_from).
//   * core_tc_block_kernel (corners of a multiple of 512 vertices, 16-byte aligned rows: every real graph): a workgroup of eight waves takes a
//     256 x 256 block of (i, j), wave (wi, wj) its 64 x 128 part (2 x 4 accumulator tiles: six operand words expanded per eight MFMAs, 34 vector instructions), over
//     column chunks of 512: the chunk of the 256 I rows and the 256 J rows (32 KB, 64 contiguous bytes per row) goes global -> registers
//     -> LDS (two stages: one workgroup barrier per chunk), the next chunk's loads in flight while this one is multiplied; LDS rows of 20 words (the sixteen lanes of a quarter of a
//     ds_read_b128 hit sixteen different bank groups).  The order of the columns inside an operand fragment does not matter and neither
//     does the assignment of column words to MFMA steps -- both operands are rows of the same matrix, expanded the same way -- so lane
//     (row l & 31, half h = l >> 5) reads the four words 4 (2 q + h) .. + 3 of its row with one 16-byte read and feeds word w to step
//     4 q + w.  A first version with the operands straight from global memory (a wave per 64 x 64 block, 16-byte loads) moved every line
//     four times through L1: 0.75 ms for H = 16 K where the MFMAs need 0.15.  Long column ranges are cut into PIECES of 16 chunks (the
//     masked sum is linear in the column range), so that a task is ~10 us;
//   * core_tc_kernel<GUARD> (any other corner: small graphs, tests): a wave per 64 x 64 block, one word per load and step, rows and words
//     beyond the corner read as zero.
#include <algorithm>
#include "gm_flat.h"

namespace gm {

typedef int ctc_v8i __attribute__((ext_vector_type(8)));
typedef float ctc_v16f __attribute__((ext_vector_type(16)));

// 32 bits -> 32 FP4 (E2M1) nibbles, bit 4 p + r of the word in nibble p of register r.  The two operands of a product encode a set bit
// DIFFERENTLY so that most registers need no shift: bit class r = 0 / 1 / 2 / 3 is 0.5 / 1 / 2 / 2 in the A operand (nibble 0001 / 0010 /
// 0100 / 0100) and 2 / 1 / 0.5 / 0.5 in the B operand -- every product of two set bits is exactly 1.  Five and seven vector instructions
// (both operands as 1.0 -- x << 1, x, x >> 1, x >> 2, each & 0x22222222 -- cost seven each).
__device__ __forceinline__ ctc_v8i ctc_expand_a(const unsigned x) {
  ctc_v8i r = {(int)(x & 0x11111111u), (int)(x & 0x22222222u), (int)(x & 0x44444444u), (int)((x >> 1) & 0x44444444u), 0, 0, 0, 0};
  return r;
}
__device__ __forceinline__ ctc_v8i ctc_expand_b(const unsigned x) {
  ctc_v8i r = {(int)((x << 2) & 0x44444444u), (int)(x & 0x22222222u), (int)((x >> 2) & 0x11111111u), (int)((x >> 3) & 0x11111111u), 0, 0, 0, 0};
  return r;
}
// sum of the accumulators whose mask bit is set: register r of this lane is bit (r & 3) + 8 (r >> 2) of w (already shifted by 4 (l >> 5))
__device__ __forceinline__ float ctc_masked_sum(const ctc_v16f &acc, const unsigned w) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned mb = (w >> q) & 0x01010101u;
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) s = fmaf(acc[q + 4 * pp], (float)((mb >> (8 * pp)) & 0xffu), s);
  }
  return s;
}
#define CTC_MFMA(a, b, c) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f)  // FP4 x FP4, unit scales

// ---- any corner: a wave per 64 x 64 block, operands word by word from global memory (small graphs, sizes that are no multiple of 512) ----
__global__ __launch_bounds__(kCtcWaves *GM_WAVE) void core_tc_kernel(const CoreTcParams p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const int l31 = lane & 31, h = lane >> 5;
  const int H = p.h, rw = p.row_words;
  const int wtc = (H + 31) >> 5;  // words of a corner row
  const unsigned *__restrict__ M = p.core + (size_t)p.row0 * (size_t)rw + (size_t)p.word0;
  unsigned long long tot = 0;
  unsigned c = 0;
  for (;;) {
    unsigned q = 0;
    if (lane == 0) q = atomicAdd(p.queue, 1u);
    q = (unsigned)readfirst((int)q);
    const long long t64 = (long long)p.first + (long long)q * p.step;
    if (t64 >= (long long)p.ntasks) break;
    const int t = (int)t64;
    // t = JB (JB + 1) / 2 + IB, IB <= JB
    int JB = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while ((JB + 1) * (JB + 2) / 2 <= t) ++JB;
    while (JB * (JB + 1) / 2 > t) --JB;
    const int IB = t - JB * (JB + 1) / 2;
    // this lane's rows of the I and the J block (two 32-row tiles each); rows beyond the corner read row 0 and count as zero
    const int ri = IB * 64 + l31, rj = JB * 64 + l31;
    const bool vi0 = ri < H, vi1 = ri + 32 < H, vj0 = rj < H, vj1 = rj + 32 < H;
    const unsigned *pi0 = M + (size_t)(vi0 ? ri : 0) * rw, *pi1 = M + (size_t)(vi1 ? ri + 32 : 0) * rw;
    const unsigned *pj0 = M + (size_t)(vj0 ? rj : 0) * rw, *pj1 = M + (size_t)(vj1 ? rj + 32 : 0) * rw;
    // the mask of the block: word (32-column J tile) of the lane's rows of the I tiles
    unsigned mw[2][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int wc = JB * 2 + jj;
      const bool in = wc < wtc;
      const unsigned a = pi0[in ? wc : 0], b = pi1[in ? wc : 0];
      mw[jj][0] = (in && vi0) ? a : 0u;
      mw[jj][1] = (in && vi1) ? b : 0u;
    }
    if (__ballot((mw[0][0] | mw[0][1] | mw[1][0] | mw[1][1]) != 0u) == 0ull) continue;  // no edge (i, j) in this block
    ctc_v16f acc[2][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jj][ii][r] = 0.f;
    const int k1 = (wtc + 1) >> 1;  // column steps of 64 = 2 words: lane half h takes word 2 k + h; steps below the J block hold no bit of its rows
    for (int ks = JB; ks < k1; ++ks) {
      const int wc = 2 * ks + h;
      const bool in = wc < wtc;
      const int wx = in ? wc : 0;
      const unsigned a0 = pi0[wx], a1 = pi1[wx], b0 = pj0[wx], b1 = pj1[wx];
      const ctc_v8i fi0 = ctc_expand_b((in && vi0) ? a0 : 0u), fi1 = ctc_expand_b((in && vi1) ? a1 : 0u);
      const ctc_v8i fj0 = ctc_expand_a((in && vj0) ? b0 : 0u), fj1 = ctc_expand_a((in && vj1) ? b1 : 0u);
      acc[0][0] = CTC_MFMA(fj0, fi0, acc[0][0]);
      acc[0][1] = CTC_MFMA(fj0, fi1, acc[0][1]);
      acc[1][0] = CTC_MFMA(fj1, fi0, acc[1][0]);
      acc[1][1] = CTC_MFMA(fj1, fi1, acc[1][1]);
    }
    float s = 0.f;  // <= 4 tiles x 16 registers x H: exact in f32 (H <= 2^15)
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) s += ctc_masked_sum(acc[jj][ii], mw[jj][ii] >> (4 * h));
    c += (unsigned)s;
    if (c > 0x7fffffffu) {
      tot += (unsigned long long)c;
      c = 0;
    }
  }
  tot += (unsigned long long)c;
  const unsigned long long s0 = wave_sum_u64(tot);
  if (lane == 0 && s0) atomicAdd(&p.counters[0], s0);
}

// ---- corners of a multiple of 512 vertices: 256 x 256 blocks through LDS ------------------------------------------------------------
constexpr int kCtcBWaves = 8;        // wave (wi = w & 3, wj = w >> 2): I rows 64 wi .. + 63, J rows 128 wj .. + 127 of the block
// (a column chunk: 512 columns = 16 words = 64 bytes of a row)
constexpr int kCtcBStride = 20;      // LDS words per row (16 + 4: see the header)
// (kCtcBPiece, gm_mine.h: chunks per task of the triangle count)
constexpr int kCtcBPieceSup = 32;    // ... of the edge supports' product: every piece ends with an epilogue of atomics per edge
constexpr int kCtcBStages = 2;  // two LDS stages (80 KB): ONE workgroup barrier per chunk (one stage, two barriers: 5 - 6 % slower, profiles/r05/ab_tc_core.txt)
constexpr int kCtcBPanWords = 512 * kCtcBStride;
struct alignas(16) CtcBlockLds {
  unsigned pan[kCtcBStages * kCtcBPanWords];  // per stage -- rows 0 .. 255: the I rows' chunk, 256 .. 511: the J rows'
  unsigned queue_pos;
  int pad_[3];
};
__host__ __device__ inline int ctc_block_tasks(int h) {  // (pair of 256-row blocks IB <= JB) x (piece of the column range)
  const int nb = h >> 8, nc = h >> 9;
  return nb * (nb + 1) / 2 * ((nc + kCtcBPiece - 1) / kCtcBPiece);
}

// SUP (edge supports, gm_sup.hip): `core` is the SYMMETRIC corner A = M + M^T, the column range is whole (a triangle's third vertex lies
// before, between or behind i and j: t(i, j) = (A A)_ij), and the epilogue adds every masked accumulator to the support of its edge --
// DAG entry rp[base + i] + first[i][word of j] + the set bits of the word below j -- instead of summing them
template <bool SUP>
__global__ __launch_bounds__(kCtcBWaves *GM_WAVE) void core_tc_block_kernel(const CoreTcParams p) {
  __shared__ CtcBlockLds S;
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wave = readfirst(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int wi = wave & 3, wj = wave >> 2;
  const int H = p.h, rw = p.row_words;
  constexpr int kPiece = SUP ? kCtcBPieceSup : kCtcBPiece;
  const int nc = H >> 9, maxp = (nc + kPiece - 1) / kPiece;
  const unsigned *__restrict__ M = p.core + (size_t)p.row0 * (size_t)rw + (size_t)p.word0;
  // this thread's four 16-byte pieces of a chunk: piece x = tid + 512 k -> row x >> 2 of the 512 staged rows, segment x & 3 of its 64 bytes
  const int seg = tid & 3, srow = tid >> 2;  // rows srow, srow + 128 (I), srow + 256, srow + 384 (J)
  // the LDS rows this lane reads its operand words from
  const uint4 *li[2], *lj[4];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) li[ii] = reinterpret_cast<const uint4 *>(&S.pan[(64 * wi + 32 * ii + l31) * kCtcBStride + 4 * h]);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) lj[jj] = reinterpret_cast<const uint4 *>(&S.pan[(256 + 128 * wj + 32 * jj + l31) * kCtcBStride + 4 * h]);
  unsigned long long tot = 0;
  unsigned c = 0;
  for (;;) {
    if (tid == 0) S.queue_pos = atomicAdd(p.queue, 1u);
    __syncthreads();
    const unsigned q = S.queue_pos;
    __syncthreads();
    const long long t64 = (long long)p.first + (long long)q * p.step;
    if (t64 >= (long long)p.ntasks) break;
    int IB, JB, piece;
    if (!SUP && p.tasks != nullptr) {  // the chosen pairs' pieces, longest first (gm_tasks.hip tc_pairs_setup)
      const unsigned t = p.tasks[t64];
      IB = (int)(t & 255u);
      JB = (int)((t >> 8) & 255u);
      piece = (int)(t >> 16);
    } else {
      const int pair = (int)(t64 / maxp);
      piece = (int)(t64 - (long long)pair * maxp);
      JB = (int)((sqrtf(8.f * (float)pair + 1.f) - 1.f) * 0.5f);
      while ((JB + 1) * (JB + 2) / 2 <= pair) ++JB;
      while (JB * (JB + 1) / 2 > pair) --JB;
      IB = pair - JB * (JB + 1) / 2;
    }
    // chunks below the J block hold no bit of its rows (strictly upper triangular); the chunk with the diagonal is taken whole
    const int cb = (SUP ? 0 : (JB >> 1)) + piece * kPiece, ce = min(cb + kPiece, nc);
    if (cb >= nc) continue;  // (workgroup-uniform: this pair has fewer pieces)
    // (the first chunk is requested before the mask words: one round trip for both)
    const uint4 *g0 = reinterpret_cast<const uint4 *>(M + (size_t)(256 * IB + srow) * rw) + seg;
    const uint4 *g1 = reinterpret_cast<const uint4 *>(M + (size_t)(256 * IB + srow + 128) * rw) + seg;
    const uint4 *g2 = reinterpret_cast<const uint4 *>(M + (size_t)(256 * JB + srow) * rw) + seg;
    const uint4 *g3 = reinterpret_cast<const uint4 *>(M + (size_t)(256 * JB + srow + 128) * rw) + seg;
    uint4 r0 = g0[4 * cb], r1 = g1[4 * cb], r2 = g2[4 * cb], r3 = g3[4 * cb];
    // the mask of this wave's part: word (32-column J tile) of the lane's rows of its I tiles
    unsigned mw[4][2];
    unsigned any_bits = 0u;
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const unsigned *row = M + (size_t)(256 * IB + 64 * wi + 32 * ii + l31) * rw + 8 * JB + 4 * wj;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        unsigned w = row[jj];
        if (SUP && IB == JB) {  // the symmetric matrix: only the edges i < j of a diagonal block
          const int below = 64 * wi + 32 * ii + l31 - (128 * wj + 32 * jj);  // columns 0 .. below of this word are <= i
          w = below >= 31 ? 0u : (below >= 0 ? w & ~((2u << below) - 1u) : w);
        }
        mw[jj][ii] = w;
        any_bits |= w;
      }
    }
    const bool any = __ballot(any_bits != 0u) != 0ull;  // (wave-uniform) no edge (i, j) in this part: the wave only helps staging
    ctc_v16f acc[4][2];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jj][ii][r] = 0.f;
    auto stage_store = [&](const int st) {
      unsigned *pan = S.pan + st * kCtcBPanWords;
      *reinterpret_cast<uint4 *>(&pan[(srow) * kCtcBStride + 4 * seg]) = r0;
      *reinterpret_cast<uint4 *>(&pan[(srow + 128) * kCtcBStride + 4 * seg]) = r1;
      *reinterpret_cast<uint4 *>(&pan[(srow + 256) * kCtcBStride + 4 * seg]) = r2;
      *reinterpret_cast<uint4 *>(&pan[(srow + 384) * kCtcBStride + 4 * seg]) = r3;
    };
    // chunk cb into stage 0, chunk cb + 1 requested (the stages of the previous task were last read before its final barrier)
    stage_store(0);
    __syncthreads();
    if (cb + 1 < ce) { r0 = g0[4 * cb + 4]; r1 = g1[4 * cb + 4]; r2 = g2[4 * cb + 4]; r3 = g3[4 * cb + 4]; }
    for (int ch = cb; ch < ce; ++ch) {
      const int st = (ch - cb) & 1;
      const int so = st * (kCtcBPanWords / 4);  // (uint4 units)
      if (any) {
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {  // words 4 (2 qq + h) .. + 3 of the chunk: word w feeds step 4 qq + w
          const uint4 xi0 = li[0][so + 2 * qq], xi1 = li[1][so + 2 * qq];
          const uint4 xj0 = lj[0][so + 2 * qq], xj1 = lj[1][so + 2 * qq], xj2 = lj[2][so + 2 * qq], xj3 = lj[3][so + 2 * qq];
          const unsigned wi0[4] = {xi0.x, xi0.y, xi0.z, xi0.w}, wi1[4] = {xi1.x, xi1.y, xi1.z, xi1.w};
          const unsigned wj0[4] = {xj0.x, xj0.y, xj0.z, xj0.w}, wj1[4] = {xj1.x, xj1.y, xj1.z, xj1.w};
          const unsigned wj2[4] = {xj2.x, xj2.y, xj2.z, xj2.w}, wj3[4] = {xj3.x, xj3.y, xj3.z, xj3.w};
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const ctc_v8i fi0 = ctc_expand_b(wi0[s]), fi1 = ctc_expand_b(wi1[s]);  // (the four J words take the cheaper encoding)
            const ctc_v8i fj0 = ctc_expand_a(wj0[s]), fj1 = ctc_expand_a(wj1[s]), fj2 = ctc_expand_a(wj2[s]), fj3 = ctc_expand_a(wj3[s]);
            acc[0][0] = CTC_MFMA(fj0, fi0, acc[0][0]);
            acc[0][1] = CTC_MFMA(fj0, fi1, acc[0][1]);
            acc[1][0] = CTC_MFMA(fj1, fi0, acc[1][0]);
            acc[1][1] = CTC_MFMA(fj1, fi1, acc[1][1]);
            acc[2][0] = CTC_MFMA(fj2, fi0, acc[2][0]);
            acc[2][1] = CTC_MFMA(fj2, fi1, acc[2][1]);
            acc[3][0] = CTC_MFMA(fj3, fi0, acc[3][0]);
            acc[3][1] = CTC_MFMA(fj3, fi1, acc[3][1]);
          }
        }
      }
      // chunk ch + 1 into the other stage (its loads had this chunk's products to land), chunk ch + 2 requested
      if (ch + 1 < ce) stage_store(st ^ 1);
      if (ch + 2 < ce) { r0 = g0[4 * ch + 8]; r1 = g1[4 * ch + 8]; r2 = g2[4 * ch + 8]; r3 = g3[4 * ch + 8]; }
      __syncthreads();  // everybody has read stage st and written stage st ^ 1
    }
    if (any && SUP) {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 256 * IB + 64 * wi + 32 * ii + l31;
        const int e_row = p.rp[p.base + i];
        const unsigned short *__restrict__ fr = p.first_pos + (size_t)i * (size_t)rw + 8 * JB + 4 * wj;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const unsigned w = mw[jj][ii];
          if (w == 0u) continue;
          const int e_word = e_row + (int)fr[jj];
#pragma unroll
          for (int r = 0; r < 16; ++r) {  // register r of this lane: bit (r & 3) + 8 (r >> 2) + 4 h of the word
            const int b = (r & 3) + 8 * (r >> 2) + 4 * h;
            const unsigned v = (unsigned)acc[jj][ii][r];
            if (((w >> b) & 1u) && v) atomicAdd(&p.sup[e_word + __builtin_popcount(w & ((1u << b) - 1u))], v);
          }
        }
      }
    } else if (any) {
      float s = 0.f;  // <= 8 tiles x 16 registers x 8192 columns of a piece: exact in f32
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) s += ctc_masked_sum(acc[jj][ii], mw[jj][ii] >> (4 * h));
      c += (unsigned)s;
      if (c > 0x7fffffffu) {
        tot += (unsigned long long)c;
        c = 0;
      }
    }
  }
  if (SUP) return;
  tot += (unsigned long long)c;
  const unsigned long long s0 = wave_sum_u64(tot);  // one atomic per workgroup (same-address atomics queue up, ~10 ns each)
  __syncthreads();
  unsigned long long *part = reinterpret_cast<unsigned long long *>(S.pan);
  if (lane == 0) part[wave] = s0;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kCtcBWaves; ++w) t += part[w];
    if (t) atomicAdd(&p.counters[0], t);
  }
}

bool core_tc_fast_path(const CoreTcParams &p) {  // whole chunks of 512 columns, rows and the corner 16-byte aligned
  return p.h >= 512 && p.h % 512 == 0 && p.row_words % 4 == 0 && p.word0 % 4 == 0 && (reinterpret_cast<uintptr_t>(p.core) & 15u) == 0;
}

// p.first / p.step = the rank and the world of the launch (every world-th task); ntasks is filled in here
hipError_t launch_core_tc(CoreTcParams p, int cu_count, hipStream_t stream) {
  static_assert(sizeof(CtcBlockLds) <= 163840, "one workgroup per CU (two waves per SIMD: 246 registers), static LDS");
  static_assert(kCtcBPiece * 512 * 128 < (1 << 24), "a piece's masked sum stays exact in f32");
  static_assert(kCtcBPieceSup * 512 < (1 << 24), "an accumulator of a supports' piece stays exact in f32");
  if (p.core == nullptr || p.h < 1 || p.h > kCtcMaxH || p.step < 1 || p.first < 0 || p.first >= p.step) return hipErrorInvalidValue;
  const bool fast = core_tc_fast_path(p);
  if (p.tasks != nullptr && (!fast || p.n_list < 0)) return hipErrorInvalidValue;  // (a list of block pairs: the block kernel only)
  const int nJ = (p.h + 63) >> 6;
  p.ntasks = p.tasks != nullptr ? p.n_list : (fast ? ctc_block_tasks(p.h) : nJ * (nJ + 1) / 2);
  const long long mine = ((long long)p.ntasks - p.first + p.step - 1) / p.step;
  if (mine <= 0) return hipSuccess;
  if (fast) {
    const int grid = (int)std::max<long long>(1, std::min<long long>(mine, (long long)cu_count));
    hipLaunchKernelGGL((core_tc_block_kernel<false>), dim3((unsigned)grid), dim3(kCtcBWaves * GM_WAVE), 0, stream, p);
  } else {
    const int grid = (int)std::max<long long>(1, std::min<long long>((mine + kCtcWaves - 1) / kCtcWaves, (long long)cu_count * 3));
    hipLaunchKernelGGL(core_tc_kernel, dim3((unsigned)grid), dim3(kCtcWaves * GM_WAVE), 0, stream, p);
  }
  return hipGetLastError();
}

// ---- the symmetric corner of the edge supports: A = M + M^T as a bit matrix of its own (h / 32 words per row) and, per (row, word), the
// position inside the row's DAG entries of the first entry whose bit lies in that word (rows of at most kTctStageMax entries)
__global__ __launch_bounds__(256) void core_sym_fill_kernel(int nv, int base, int words, long long e0, long long e1, const int *__restrict__ rp,
                                                             const int *__restrict__ col, unsigned *__restrict__ bits, unsigned short *__restrict__ first_pos) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = e0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
    int lo = base, hi = nv - 1;  // the row of entry e
    while (lo < hi) {
      const int mid = (int)(((long long)lo + hi + 1) >> 1);
      if (rp[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int u = lo - base, v = col[e] - base;  // (topological: v > u >= 0)
    atomicOr(&bits[(size_t)u * (size_t)words + (size_t)(v >> 5)], 1u << (v & 31));
    atomicOr(&bits[(size_t)v * (size_t)words + (size_t)(u >> 5)], 1u << (u & 31));
    const long long er = (long long)rp[lo];
    if (e == er || ((col[e - 1] - base) >> 5) != (v >> 5)) first_pos[(size_t)u * (size_t)words + (size_t)(v >> 5)] = (unsigned short)(e - er);
  }
}
hipError_t launch_core_sym_fill(int nv, int base, int words, long long e0, long long e1, const int *rp, const int *col, unsigned *bits,
                                unsigned short *first_pos, int cu_count, hipStream_t stream) {
  if (e1 <= e0) return hipSuccess;
  const long long blocks = std::min<long long>((e1 - e0 + 255) / 256, (long long)cu_count * 32);
  hipLaunchKernelGGL(core_sym_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, nv, base, words, e0, e1, rp, col, bits, first_pos);
  return hipGetLastError();
}
// the supports of the corner's edges: p.core = the symmetric corner (row_words = h / 32, row0 = word0 = 0), p.rp / p.base / p.first_pos / p.sup
hipError_t launch_core_sup(CoreTcParams p, int cu_count, hipStream_t stream) {
  if (p.core == nullptr || p.sup == nullptr || p.first_pos == nullptr || p.rp == nullptr || p.h < 512 || p.h % 512 != 0 || p.h > kCtcMaxH ||
      p.row_words != p.h / 32 || p.row0 != 0 || p.word0 != 0 || p.step < 1 || p.first < 0 || p.first >= p.step)
    return hipErrorInvalidValue;
  const int nb = p.h >> 8, nc = p.h >> 9;
  p.ntasks = nb * (nb + 1) / 2 * ((nc + kCtcBPieceSup - 1) / kCtcBPieceSup);
  const long long mine = ((long long)p.ntasks - p.first + p.step - 1) / p.step;
  if (mine <= 0) return hipSuccess;
  const int grid = (int)std::max<long long>(1, std::min<long long>(mine, (long long)cu_count));
  hipLaunchKernelGGL((core_tc_block_kernel<true>), dim3((unsigned)grid), dim3(kCtcBWaves * GM_WAVE), 0, stream, p);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_ctc_kernel() {}
void gm_touch_ctc() { hipLaunchKernelGGL(gm_touch_ctc_kernel, dim3(1), dim3(1), 0, 0); }
