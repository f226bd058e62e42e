// gm_rect_local.hip -- local 4-cycle counts (gm_rect_local; DESIGN.md "Local 4-cycle counts"): the 4-cycles on every entry of the graph the
// walk runs on, and their way back to the caller's entries.
//   rect_local_kernel      the pruned enumeration of wrect_kernel (gm_wrect.hip; rectangle.h:1-11): a centre v0 and an end x < v0 define
//                          P = {p in N(v0) ^ N(x) : p < v0}, n = |P|, and every 4-cycle v0 - p - x - q has exactly one such (v0, x) -- v0 its
//                          largest id, x the vertex opposite.  Of the C(n, 2) cycles of a pair each of the 2 n edges (v0, p), (p, x) lies in
//                          n - 1.  A workgroup keeps ONE 32-bit counter per id of one range in LDS and makes three steps per (centre, range):
//                            walk 1  v0 -> p -> x: c(x) += 1 (a non-returning LDS atomic per arrival)
//                            walk 2  (after a barrier) the same keys again: where c(x) >= 2, c(x) - 1 is added to acc[the key's own position
//                                    in row p] (the entry p -> x: no search; consecutive keys of a row are consecutive addresses) and to the
//                                    spoke sum of row p, a 64-bit LDS accumulator per row of the wave
//                            clear   a sweep of the range with 16-byte stores (the walks of a centre touch a small part of a range on a
//                                    sparse graph, but a third walk would cost what the second does; the sweep is 4 stores per thread)
//                          The spoke sum of row p belongs to the entry v0 -> p = rp[v0] + (the row's index in the centre's row): a one-task
//                          centre adds it once after all of its ranges, a per-range task of a hub centre once per (row, range) where it is
//                          not zero -- the ranges of a hub run on different workgroups.  Tasks, masks and idx0 are wrect_kernel's (gm_centre_plan.h
//                          wrect_tasks, wrect_mask_kernel): {v0, -1} every range of a centre with at most one neighbour below it per thread,
//                          from the top down; {v0, k} range k of a centre with more.
//                          Most ends of a sparse graph are reached once: c(x) < 2 costs one LDS read in walk 2 and nothing else.
//   rect_local_map_kernel  per entry (u, v) of the CALLER's symmetric CSR (a lane each, the row as local_map_kernel finds it): both ends through
//                          the numbering of the copy, the two entries a -> b and b -> a by one bisection each, the sum of their credits to
//                          the caller's entry index; the sum of all of them is 8 R
// Everything is uint64 arithmetic modulo 2^64; the global adds are atomicAdd(unsigned long long *) with unused results, so the arrays do not
// depend on the order in which the workgroups arrive.  Plain HIP atomics and vector stores only.
#include "gm_setops.h"
#include "gm_mine.h"

namespace gm {

struct alignas(16) RectLocalLds {
  unsigned n[kRectLocalRange];                             // per end of the range: its 2-paths from the centre
  unsigned long long spk[kRectLocalWaves][GM_WAVE];        // per row of the wave: the credits of its spoke v0 -> p
  int off[kRectLocalWaves][GM_WAVE], kb[kRectLocalWaves][GM_WAVE];  // the rows of a wave, flattened over its lanes
  int red[kRectLocalWaves];
  int2 task;
};
static_assert(kRectLocalRange % 4 == 0, "the clearing sweep stores four counters at a time");
static_assert(sizeof(RectLocalLds) <= 65536, "a statically sized LDS block");

// The keys [kb, kb + llen) of this wave's 64 rows against the counters of the range that starts at lo.  PASS 0: c(x) += 1.  PASS 1: where
// c(x) >= 2, c(x) - 1 to the key's entry and to the row's spoke sum.  Called by every lane of the wave (the scan is a DPP scan).
template <int PASS>
__device__ __forceinline__ void rect_local_walk(RectLocalLds &S, const int *__restrict__ col, unsigned long long *__restrict__ acc, const int wave,
                                                const int lane, const int kb, int llen, const int lo) {
  unsigned long long lm = __ballot(llen >= kRectLocalLong);
  while (lm) {  // wave-uniform
    const int l = __ffsll((long long)lm) - 1;
    lm &= lm - 1ull;
    const int base = readlane(kb, l), len = readlane(llen, l);
    unsigned long long part = 0;
    for (int j0 = 0; j0 < len; j0 += 4 * GM_WAVE) {
      int key[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) key[q] = col[base + min(j0 + q * GM_WAVE + lane, len - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = j0 + q * GM_WAVE + lane;
        if (j < len) {
          const unsigned o = (unsigned)(key[q] - lo);
          if (PASS == 0) {
            atomicAdd(&S.n[o], 1u);  // (result unused: ds_add_u32)
          } else {
            const unsigned c = S.n[o];
            if (c >= 2u) {
              atomicAdd(&acc[base + j], (unsigned long long)(c - 1u));  // (result unused; a wave's adds of one step are contiguous)
              part += (unsigned long long)(c - 1u);
            }
          }
        }
      }
    }
    if (PASS == 1) {
      part = wave_sum_u64(part);
      if (lane == 0 && part) atomicAdd(&S.spk[wave][l], part);
    }
  }
  if (llen >= kRectLocalLong) llen = 0;
  const int incl = wave_incl_scan_add(llen);
  const int total = readlane(incl, GM_WAVE - 1);  // (< 64 * kRectLocalLong)
  if (total == 0) return;                         // wave-uniform
  wave_sync();
  S.off[wave][lane] = incl - llen;
  S.kb[wave][lane] = kb;
  wave_sync();
  for (int pp = lane; pp < total; pp += GM_WAVE) {
    int a = 0, b = GM_WAVE - 1;  // the row of key pp: the largest lane whose offset is <= pp (rows without keys share the offset of the next one)
    while (a < b) {
      const int mid = (a + b + 1) >> 1;
      if (S.off[wave][mid] <= pp) a = mid; else b = mid - 1;
    }
    const int e = S.kb[wave][a] + (pp - S.off[wave][a]);
    const unsigned o = (unsigned)(col[e] - lo);
    if (PASS == 0) {
      atomicAdd(&S.n[o], 1u);
    } else {
      const unsigned c = S.n[o];
      if (c >= 2u) {
        atomicAdd(&acc[e], (unsigned long long)(c - 1u));
        atomicAdd(&S.spk[wave][a], (unsigned long long)(c - 1u));  // (the lane of a key is not the lane of its row)
      }
    }
  }
  wave_sync();
}

__global__ __launch_bounds__(kRectLocalThreads) void rect_local_kernel(const RectLocalParams p) {
  __shared__ RectLocalLds S;
  const int *__restrict__ rp = p.rp;
  const int *__restrict__ col = p.col;
  const int lane = threadIdx.x & (GM_WAVE - 1), wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int W = p.range;
  for (int i = tid; i < kRectLocalRange; i += kRectLocalThreads) S.n[i] = 0u;
  // every wave is done with the range [lo, hi) (a barrier lies between): the counters cleared, four at a time (hi - lo <= kRectLocalRange)
  auto clear = [&](const int lo, const int hi) {
    for (int i = 4 * tid; i < hi - lo; i += 4 * kRectLocalThreads) *reinterpret_cast<uint4 *>(&S.n[i]) = make_uint4(0u, 0u, 0u, 0u);
  };
  for (;;) {
    if (tid == 0) {
      const unsigned long long q = atomicAdd(p.queue, 1ull);
      S.task = q < p.count ? p.tasks[q] : make_int2(-1, -1);
    }
    __syncthreads();
    const int2 t = S.task;
    if (t.x < 0) break;
    const int v0 = t.x;
    const int r0 = rp[v0], nitems = p.idx0[v0];
    if (t.y >= 0) {  // ---- one range of a centre with many neighbours below it: the rows in batches of one per thread
      const int k = t.y, lo = k * W, hi = min(lo + W, v0);
      const int bit = k / p.grp;
      // row i of the centre cut to the range (two bisections, after the row's mask has said that it has a key in the range's group at all)
      auto cut = [&](const int i, int &kb, int &llen) {
        kb = 0;
        llen = 0;
        if (i < nitems) {
          const int x = col[r0 + i];
          if ((p.rmask[x] >> bit) & 1ull) {
            const int rb = rp[x], dp = rp[x + 1] - rb;
            const int a = lower_bound(col + rb, dp, lo);
            llen = lower_bound(col + rb + a, dp - a, hi);
            kb = rb + a;
          }
        }
      };
      int any = 0;
      for (int base = wave * GM_WAVE; base < nitems; base += kRectLocalThreads) {  // (wave-uniform)
        int kb, llen;
        cut(base + lane, kb, llen);
        any |= llen;
        rect_local_walk<0>(S, col, p.acc, wave, lane, kb, llen, lo);
      }
      if (__syncthreads_or(any)) {  // (workgroup-uniform)
        for (int base = wave * GM_WAVE; base < nitems; base += kRectLocalThreads) {
          int kb, llen;
          cut(base + lane, kb, llen);
          if (__ballot(llen > 0) == 0ull) continue;  // (wave-uniform)
          S.spk[wave][lane] = 0ull;
          wave_sync();
          rect_local_walk<1>(S, col, p.acc, wave, lane, kb, llen, lo);
          wave_sync();
          const unsigned long long s = S.spk[wave][lane];
          if (s) atomicAdd(&p.acc[r0 + base + lane], s);  // (only a row with keys has a sum: base + lane < nitems)
          wave_sync();
        }
        __syncthreads();
        clear(lo, hi);
      }
      __syncthreads();
    } else {  // ---- every range of a centre with at most one neighbour below it per thread, from the top down
      const int row = lane * kRectLocalWaves + wave;  // (a centre with 100 neighbours gives every wave 25 rows)
      const bool valid = row < nitems;
      const int x = valid ? col[r0 + row] : 0;
      const int rb = valid ? rp[x] : 0, dp = valid ? rp[x + 1] - rb : 0;
      int ke = valid ? rb + lower_bound(col + rb, dp, v0) : 0;  // the keys below v0
      S.spk[wave][lane] = 0ull;
      wave_sync();
      for (;;) {
        const int top = ke > rb ? col[ke - 1] + 1 : 0;  // the largest key left in this row, + 1
        const int m = wave_max_nonneg(top);
        if (lane == 0) S.red[wave] = m;
        __syncthreads();
        int mm = 0;
#pragma unroll
        for (int w = 0; w < kRectLocalWaves; ++w) mm = max(mm, S.red[w]);
        if (mm == 0) break;  // (workgroup-uniform)
        const int lo = ((mm - 1) / W) * W, hi = min(lo + W, v0);
        const int kb = rb + lower_bound(col + rb, ke - rb, lo);
        rect_local_walk<0>(S, col, p.acc, wave, lane, kb, ke - kb, lo);
        __syncthreads();
        rect_local_walk<1>(S, col, p.acc, wave, lane, kb, ke - kb, lo);
        ke = kb;
        __syncthreads();
        clear(lo, hi);
        __syncthreads();
      }
      wave_sync();
      const unsigned long long s = S.spk[wave][lane];
      if (s) atomicAdd(&p.acc[r0 + row], s);  // (only a valid row has a sum)
      wave_sync();
    }
  }
}

// block-wide sum of one lane-private 64-bit value -> one atomic per workgroup (256 threads, every lane active)
__device__ __forceinline__ void rect_local_block_add(unsigned long long v, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long part[4];
  const unsigned long long s = wave_sum_u64(v);
  if ((threadIdx.x & (GM_WAVE - 1)) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = part[0] + part[1] + part[2] + part[3];
    if (t) atomicAdd(out, t);
  }
}

__global__ __launch_bounds__(256) void rect_local_map_kernel(const RectLocalMapParams p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s = 0;
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < p.ne; base += stride) {  // wave-uniform
    const long long e = base + lane;
    const int u = local_wave_row(p.rp, p.nv, p.ne, base, e);
    if (e >= p.ne) continue;
    const int v = p.col[e];
    const int a = p.newid ? p.newid[u] : u, b = p.newid ? p.newid[v] : v;
    unsigned long long t = 0;
    if (a != b) {
      int pos = 0;
      const int ra = p.drp[a], rb = p.drp[b];
      if (contains(p.dcol + ra, p.drp[a + 1] - ra, b, &pos)) t += p.acc[ra + pos];
      if (contains(p.dcol + rb, p.drp[b + 1] - rb, a, &pos)) t += p.acc[rb + pos];
    }
    p.out[e] = t;
    s += t;
  }
  rect_local_block_add(s, p.sum);
}

int rect_local_per_cu() { return (int)std::max<size_t>(1, std::min<size_t>(163840 / sizeof(RectLocalLds), 2048 / kRectLocalThreads)); }
hipError_t launch_rect_local(const RectLocalParams &p, int grid_blocks, hipStream_t stream) {
  if (p.range < 1 || p.range > kRectLocalRange || p.grp < 1 || !p.rmask || !p.idx0 || !p.tasks || !p.acc) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rect_local_kernel, dim3((unsigned)grid_blocks), dim3(kRectLocalThreads), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_rect_local_map(const RectLocalMapParams &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!p.acc || !p.out || !p.sum) return hipErrorInvalidValue;
  const long long blocks = std::max<long long>(1, std::min<long long>((p.ne + 255) / 256, (long long)cu_count * 8));
  hipLaunchKernelGGL(rect_local_map_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_rect_local_kernel() {}
void gm_touch_rect_local() { hipLaunchKernelGGL(gm_touch_rect_local_kernel, dim3(1), dim3(1), 0, 0); }
