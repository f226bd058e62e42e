// gm_nucleus34.hip -- triangle nuclei (gm_tri_clique4_local / gm_nucleus34 / gm_nucleus34_decompose; DESIGN.md "Triangle nuclei"): the
// 4-cliques on every triangle of the caller's SYMMETRIC graph, peeled in whole-frontier rounds into the (3,4)-nuclei.  A triangle's id is
// its slot in gm_tc_list's order: ascending entry (u, v) of the oriented copy, then ascending third vertex w of N+(u) & N+(v).
//   nuc_index_kernel<FILL>  the index, gm_list.hip's two walks per ENTRY instead of per batch: COUNT c(e) = |N+(u) & N+(v)|, a 64-bit scan
//                           (hipCUB) = tri_off, FILL tri_w (the third vertices of every entry's segment, ascending) and tri_e (the entry of
//                           every triangle) at slots tri_off[e] + the ballot rank -- no atomic cursor
//   nuc_count_kernel        K4(t) = |N(u) & N(v) & N(w)| of every triangle, their sum and the smallest of them; the marks alive
//   nuc_mark_kernel         a round, steps 1 + 2 (ktr_mark_kernel over triangles): last round's frontier becomes removed, the alive
//                           triangles below the threshold become the frontier -- one atomic per wave reserves their slots, theta and the
//                           round are written -- and the smallest count that stays is kept
//   nuc_peel_kernel         step 3.  A triangle is BLOCKED for frontier triangle t when it is removed, or in the frontier at an id below
//                           t's.  t = (u, v, w) takes every common neighbour x of its corners, looks up the ids of (u, v, x), (u, w, x),
//                           (v, w, x) and, unless one of them is blocked, adds one to the destroyed total and subtracts one from each of
//                           the three that is outside the frontier
//   nuc_out_kernel          K4(t) inside the nucleus or GM_TRUSS_REMOVED; the survivors and the sum of their counts
// One gather serves the count and the peel (nuc_walk): row u of the symmetric graph is streamed -- the orientation goes by (degree, id), so
// it is the shortest of the three -- and rows v and w are bisected.  A triangle whose row u is below kNucWholeWave entries takes a group of
// kNucGroup lanes, eight triangles to a wave; the longer ones of a wave's eight follow one after the other, strided by the whole wave, their
// descriptors read from the group's first lane.  No LDS, no scratch; the marks do not change while a peel kernel runs, so the result does not
// depend on the order of arrival.  Three 32-bit atomics per destroyed clique at most, one 64-bit atomic per wave.  Plain HIP, vector atomics.
#include "gm_scan.h"

namespace gm {

constexpr int kNucPerWave = GM_WAVE / kNucGroup;  // triangles (entries) of a wave's trip
static_assert(kNucGroup == 8 && kNucPerWave == 8, "the group's share of a ballot is one byte");

template <bool FILL>
__global__ __launch_bounds__(256) void nuc_index_kernel(const NucIndexParams p) {
  const int lane = threadIdx.x & (GM_WAVE - 1), grp = lane / kNucGroup, gl = lane % kNucGroup;
  const long long nb = (p.ne + kNucPerWave - 1) / kNucPerWave;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long b = wave0; b < nb; b += nwaves) {  // wave-uniform
    const long long e = b * kNucPerWave + grp;
    const bool live = e < p.ne;
    const long long ec = min(e, p.ne - 1);
    const int u = local_row_of(p.rp, p.nv, ec), v = p.col[ec];
    const int ru = p.rp[u], du = p.rp[u + 1] - ru, rv = p.rp[v], dv = p.rp[v + 1] - rv;
    const bool u_short = du <= dv;
    const int sb = u_short ? ru : rv, lb = u_short ? rv : ru, ln = u_short ? dv : du;
    const int sn = live ? (u_short ? du : dv) : 0;
    const bool whole = sn >= kNucWholeWave;
    unsigned long long at = 0;
    if constexpr (FILL) at = p.off[ec];
    int n = 0;
    {  // the short lists: a group each, in trips of kNucGroup keys (the ranks come from the group's byte of the ballot)
      const int mine = whole ? 0 : sn;
      const int longest = wave_max_nonneg(mine);
      for (int k0 = 0; k0 < longest; k0 += kNucGroup) {  // wave-uniform
        const int k = k0 + gl;
        bool found = false;
        int key = 0;
        if (k < mine) {
          int pos = 0;
          key = p.col[sb + k];
          found = contains(p.col + lb, ln, key, &pos);
        }
        const unsigned m = (unsigned)(__ballot(found) >> (grp * kNucGroup)) & 0xFFu;
        if constexpr (FILL) {
          if (found) {
            const unsigned long long slot = at + (unsigned)(n + __popc(m & ((1u << gl) - 1u)));
            p.tri_w[slot] = key;
            p.tri_e[slot] = (int)e;
          }
        }
        n += __popc(m);
      }
    }
    unsigned long long longs = __ballot(whole && gl == 0);
    while (longs) {  // wave-uniform: the long lists, the whole wave each
      const int src = readfirst((int)__builtin_ctzll(longs));
      longs &= longs - 1ull;
      const int s_b = readlane(sb, src), s_n = readlane(sn, src), l_b = readlane(lb, src), l_n = readlane(ln, src), ee = readlane((int)e, src);
      const unsigned long long at2 = ((unsigned long long)(unsigned)readlane((int)(at >> 32), src) << 32) | (unsigned)readlane((int)at, src);
      int nn = 0;
      for (int t = 0; t < s_n; t += GM_WAVE) {
        const bool in = t + lane < s_n;
        const int key = p.col[s_b + (in ? t + lane : 0)];
        int pos = 0;
        const bool found = in && contains(p.col + l_b, l_n, key, &pos);
        const unsigned long long m = __ballot(found);
        if constexpr (FILL) {
          if (found) {
            const unsigned long long slot = at2 + (unsigned)(nn + rank_below(m));
            p.tri_w[slot] = key;
            p.tri_e[slot] = ee;
          }
        }
        nn += (int)__popcll(m);
      }
      if (lane == src) n = nn;
    }
    if constexpr (!FILL) {
      if (live && gl == 0) p.cnt[e] = (unsigned long long)n;
    }
  }
}

// ---- the gather: the common neighbours of a triangle's corners ------------------------------------------------------------------------------
// u -> v -> w in the orientation's order, the symmetric rows of the three
struct NucTri {
  int u, v, w, ru, du, rv, dv, rw, dw;
};
__device__ __forceinline__ NucTri nuc_tri(const Nuc34Params &p, const unsigned t) {
  NucTri tr;
  const int e = p.tri_e[t];
  tr.u = local_row_of(p.drp, p.nv, e);
  tr.v = p.dcol[e];
  tr.w = p.tri_w[t];
  tr.ru = p.rp[tr.u]; tr.du = p.rp[tr.u + 1] - tr.ru;
  tr.rv = p.rp[tr.v]; tr.dv = p.rp[tr.v + 1] - tr.rv;
  tr.rw = p.rp[tr.w]; tr.dw = p.rp[tr.w + 1] - tr.rw;
  return tr;
}
// f(x) for the common neighbours x at the positions first, first + step, ... of row u, in the lane that met them
template <class F>
__device__ __forceinline__ void nuc_common(const Nuc34Params &p, const NucTri &tr, const int first, const int step, F f) {
  for (int k = first; k < tr.du; k += step) {
    const int x = p.col[tr.ru + k];
    int pos = 0;
    if (x == tr.u || x == tr.v || x == tr.w) continue;  // (a self loop)
    if (contains(p.col + tr.rv, tr.dv, x, &pos) && contains(p.col + tr.rw, tr.dw, x, &pos)) f(x);
  }
}
// The triangles ids(0 .. n), eight to a wave's trip: f(tr, t, x) for every common neighbour x of triangle t, then done(t, how many there
// were) in the first lane of t's group.  Every lane of the workgroup calls it.
template <class Ids, class F, class D>
__device__ __forceinline__ void nuc_walk(const Nuc34Params &p, const unsigned long long n, Ids ids, F f, D done) {
  const int lane = threadIdx.x & (GM_WAVE - 1), grp = lane / kNucGroup, gl = lane % kNucGroup;
  const unsigned long long nb = (n + kNucPerWave - 1) / kNucPerWave;
  const unsigned long long wave0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
  for (unsigned long long b = wave0; b < nb; b += nwaves) {  // wave-uniform
    const unsigned long long i = b * kNucPerWave + grp;
    const bool live = i < n;
    const unsigned t = ids(live ? i : n - 1);
    const NucTri tr = nuc_tri(p, t);
    const bool whole = live && tr.du >= kNucWholeWave;
    unsigned c = 0;
    if (live && !whole)
      nuc_common(p, tr, gl, kNucGroup, [&](const int x) {
        ++c;
        f(tr, t, x);
      });
    for (int o = 1; o < kNucGroup; o <<= 1) c += (unsigned)__shfl_xor((int)c, o, GM_WAVE);
    unsigned long long longs = __ballot(whole && gl == 0);
    while (longs) {  // wave-uniform: the whole wave on one triangle, its descriptor out of the group's first lane
      const int src = readfirst((int)__builtin_ctzll(longs));
      longs &= longs - 1ull;
      NucTri lt;
      lt.u = readlane(tr.u, src); lt.v = readlane(tr.v, src); lt.w = readlane(tr.w, src);
      lt.ru = readlane(tr.ru, src); lt.du = readlane(tr.du, src);
      lt.rv = readlane(tr.rv, src); lt.dv = readlane(tr.dv, src);
      lt.rw = readlane(tr.rw, src); lt.dw = readlane(tr.dw, src);
      const unsigned t2 = (unsigned)readlane((int)t, src);
      int cc = 0;
      nuc_common(p, lt, lane, GM_WAVE, [&](const int x) {
        ++cc;
        f(lt, t2, x);
      });
      cc = wave_sum(cc);
      if (lane == src) c = (unsigned)cc;
    }
    if (live && gl == 0) done(t, c);
  }
}

__global__ __launch_bounds__(256) void nuc_count_kernel(const Nuc34Params p, unsigned *__restrict__ out) {
  unsigned long long sum = 0;
  unsigned least = ~0u;
  nuc_walk(
      p, p.nt, [](const unsigned long long i) { return (unsigned)i; }, [](const NucTri &, const unsigned, const int) {},
      [&](const unsigned t, const unsigned c) {
        out[t] = c;
        if (p.mark) p.mark[t] = LM_ALIVE;
        sum += c;
        least = min(least, c);
      });
  sum = wave_sum_u64(sum);
  for (int o = 32; o >= 1; o >>= 1) least = min(least, (unsigned)__shfl_xor((int)least, o, GM_WAVE));
  if ((threadIdx.x & (GM_WAVE - 1)) == 0) {
    if (sum) atomicAdd(&p.words[NW_TOTAL], sum);
    if (least != ~0u) atomicMax(&p.words[CW_LEAST], ~0ull - (unsigned long long)least);
  }
}

__global__ __launch_bounds__(256) void nuc_mark_kernel(const Nuc34Params p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned least = ~0u;
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < p.nt; base += stride) {  // wave-uniform
    const unsigned long long t = base + lane;
    bool enters = false;
    if (t < p.nt) {
      const unsigned char m = p.mark[t];
      if (m == LM_FRONTIER) {
        p.mark[t] = LM_REMOVED;
      } else if (m == LM_ALIVE) {
        const unsigned s = p.cnt[t];
        enters = s < p.thr;
        if (enters) {
          p.mark[t] = LM_FRONTIER;
          if (p.theta) p.theta[t] = p.level;
          if (p.round) p.round[t] = p.round_no;
        } else {
          least = min(least, s);
        }
      }
    }
    const unsigned long long bm = __ballot(enters);
    if (bm) {  // one atomic per wave: the leader reserves the slots of the list
      const int leader = readfirst((int)__builtin_ctzll(bm));
      unsigned at = 0;
      if (lane == leader) at = (unsigned)atomicAdd(&p.words[CW_FRONT], (unsigned long long)__popcll(bm));
      at = (unsigned)readlane((int)at, leader);
      if (enters) p.front[at + (unsigned)rank_below(bm)] = (unsigned)t;
    }
  }
  for (int o = 32; o >= 1; o >>= 1) least = min(least, (unsigned)__shfl_xor((int)least, o, GM_WAVE));
  if (lane == 0 && least != ~0u) atomicMax(&p.words[CW_LEAST], ~0ull - (unsigned long long)least);
}

// ---- the ids of a frontier triangle's siblings ----------------------------------------------------------------------------------------------
// a comes before b in the orientation's order: by (symmetric degree, id)
__device__ __forceinline__ bool nuc_below(const int da, const int a, const int db, const int b) { return da < db || (da == db && a < b); }
// the id of the triangle a -> b -> c, which exists: b bisected in row a of the oriented copy, c in the segment of that entry
__device__ __forceinline__ bool nuc_tri_id(const Nuc34Params &p, const int a, const int b, const int c, unsigned *id) {
  const int r0 = p.drp[a];
  int pos = 0;
  if (!contains(p.dcol + r0, p.drp[a + 1] - r0, b, &pos)) return false;
  const int e = r0 + pos;
  const unsigned long long o0 = p.tri_off[e];
  const int n = (int)(p.tri_off[e + 1] - o0);
  if (!contains(p.tri_w + o0, n, c, &pos)) return false;
  *id = (unsigned)(o0 + (unsigned)pos);
  return true;
}
// ... of the triangle {a, b, x}, a before b
__device__ __forceinline__ bool nuc_id_with(const Nuc34Params &p, const int a, const int da, const int b, const int db, const int x, const int dx,
                                            unsigned *id) {
  if (nuc_below(dx, x, da, a)) return nuc_tri_id(p, x, a, b, id);
  if (nuc_below(dx, x, db, b)) return nuc_tri_id(p, a, x, b, id);
  return nuc_tri_id(p, a, b, x, id);
}
__device__ __forceinline__ bool nuc_blocked(const unsigned char m, const unsigned id, const unsigned t) {
  return m == LM_REMOVED || (m == LM_FRONTIER && id < t);
}

__global__ __launch_bounds__(256) void nuc_peel_kernel(const Nuc34Params p, const unsigned n_front) {
  unsigned long long destroyed = 0;
  nuc_walk(
      p, n_front, [&](const unsigned long long i) { return p.front[i]; },
      [&](const NucTri &tr, const unsigned t, const int x) {
        const int dx = p.rp[x + 1] - p.rp[x];
        unsigned i1 = 0, i2 = 0, i3 = 0;
        if (!nuc_id_with(p, tr.u, tr.du, tr.v, tr.dv, x, dx, &i1) || !nuc_id_with(p, tr.u, tr.du, tr.w, tr.dw, x, dx, &i2) ||
            !nuc_id_with(p, tr.v, tr.dv, tr.w, tr.dw, x, dx, &i3)) {
          atomicAdd(&p.words[CW_ERR], 1ull);  // (cannot happen: the three are triangles of the graph)
          return;
        }
        const unsigned char m1 = p.mark[i1], m2 = p.mark[i2], m3 = p.mark[i3];
        if (nuc_blocked(m1, i1, t) || nuc_blocked(m2, i2, t) || nuc_blocked(m3, i3, t)) return;
        ++destroyed;
        if (m1 == LM_ALIVE) atomicSub(&p.cnt[i1], 1u);
        if (m2 == LM_ALIVE) atomicSub(&p.cnt[i2], 1u);
        if (m3 == LM_ALIVE) atomicSub(&p.cnt[i3], 1u);
      },
      [](const unsigned, const unsigned) {});
  destroyed = wave_sum_u64(destroyed);
  if ((threadIdx.x & (GM_WAVE - 1)) == 0 && destroyed) atomicAdd(&p.words[CW_DESTROYED], destroyed);
}

__global__ __launch_bounds__(256) void nuc_out_kernel(const Nuc34Params p, unsigned *__restrict__ out) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long alive = 0, sum = 0;
  for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < p.nt; t += stride) {
    const bool in = p.mark[t] == LM_ALIVE;
    const unsigned k = in ? p.cnt[t] : 0xFFFFFFFFu;
    if (out) out[t] = k;
    alive += in ? 1ull : 0ull;
    sum += in ? (unsigned long long)k : 0ull;
  }
  alive = wave_sum_u64(alive);
  sum = wave_sum_u64(sum);
  if ((threadIdx.x & (GM_WAVE - 1)) == 0) {
    if (alive) atomicAdd(&p.words[CW_ALIVE], alive);
    if (sum) atomicAdd(&p.words[CW_SUM], sum);
  }
}

static inline dim3 nuc_grid(unsigned long long n, unsigned long long per_block, int cu_count) {
  return dim3((unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((n + per_block - 1) / per_block, (unsigned long long)cu_count * 8)));
}
static bool nuc_params_ok(const Nuc34Params &p) {
  return p.rp && p.col && p.drp && p.dcol && p.tri_off && p.tri_w && p.tri_e && p.words && p.nt < 0xFFFFFFFFull;
}

hipError_t launch_nuc_index(const NucIndexParams &p, bool fill, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!p.rp || !p.col || p.ne >= (1ll << 31) || (fill ? (!p.off || !p.tri_w || !p.tri_e) : !p.cnt)) return hipErrorInvalidValue;
  const dim3 grid = nuc_grid((unsigned long long)p.ne, 4 * kNucPerWave, cu_count);
  if (fill) hipLaunchKernelGGL(nuc_index_kernel<true>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(nuc_index_kernel<false>, grid, dim3(256), 0, stream, p);
  return hipGetLastError();
}
// Synchronises the stream (the temporaries go back).
hipError_t nuc_index_scan(const unsigned long long *cnt, unsigned long long *off, size_t n, hipStream_t stream) {
  ScanTemp tmp;
  const hipError_t e = dev_exclusive_sum(tmp, cnt, off, n, stream);
  return e != hipSuccess ? e : hipStreamSynchronize(stream);
}
hipError_t launch_nuc_count(const Nuc34Params &p, unsigned *out, int cu_count, hipStream_t stream) {
  if (p.nt == 0) return hipSuccess;
  if (!nuc_params_ok(p) || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nuc_count_kernel, nuc_grid(p.nt, 4 * kNucPerWave, cu_count), dim3(256), 0, stream, p, out);
  return hipGetLastError();
}
hipError_t launch_nuc_mark(const Nuc34Params &p, int cu_count, hipStream_t stream) {
  if (p.nt == 0) return hipSuccess;
  if (!nuc_params_ok(p) || !p.cnt || !p.mark || !p.front) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nuc_mark_kernel, nuc_grid(p.nt, 256, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_nuc_peel(const Nuc34Params &p, unsigned n_front, int cu_count, hipStream_t stream) {
  if (n_front == 0) return hipSuccess;
  if (!nuc_params_ok(p) || !p.cnt || !p.mark || !p.front || (unsigned long long)n_front > p.nt) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nuc_peel_kernel, nuc_grid(n_front, 4 * kNucPerWave, cu_count), dim3(256), 0, stream, p, n_front);
  return hipGetLastError();
}
hipError_t launch_nuc_out(const Nuc34Params &p, unsigned *out, int cu_count, hipStream_t stream) {
  if (p.nt == 0) return hipSuccess;
  if (!nuc_params_ok(p) || !p.cnt || !p.mark) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nuc_out_kernel, nuc_grid(p.nt, 256, cu_count), dim3(256), 0, stream, p, out);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_nucleus34_kernel() {}
void gm_touch_nucleus34() { hipLaunchKernelGGL(gm_touch_nucleus34_kernel, dim3(1), dim3(1), 0, 0); }
