// gm_local.hip -- local triangle counts and the k-truss (gm_tc_local / gm_ktruss / gm_truss_decompose; DESIGN.md "Local counts and k-truss").
// The supports t(e) = |N(u) ^ N(v)| come from the triangle pass of the oriented copy (gm_sup.hip, unchanged), one per DAG entry of the copy
// the pass ran on.  The kernels here bring them back to the caller and peel:
//   local_map_kernel       per entry (u, v) of the CALLER's symmetric CSR (a lane each; the row from two bisections per WAVE): both ends through the numbering of the renumbered copy, the DAG
//                          entry by a bisection of the renumbered row (the row of the smaller end under a topological numbering, else
//                          either row), its support to the caller's entry index; the sum of all of them is 6 T
//                          (a template on the value: 32-bit supports, or the 64-bit k-clique counts of gm_clique_local)
//   local_vertex_kernel    T_v = 1/2 sum of the supports of row v in 64 bits: a lane per short row, the whole wave per long one
//                          (64-bit values: the sum / (k - 1), the k-cliques at a vertex)
//   local_rev_kernel       once per handle: per entry (u, v) the index of (v, u).  An undirected edge lives at its CANONICAL entry
//                          min(e, rev[e]) -- the one in the row of its smaller end
//   local_mark_kernel      a round, steps 1 + 2: last round's frontier becomes removed, the alive edges below the threshold become the
//                          frontier (appended to a list, counted), the smallest support that stays is kept for the level jump
//   local_peel_kernel      step 3: one wave per frontier edge (u, v) streams the shorter of N(u), N(v) and bisects the longer one
//                          (gm_setops.h); the marks do not change while it runs, so every wave sees the state the round began with
//   local_truss_out_kernel both directions of every edge: its support inside the truss / GM_TRUSS_REMOVED, or its trussness
// The rule of the decrements: a triangle counts only if its other two edges were not removed when the round began; a surviving edge loses
// one per destroyed triangle -- issued by the frontier edge of the triangle, by the one with the smaller canonical entry when there are
// two, by nobody when all three leave.  Plain HIP atomics and vector stores only.
#include "gm_setops.h"
#include "gm_mine.h"

namespace gm {

// (local_row_of / local_row_in / local_wave_row, the row of an entry: gm_setops.h -- the triangle listing takes its batches the same way)

// block-wide sum of one lane-private 64-bit value -> one atomic per workgroup (256 threads, every lane active)
__device__ __forceinline__ void local_block_add(unsigned long long v, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long part[4];
  const unsigned long long s = wave_sum_u64(v);
  if ((threadIdx.x & (GM_WAVE - 1)) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = part[0] + part[1] + part[2] + part[3];
    if (t) atomicAdd(out, t);
  }
}

template <class V>
__global__ __launch_bounds__(256) void local_map_kernel(const LocalMapParamsT<V> p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long s = 0;
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < p.ne; base += stride) {  // wave-uniform
    const long long e = base + lane;
    const int u = local_wave_row(p.rp, p.nv, p.ne, base, e);
    if (e >= p.ne) continue;
    const int v = p.col[e];
    const int a = p.newid ? p.newid[u] : u, b = p.newid ? p.newid[v] : v;
    V t = 0;
    if (a != b) {
      // (topological: the edge is an entry of the row of its smaller end; else it is in one of the two rows)
      int x = p.topo ? min(a, b) : a, y = p.topo ? max(a, b) : b;
      int r0 = p.drp[x], n = p.drp[x + 1] - r0, pos = 0;
      bool found = contains(p.dcol + r0, n, y, &pos);
      if (!found && !p.topo) {
        r0 = p.drp[y];
        n = p.drp[y + 1] - r0;
        found = contains(p.dcol + r0, n, x, &pos);
      }
      if (found) t = p.dsup[r0 + pos];
    }
    p.out[e] = t;
    s += t;
  }
  local_block_add(s, p.sum);
}

// a wave takes 64 consecutive rows: every lane sums its own short row, the rows beyond kLocalShortRow entries are summed by all 64 lanes
// (HALF: half the sum, the triangles at a vertex; else the sum / div, the k-cliques at a vertex with div = k - 1)
template <class V, bool HALF>
__global__ __launch_bounds__(256) void local_vertex_kernel(int nv, const int *__restrict__ rp, const V *__restrict__ sup,
                                                           unsigned long long *__restrict__ tv, const unsigned div) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long base = wave0 * GM_WAVE; base < nv; base += nwaves * GM_WAVE) {
    const long long v = base + lane;
    const int r0 = v < nv ? rp[v] : 0, r1 = v < nv ? rp[v + 1] : 0;
    unsigned long long s = 0;
    if (r1 - r0 <= kLocalShortRow)
      for (int j = r0; j < r1; ++j) s += sup[j];
    unsigned long long longs = __ballot(r1 - r0 > kLocalShortRow);
    while (longs) {  // wave-uniform
      const int l = readfirst((int)__builtin_ctzll(longs));
      longs &= longs - 1ull;
      const int b = readlane(r0, l), e = readlane(r1, l);
      unsigned long long part = 0;
      for (int j = b + lane; j < e; j += GM_WAVE) part += sup[j];
      part = wave_sum_u64(part);
      if (lane == l) s = part;
    }
    if (v < nv) tv[v] = HALF ? s >> 1 : s / (unsigned long long)div;
  }
}

__global__ __launch_bounds__(256) void local_rev_kernel(int nv, long long ne, const int *__restrict__ rp, const int *__restrict__ col,
                                                        int *__restrict__ rev) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < ne; base += stride) {  // wave-uniform
    const long long e = base + lane;
    const int u = local_wave_row(rp, nv, ne, base, e);
    if (e >= ne) continue;
    const int v = col[e];
    const int r0 = rp[v];
    int pos = 0;
    // (a self loop, or an entry without its reverse -- not a symmetric graph: the entry is its own reverse and never an edge)
    rev[e] = (u != v && contains(col + r0, rp[v + 1] - r0, u, &pos)) ? r0 + pos : (int)e;
  }
}

__global__ __launch_bounds__(256) void local_peel_init_kernel(long long ne, const int *__restrict__ rev, unsigned char *__restrict__ mark) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += stride) mark[e] = (long long)rev[e] > e ? LM_ALIVE : LM_REMOVED;
}

__global__ __launch_bounds__(256) void local_mark_kernel(const LocalPeelParams p) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned least = 0xFFFFFFFFu;
  for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < p.ne; base += stride) {  // wave-uniform
    const long long c = base + lane;
    bool enters = false;
    if (c < p.ne && (long long)p.rev[c] > c) {  // a canonical entry
      const unsigned char m = p.mark[c];
      if (m == LM_FRONTIER) {
        p.mark[c] = LM_REMOVED;
      } else if (m == LM_ALIVE) {
        const unsigned s = p.sup[c];
        enters = s < p.thr;
        if (enters) {
          p.mark[c] = LM_FRONTIER;
          if (p.truss) p.truss[c] = p.level;
        } else {
          least = min(least, s);
        }
      }
    }
    const unsigned long long bm = __ballot(enters);
    if (bm) {  // one atomic per wave: the leader reserves the slots of the list
      const int leader = readfirst((int)__builtin_ctzll(bm));
      int at = 0;
      if (lane == leader) at = (int)atomicAdd(&p.cnt[0], (unsigned)__popcll(bm));
      at = readlane(at, leader);
      if (enters) p.front[at + rank_below(bm)] = (int)c;
    }
  }
  // the smallest support that stays: over the wave, over the workgroup, then one atomic per workgroup
  __shared__ unsigned part[4];
  for (int o = 32; o >= 1; o >>= 1) least = min(least, (unsigned)__shfl_xor((int)least, o, 64));
  if (lane == 0) part[threadIdx.x >> 6] = least;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned m = min(min(part[0], part[1]), min(part[2], part[3]));
    if (m != 0xFFFFFFFFu) atomicMax(&p.cnt[1], 0xFFFFFFFFu - m);
  }
}

__global__ __launch_bounds__(256) void local_peel_kernel(const LocalPeelParams p, const unsigned n_front) {
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long i = wave0; i < (long long)n_front; i += nwaves) {
    const int c = p.front[i];
    const int u = local_row_of(p.rp, p.nv, c), v = p.col[c];
    const int ru = p.rp[u], du = p.rp[u + 1] - ru, rv = p.rp[v], dv = p.rp[v + 1] - rv;
    const bool u_short = du <= dv;
    const int sb = u_short ? ru : rv, sn = u_short ? du : dv, lb = u_short ? rv : ru, ln = u_short ? dv : du;
    for (int k = lane; k < sn; k += GM_WAVE) {
      int pos = 0;
      if (!contains(p.col + lb, ln, p.col[sb + k], &pos)) continue;
      const int es = sb + k, el = lb + pos;  // the other two edges of the triangle, as entries of the two rows
      const int cs = min(es, p.rev[es]), cl = min(el, p.rev[el]);
      const unsigned char ms = p.mark[cs], ml = p.mark[cl];
      if (ms == LM_REMOVED || ml == LM_REMOVED) continue;  // the triangle was gone before the round
      const bool fs = ms == LM_FRONTIER, fl = ml == LM_FRONTIER;
      if (!fs && !fl) {
        atomicSub(&p.sup[cs], 1u);
        atomicSub(&p.sup[cl], 1u);
      } else if (fs && !fl) {
        if (c < cs) atomicSub(&p.sup[cl], 1u);
      } else if (fl && !fs) {
        if (c < cl) atomicSub(&p.sup[cs], 1u);
      }
    }
  }
}

__global__ __launch_bounds__(256) void local_truss_out_kernel(const LocalPeelParams p, unsigned *__restrict__ out, unsigned long long *__restrict__ sum) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned long long alive = 0;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < p.ne; e += stride) {
    const int r = p.rev[e];
    const long long c = min(e, (long long)r);
    unsigned val;
    if ((long long)r == e) {
      val = p.truss ? 0u : 0xFFFFFFFFu;  // not an edge
    } else if (p.truss) {
      val = p.truss[c];
    } else {
      const bool in = p.mark[c] == LM_ALIVE;
      val = in ? p.sup[c] : 0xFFFFFFFFu;
      alive += (in && c == e) ? 1ull : 0ull;
    }
    if (out) out[e] = val;
  }
  local_block_add(alive, sum);
}

static inline dim3 local_grid(long long n, long long per_block, int cu_count) {
  return dim3((unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, (long long)cu_count * 8)));
}
hipError_t launch_local_map(const LocalMapParams &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!p.out || !p.dsup || !p.sum) return hipErrorInvalidValue;
  hipLaunchKernelGGL(local_map_kernel<unsigned>, local_grid(p.ne, 256, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_local_map(const LocalMapParams64 &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  if (!p.out || !p.dsup || !p.sum) return hipErrorInvalidValue;
  hipLaunchKernelGGL(local_map_kernel<unsigned long long>, local_grid(p.ne, 256, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_local_vertices(int nv, const int *rp, const unsigned *sup, unsigned long long *tv, int cu_count, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  hipLaunchKernelGGL((local_vertex_kernel<unsigned, true>), local_grid(nv, 256, cu_count), dim3(256), 0, stream, nv, rp, sup, tv, 2u);
  return hipGetLastError();
}
hipError_t launch_local_vertices(int nv, const int *rp, const unsigned long long *cnt, unsigned div, unsigned long long *kv, int cu_count, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  if (div == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL((local_vertex_kernel<unsigned long long, false>), local_grid(nv, 256, cu_count), dim3(256), 0, stream, nv, rp, cnt, kv, div);
  return hipGetLastError();
}
hipError_t launch_local_rev(int nv, long long ne, const int *rp, const int *col, int *rev, int cu_count, hipStream_t stream) {
  if (ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(local_rev_kernel, local_grid(ne, 256, cu_count), dim3(256), 0, stream, nv, ne, rp, col, rev);
  return hipGetLastError();
}
hipError_t launch_local_peel_init(long long ne, const int *rev, unsigned char *mark, int cu_count, hipStream_t stream) {
  if (ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(local_peel_init_kernel, local_grid(ne, 256, cu_count), dim3(256), 0, stream, ne, rev, mark);
  return hipGetLastError();
}
hipError_t launch_local_mark(const LocalPeelParams &p, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(local_mark_kernel, local_grid(p.ne, 256, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_local_peel(const LocalPeelParams &p, unsigned n_front, int cu_count, hipStream_t stream) {
  if (n_front == 0) return hipSuccess;
  hipLaunchKernelGGL(local_peel_kernel, local_grid(n_front, 4, cu_count), dim3(256), 0, stream, p, n_front);
  return hipGetLastError();
}
hipError_t launch_local_truss_out(const LocalPeelParams &p, unsigned *out, unsigned long long *sum, int cu_count, hipStream_t stream) {
  if (p.ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(local_truss_out_kernel, local_grid(p.ne, 256, cu_count), dim3(256), 0, stream, p, out, sum);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_local_kernel() {}
void gm_touch_local() { hipLaunchKernelGGL(gm_touch_local_kernel, dim3(1), dim3(1), 0, 0); }
