// gm_list.hip -- triangle LISTING (gm_tc_list; DESIGN.md "Triangle listing"): every triangle of a symmetric graph once, as three ids of the
// caller's numbering a < b < c, in an order that is fixed for the handle, windowed.  The walk is the triangle count's -- per entry (u, v) of
// the oriented copy the shorter of N+(u), N+(v) is streamed against the longer -- run twice over the same batches of 64 consecutive entries:
//   list_kernel<false>  COUNT: the matches of every batch (64 bits each); an exclusive scan (hipCUB) turns them into the batch's first slot
//   list_kernel<true>   FILL: the same walk; a match's slot = first slot of its batch + its number inside the batch, which is ascending
//                       entry, then ascending position in the streamed list.  Batches whose slots miss the window are not walked
// Short lists do not cost a wave each: the lengths of a run of lists below kListWholeWave keys are scanned across the lanes and the
// (entry, key) pairs dealt to lanes, the owner of a pair found by bisection of the scanned offsets (LDS); a list of kListWholeWave keys or
// more is strided by the whole wave.  The runs and the long lists alternate in entry order, so the matches leave the walk in slot order:
// the rank is a carried base + the 64-bit ballot's rank_below, no atomic cursor.  The longer list is bisected in global memory
// (gm_setops.h): exact for any row length, no stage to fall out of.  Matches are queued in LDS (a ring of 128 triples per wave) and leave
// 64 at a time: 768 contiguous bytes, three dword stores whose lanes cover neighbouring addresses.  Plain HIP, vector stores only.
#include "gm_scan.h"

namespace gm {

struct alignas(16) ListLds {
  int4 desc[GM_WAVE];      // per entry of the batch: {streamed list, searched list, its length, u}
  int v[GM_WAVE];
  int incl[GM_WAVE];       // inclusive scan of the streamed lengths of the current run (0 outside the run)
  int q[3 * 2 * GM_WAVE];  // FILL: the ring of queued triples
};

template <bool FILL>
__global__ __launch_bounds__(256) void list_kernel(const ListParams p) {
  __shared__ ListLds lds[4];
  ListLds &L = lds[threadIdx.x >> 6];
  const int lane = threadIdx.x & (GM_WAVE - 1);
  const long long nb = (p.ne + GM_WAVE - 1) >> 6;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long b = wave0; b < nb; b += nwaves) {  // wave-uniform
    unsigned long long slot0 = 0;  // FILL: the slot of the ring's head
    if constexpr (FILL) {
      const unsigned long long lo = p.off[b], hi = p.off[b + 1];
      if (hi <= p.first || lo >= p.first + p.nw) continue;  // (an empty batch too)
      slot0 = lo;
    }
    const long long base = b << 6, e = base + lane;
    const int u = local_wave_row(p.rp, p.nv, p.ne, base, e);
    const int v = p.col[min(e, p.ne - 1)];
    const int ru = p.rp[u], du = p.rp[u + 1] - ru, rv = p.rp[v], dv = p.rp[v + 1] - rv;
    const bool u_short = du <= dv;
    const int sb = u_short ? ru : rv, lb = u_short ? rv : ru, ln = u_short ? dv : du;
    const int sn = e < p.ne ? (u_short ? du : dv) : 0;
    L.desc[lane] = make_int4(sb, lb, ln, u);
    L.v[lane] = v;
    unsigned cnt = 0;        // COUNT: this lane's matches
    int qn = 0, qhead = 0;   // FILL: queued triples, the ring's head (0 or 64); wave-uniform

    // triples [qhead, qhead + n) of the ring -> slots [slot0, slot0 + n): ints j, j + 64, j + 128 of the run, clipped to the window
    auto flush = [&](const int n) {
      const long long d0 = 3ll * ((long long)slot0 - (long long)p.first), lim = 3ll * (long long)p.nw;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int j = r * GM_WAVE + lane;
        const long long d = d0 + j;
        if (j < 3 * n && d >= 0 && d < lim) p.tri[d] = L.q[3 * qhead + j];
      }
    };
    auto emit = [&](const bool found, const int a0, const int a1, const int a2) {
      if constexpr (!FILL) {
        cnt += found ? 1u : 0u;
      } else {
        const unsigned long long m = __ballot(found);
        if (m == 0ull) return;  // wave-uniform
        if (found) {
          const int lo3 = min(a0, min(a1, a2)), hi3 = max(a0, max(a1, a2));
          const int at = 3 * ((qhead + qn + rank_below(m)) & (2 * GM_WAVE - 1));
          L.q[at] = lo3;
          L.q[at + 1] = a0 ^ a1 ^ a2 ^ lo3 ^ hi3;
          L.q[at + 2] = hi3;
        }
        qn += __popcll(m);
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

    const unsigned long long longs = __ballot(sn >= kListWholeWave);
    for (int seg = 0;;) {  // the run of short lists [seg, end), then the long list `end`
      const unsigned long long rest = seg < GM_WAVE ? longs >> seg : 0ull;
      const int end = rest ? seg + readfirst((int)__builtin_ctzll(rest)) : GM_WAVE;
      const int len = (lane >= seg && lane < end) ? sn : 0;
      const int incl = wave_incl_scan_add(len);
      const int total = readlane(incl, GM_WAVE - 1);
      if (total > 0) {
        L.incl[lane] = incl;
        wave_sync();
        for (int t = 0; t < total; t += GM_WAVE) {
          const int pos = t + lane;
          const bool in = pos < total;
          int own = 0;  // the number of lanes with incl <= pos: the pair's entry
#pragma unroll
          for (int s = GM_WAVE / 2; s >= 1; s >>= 1) own += (L.incl[own + s - 1] <= pos) ? s : 0;
          const int4 d = L.desc[own];
          const int k = pos - (own > 0 ? L.incl[own - 1] : 0);
          const int key = p.col[in ? d.x + k : 0];
          int at = 0;
          emit(in && contains(p.col + d.y, d.z, key, &at), d.w, L.v[own], key);
        }
        wave_sync();
      }
      if (end >= GM_WAVE) break;
      const int s_b = readlane(sb, end), s_n = readlane(sn, end), l_b = readlane(lb, end), l_n = readlane(ln, end);
      const int uu = readlane(u, end), vv = readlane(v, end);
      for (int t = 0; t < s_n; t += GM_WAVE) {
        const bool in = t + lane < s_n;
        const int key = p.col[s_b + (in ? t + lane : 0)];
        int at = 0;
        emit(in && contains(p.col + l_b, l_n, key, &at), uu, vv, key);
      }
      seg = end + 1;
    }

    if constexpr (FILL) {
      wave_sync();
      flush(qn);
      wave_sync();
    } else {
      const unsigned long long s = wave_sum_u64(cnt);
      if (lane == 0) p.off[b] = s;
    }
  }
}

static inline dim3 list_grid(long long nb, int cu_count) {
  return dim3((unsigned)std::max<long long>(1, std::min<long long>((nb + 3) / 4, (long long)cu_count * 8)));
}

// COUNT + scan: p.off[0 .. nb] = the first slot of every batch, p.off[nb] = T.  Synchronises the stream (the temporaries go back).
hipError_t list_count_scan(const ListParams &p, int cu_count, hipStream_t stream) {
  const long long nb = (p.ne + GM_WAVE - 1) >> 6;
  if (nb <= 0 || !p.off) return hipErrorInvalidValue;
  DevBuf<unsigned long long> cnt;
  ScanTemp tmp;
  hipError_t e = cnt.alloc((size_t)nb + 1);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(cnt.p + nb, 0, sizeof(unsigned long long), stream)) != hipSuccess) return e;
  ListParams q = p;
  q.off = cnt.p;
  hipLaunchKernelGGL(list_kernel<false>, list_grid(nb, cu_count), dim3(256), 0, stream, q);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = dev_exclusive_sum(tmp, cnt.p, p.off, (size_t)nb + 1, stream)) != hipSuccess) return e;
  return hipStreamSynchronize(stream);
}

hipError_t launch_list_fill(const ListParams &p, int cu_count, hipStream_t stream) {
  const long long nb = (p.ne + GM_WAVE - 1) >> 6;
  if (nb <= 0 || p.nw == 0) return hipSuccess;
  if (!p.off || !p.tri) return hipErrorInvalidValue;
  hipLaunchKernelGGL(list_kernel<true>, list_grid(nb, cu_count), dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace gm

// (module warm-up, gm_graph.hip finish_handle: HIP loads the code object of a translation unit when one of its kernels is first launched)
__global__ void gm_touch_list_kernel() {}
void gm_touch_list() { hipLaunchKernelGGL(gm_touch_list_kernel, dim3(1), dim3(1), 0, 0); }
