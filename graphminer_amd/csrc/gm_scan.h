// gm_scan.h -- the hipCUB (rocPRIM) scans, sorts, sums and selections of the untimed setup, each behind the size query / reserve / run protocol
// over a growable ScanTemp; included by the units that run them (gm_graph.hip, gm_tables.hip, gm_tasks.hip, gm_clique_plan.hip).
#pragma once
#include "gm_host.h"

#include <hipcub/hipcub.hpp>

// the grid of a setup kernel with one thread per item
inline dim3 grid_1d(long long n) { return dim3((unsigned)std::max<long long>(1, (n + 255) / 256)); }

template <class TI, class TO>
static hipError_t dev_exclusive_sum(ScanTemp &tmp, const TI *d_in, TO *d_out, size_t n, hipStream_t stream = 0) {
  size_t bytes = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_in, d_out, (int)n, stream);
  if (e != hipSuccess) return e;
  if ((e = tmp.reserve(bytes)) != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp.buf.p, bytes, d_in, d_out, (int)n, stream);
}
// "sizes, scan, total": the offsets of n items and, behind them, their sum -- d_in / d_out hold n + 1 elements, *total = d_out[n] on the host
template <class TI, class TO>
static hipError_t dev_scan_total(ScanTemp &tmp, const TI *d_in, TO *d_out, size_t n, TO *total) {
  const hipError_t e = dev_exclusive_sum(tmp, d_in, d_out, n + 1);
  return e != hipSuccess ? e : hipMemcpy(total, d_out + n, sizeof(TO), hipMemcpyDeviceToHost);
}

// stable radix sorts on the key bits [begin_bit, end_bit): (key, value) pairs, ascending or descending (a compile-time choice: only the
// direction a caller names is instantiated) ...
template <bool Descending, class K, class V>
static hipError_t dev_sort_pairs(ScanTemp &tmp, const K *k_in, K *k_out, const V *v_in, V *v_out, size_t n, int begin_bit = 0, int end_bit = 8 * (int)sizeof(K)) {
  size_t bytes = 0;
  auto run = [&](void *t) {
    if constexpr (Descending) return hipcub::DeviceRadixSort::SortPairsDescending(t, bytes, k_in, k_out, v_in, v_out, (int)n, begin_bit, end_bit);
    else return hipcub::DeviceRadixSort::SortPairs(t, bytes, k_in, k_out, v_in, v_out, (int)n, begin_bit, end_bit);
  };
  hipError_t e = run(nullptr);
  if (e != hipSuccess || (e = tmp.reserve(bytes)) != hipSuccess) return e;
  return run(tmp.buf.p);
}
// ... and keys alone, ascending
template <class K>
static hipError_t dev_sort_keys(ScanTemp &tmp, const K *k_in, K *k_out, size_t n, int begin_bit, int end_bit) {
  size_t bytes = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, k_in, k_out, (int)n, begin_bit, end_bit);
  if (e != hipSuccess || (e = tmp.reserve(bytes)) != hipSuccess) return e;
  return hipcub::DeviceRadixSort::SortKeys(tmp.buf.p, bytes, k_in, k_out, (int)n, begin_bit, end_bit);
}

// *total = the sum of n counters, on the host (a template so that only the units that sum carry the reduction's kernels)
template <class T>
static hipError_t dev_sum(ScanTemp &tmp, T *d_in, size_t n, T *total) {
  DevBuf<T> sum;
  size_t bytes = 0;
  hipError_t e = sum.alloc(1);
  if (e != hipSuccess || (e = hipcub::DeviceReduce::Sum(nullptr, bytes, d_in, sum.p, (int)n)) != hipSuccess) return e;
  if ((e = tmp.reserve(bytes)) != hipSuccess || (e = hipcub::DeviceReduce::Sum(tmp.buf.p, bytes, d_in, sum.p, (int)n)) != hipSuccess) return e;
  return hipMemcpy(total, sum.p, sizeof *total, hipMemcpyDeviceToHost);
}

// The vertices whose degree satisfies a predicate (a device functor of the degree), ascending: flag + iota, select, count to the host,
// degrees.  sel / degs are allocated here (degs only when there is a vertex to describe); *m = their number, 0 on an empty graph.
template <class Pred>
__global__ __launch_bounds__(256) void deg_flag_kernel(int nv, const int *__restrict__ rp, Pred pred, int *__restrict__ flag, int *__restrict__ iota) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  flag[v] = pred(rp[v + 1] - rp[v]) ? 1 : 0;
  iota[v] = v;
}
template <class Pred>
static int dev_select_by_degree(ScanTemp &tmp, int nv, const int *rp, Pred pred, DevBuf<int> &sel, DevBuf<int> &degs, int *m) {
  *m = 0;
  DevBuf<int> flag, iota, nsel;
  HIP_TRY(flag.alloc((size_t)nv));
  HIP_TRY(iota.alloc((size_t)nv));
  HIP_TRY(sel.alloc((size_t)nv));
  HIP_TRY(nsel.alloc(1));
  if (nv <= 0) return GM_OK;
  hipLaunchKernelGGL((deg_flag_kernel<Pred>), grid_1d(nv), dim3(256), 0, 0, nv, rp, pred, flag.p, iota.p);
  size_t bytes = 0;
  HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, bytes, iota.p, flag.p, sel.p, nsel.p, nv));
  HIP_TRY(tmp.reserve(bytes));
  HIP_TRY(hipcub::DeviceSelect::Flagged(tmp.buf.p, bytes, iota.p, flag.p, sel.p, nsel.p, nv));
  HIP_TRY(hipMemcpy(m, nsel.p, sizeof(int), hipMemcpyDeviceToHost));
  if (*m <= 0) return GM_OK;
  HIP_TRY(degs.alloc((size_t)*m));
  launch_gather_deg(*m, sel.p, rp, degs.p);
  return GM_OK;
}
