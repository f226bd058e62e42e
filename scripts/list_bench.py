#!/usr/bin/env python
"""Measures the triangle listing (gm_tc_list) beside its comparator, TCSolver on the oriented copy -- the same lookups without the writing --
and the stream ceiling of the box, and writes profiles/list_kernel_ms.json (the table of DESIGN.md "Triangle listing"; GM_LIB_PATH selects
another build of the library for an A/B run).  R-MAT scale 18 and 20, edge factor 16; every figure is gm_stats.kernel_ms, the median of the
last three of five calls: the count-only call on five fresh handles of the same arrays (count + scan), then on one handle the full list
(a fill after the cached count) and a window of 2^20 triangles in the middle.  Each graph's total is checked against TCSolver's.

    python scripts/list_bench.py [--scales 18 20] [--out profiles/list_kernel_ms.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, KEEP = 5, 3
WINDOW = 1 << 20


def median_ms(call):
    """call() -> kernel_ms; the median of the last KEEP of CALLS calls"""
    return round(statistics.median([call() for _ in range(CALLS)][-KEEP:]), 4)


def stream_ceiling_gbs(torch, lib, _lib):
    """gm_stream_ceiling: 16 B per lane over 4 GiB, the best of three timed passes after a first one"""
    n = 1 << 30
    buf = torch.ones(n, dtype=torch.int32, device="cuda:0")
    out = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    best = 0.0
    for i in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.gm_stream_ceiling(buf.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream or None), "gm_stream_ceiling")
        e1.record()
        torch.cuda.synchronize()
        if i:
            best = max(best, 4.0 * n / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    del buf
    return round(best, 1)


def run(scale, edge_factor, ceiling_gbs, seed=42):
    import torch

    from graphminer_amd import DeviceGraph, TCSolver, _lib
    from graphminer_amd._lib import gm_stats
    from graphminer_amd.rmat import rmat_csr_device

    lib = _lib.load()
    sym, rp, col = rmat_csr_device(scale, edge_factor, seed)

    def call(h, first, cap, buf):
        st, total, written = gm_stats(), C.c_uint64(0), C.c_uint64(0)
        _lib.check(lib.gm_tc_list(h.handle, None, first, cap, buf.data_ptr() if buf is not None else None, C.byref(total), C.byref(written), C.byref(st)),
                   "gm_tc_list")
        return st.kernel_ms, int(total.value), int(written.value)

    with sym.orient() as dag:
        tc_ms = median_ms(lambda: TCSolver(dag, return_stats=True)[1].kernel_ms)
        triangles = TCSolver(dag)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "nv": sym.nv, "entries": sym.ne, "triangles": triangles, "tc_ms": tc_ms}

    def fresh_count():
        with DeviceGraph.from_device_ptrs(sym.nv, sym.ne, rp.data_ptr(), col.data_ptr(), 0, keepalive=(rp, col)) as h:
            ms, total, _ = call(h, 0, 0, None)
            assert total == triangles, (total, triangles)
            return ms

    row["count_scan_ms"] = median_ms(fresh_count)
    buf = torch.empty(3 * triangles, dtype=torch.int32, device="cuda:0")
    assert call(sym, 0, triangles, buf)[1:] == (triangles, triangles)
    row["fill_ms"] = median_ms(lambda: call(sym, 0, triangles, buf)[0])
    win = min(WINDOW, triangles)
    mid = (triangles - win) // 2
    assert call(sym, mid, win, buf)[1:] == (triangles, win)
    row["window_triangles"] = win
    row["window_ms"] = median_ms(lambda: call(sym, mid, win, buf)[0])
    row["fill_over_tc"] = round(row["fill_ms"] / tc_ms, 3)
    row["output_gbs"] = round(12.0 * triangles / (row["fill_ms"] * 1e-3) / 1e9, 1)
    row["output_share_of_ceiling"] = round(row["output_gbs"] / ceiling_gbs, 4)
    del buf
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_kernel_ms.json"))
    a = ap.parse_args()
    import torch

    from graphminer_amd import _lib

    ceiling = stream_ceiling_gbs(torch, _lib.load(), _lib)
    rows = []
    for sc in a.scales:
        rows.append(run(sc, a.edge_factor, ceiling))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls (scripts/list_bench.py); output_gbs = 12 T / fill time",
           "stream_ceiling_gbs": ceiling, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
