#!/usr/bin/env python
"""Measures the k-clique listing (gm_clique_list) beside its two comparators -- CliqueSolver on the oriented copy of the same graph (the
count without the rows) and the time its output would take at the stream ceiling of the box (4 k T bytes over gm_stream_ceiling) -- and
writes profiles/clique_list_kernel_ms.json (the table of DESIGN.md "k-clique listing"; GM_LIB_PATH selects another build of the library
for an A/B run).  R-MAT scale 18 and 20, edge factor 16, k = 4 and k = 5; every figure is gm_stats.kernel_ms, the median of the last three
of five calls: the count-only call on five fresh handles of the same arrays (count + scan), then on one handle the full list where 4 k T
bytes fit the budget (a fill after the cached count) and a window of 2^20 rows in the middle.  Every total is checked against CliqueSolver.

    python scripts/clique_list_bench.py [--scales 18 20] [--ks 4 5] [--out profiles/clique_list_kernel_ms.json]"""
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
FULL_LIST_BYTES = 64 << 30  # a full list is filled when its 4 k T bytes stay below this


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


def run(scale, edge_factor, ks, ceiling_gbs, done, seed=42):
    import torch

    from graphminer_amd import CliqueSolver, DeviceGraph, _lib
    from graphminer_amd._lib import gm_stats
    from graphminer_amd.rmat import rmat_csr_device

    lib = _lib.load()
    sym, rp, col = rmat_csr_device(scale, edge_factor, seed)
    rows = []

    def call(h, k, first, cap, buf):
        st, total, written = gm_stats(), C.c_uint64(0), C.c_uint64(0)
        _lib.check(lib.gm_clique_list(h.handle, k, None, first, cap, buf.data_ptr() if buf is not None else None, C.byref(total), C.byref(written),
                                      C.byref(st)), "gm_clique_list")
        return st.kernel_ms, int(total.value), int(written.value)

    for k in ks:
        with sym.orient() as dag:
            solver_ms = median_ms(lambda: CliqueSolver(dag, k, return_stats=True)[1].kernel_ms)
            cliques = CliqueSolver(dag, k)
        row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "k": k, "nv": sym.nv, "entries": sym.ne, "cliques": cliques, "clique_solver_ms": solver_ms}

        def fresh_count():
            with DeviceGraph.from_device_ptrs(sym.nv, sym.ne, rp.data_ptr(), col.data_ptr(), 0, keepalive=(rp, col)) as h:
                ms, total, _ = call(h, k, 0, 0, None)
                assert total == cliques, (total, cliques)
                return ms

        row["count_scan_ms"] = median_ms(fresh_count)
        assert call(sym, k, 0, 0, None)[1] == cliques
        list_bytes = 4 * k * cliques
        row["list_bytes"] = list_bytes
        row["ceiling_ms"] = round(list_bytes / (ceiling_gbs * 1e9) * 1e3, 4)
        win = min(WINDOW, cliques)
        mid = (cliques - win) // 2
        if list_bytes <= FULL_LIST_BYTES:
            buf = torch.empty(k * cliques, dtype=torch.int32, device="cuda:0")
            assert call(sym, k, 0, cliques, buf)[1:] == (cliques, cliques)
            row["fill_ms"] = median_ms(lambda: call(sym, k, 0, cliques, buf)[0])
            row["fill_over_solver"] = round(row["fill_ms"] / solver_ms, 3)
            row["output_gbs"] = round(list_bytes / (row["fill_ms"] * 1e-3) / 1e9, 1)
            row["output_share_of_ceiling"] = round(row["output_gbs"] / ceiling_gbs, 4)
        else:
            buf = torch.empty(k * win, dtype=torch.int32, device="cuda:0")
            row["fill_ms"] = None
        assert call(sym, k, mid, win, buf)[1:] == (cliques, win)
        row["window_rows"] = win
        row["window_ms"] = median_ms(lambda: call(sym, k, mid, win, buf)[0])
        del buf
        rows.append(row)
        done(row)
    sym.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--ks", type=int, nargs="*", default=[4, 5])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clique_list_kernel_ms.json"))
    a = ap.parse_args()
    import torch

    from graphminer_amd import _lib

    ceiling = stream_ceiling_gbs(torch, _lib.load(), _lib)
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls (scripts/clique_list_bench.py); output_gbs = 4 k T / fill time; "
                    "ceiling_ms = 4 k T bytes at stream_ceiling_gbs; fill_ms null: the full list was not filled (see FULL_LIST_BYTES)",
           "stream_ceiling_gbs": ceiling, "rows": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def done(row):  # (the file is rewritten after every row: a long run that is cut short keeps what it measured)
        print(json.dumps(row), flush=True)
        doc["rows"].append(row)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    for sc in a.scales:
        run(sc, a.edge_factor, a.ks, ceiling, done)


if __name__ == "__main__":
    main()
