#!/usr/bin/env python
"""Measures the local counts and the k-truss (gm_tc_local / gm_ktruss / gm_truss_decompose) beside their comparator, the one-GPU diamond --
the same pass over the triangles of the oriented copy -- and writes profiles/local_kernel_ms.json (the table of DESIGN.md "Local counts and
k-truss"; GM_LIB_PATH selects another build of the library for an A/B run).  R-MAT scale 18 and 20, edge factor 16; every figure is gm_stats.kernel_ms, the median of the last three of five calls on one
handle.  Each graph's run is checked: the sum of the supports / 6 must equal TCSolver's total.

    python scripts/local_bench.py [--scales 18 20] [--out profiles/local_kernel_ms.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, KEEP = 5, 3


def median_ms(call):
    """call() -> (result, Stats); the median kernel_ms of the last KEEP of CALLS calls and the last result"""
    ms, res = [], None
    for _ in range(CALLS):
        res, st = call()
        ms.append(st.kernel_ms)
    return round(statistics.median(ms[-KEEP:]), 4), res


def run(scale, edge_factor, seed=42):
    import numpy as np

    from graphminer_amd import SglSolver, TCSolver, ktruss, tc_local, truss_decompose
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    with sym.orient() as dag:
        triangles = TCSolver(dag)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "nv": sym.nv, "entries": sym.ne, "triangles": triangles}
    row["diamond_ms"], _ = median_ms(lambda: SglSolver(sym, "diamond", return_stats=True))

    def local(**kw):
        r = tc_local(sym, return_stats=True, **kw)
        return r[:3], r[3]

    row["tc_local_ms"], (total, tv, sup) = median_ms(lambda: local())
    s = int(sup.astype(np.uint64).sum())
    assert s % 6 == 0 and s // 6 == triangles == total and int(tv.sum()) == 3 * triangles, (s, total, triangles)
    row["tc_local_supports_ms"], _ = median_ms(lambda: local(vertex=False))
    row["tc_local_vertices_ms"], _ = median_ms(lambda: local(entries=False))
    row["tc_local_over_diamond"] = round(row["tc_local_ms"] / row["diamond_ms"], 3)
    # what the way back costs: the supports-only call minus the support pass it starts with, timed alone on the same handle (the diamond is
    # not that pass: it has the match masks and its own sum C(t, 2)), per directed entry; the vertex sums are the rest of the full call
    import torch

    from graphminer_amd.solvers import diamond_support_partial, diamond_support_size

    n = diamond_support_size(sym, 1)
    buf = torch.empty(n, dtype=torch.int32, device="cuda:0")
    row["support_pass_ms"], _ = median_ms(lambda: (None, diamond_support_partial(sym, buf.data_ptr(), n, return_stats=True)))
    row["mapping_ms"] = round(row["tc_local_supports_ms"] - row["support_pass_ms"], 4)
    row["mapping_ns_per_entry"] = round(row["mapping_ms"] * 1e6 / max(sym.ne, 1), 4)
    row["vertex_sums_ms"] = round(row["tc_local_ms"] - row["tc_local_supports_ms"], 4)

    def truss(k):
        r = ktruss(sym, k, return_stats=True)
        return (r[0], r[2]), r[3]

    def decompose():
        r = truss_decompose(sym, return_stats=True)
        return (r[1], r[2]), r[3]

    row["truss_decompose_ms"], (k_max, rounds) = median_ms(decompose)
    row["k_max"], row["truss_decompose_rounds"] = k_max, rounds
    row["ktruss4_ms"], (row["ktruss4_edges"], row["ktruss4_rounds"]) = median_ms(lambda: truss(4))
    row["ktruss_kmax_ms"], (row["ktruss_kmax_edges"], row["ktruss_kmax_rounds"]) = median_ms(lambda: truss(k_max))
    assert row["ktruss_kmax_edges"] > 0 and ktruss(sym, k_max + 1)[0] == 0
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_kernel_ms.json"))
    a = ap.parse_args()
    rows = []
    for sc in a.scales:
        rows.append(run(sc, a.edge_factor))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls on one handle (scripts/local_bench.py)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
