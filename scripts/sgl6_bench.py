#!/usr/bin/env python
"""Measures the two 6-vertex closed forms (gm_sgl6_raw / gm_sgl6) beside their comparators and writes profiles/sgl6_kernel_ms.json (the table
of DESIGN.md "SgL, 6-vertex closed forms").  R-MAT scale 18 and 20, edge factor 16; every figure is gm_stats.kernel_ms, the median of the
last three of five calls on one handle.  The comparator of the degree-weighted 4-cycle kernel (sgl6_raw(Z | R)) is the rectangle path on the
same handle: the same pruned walk with one counter per 2-path end instead of two.  Each graph's run is checked: the R of the new kernel must
equal the rectangle count.  A graph whose first 6path call takes a minute or more is reported and left out.

    python scripts/sgl6_bench.py [--scales 18 20] [--out profiles/sgl6_kernel_ms.json]"""
import argparse
import json
import os
import statistics
import sys
import time

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
    from graphminer_amd import SGL6_RAW, SglSolver, sgl6, sgl6_raw
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "nv": sym.nv, "entries": sym.ne}
    t = time.perf_counter()
    first = sgl6(sym, "6path")
    row["first_6path_call_s"] = round(time.perf_counter() - t, 2)
    if row["first_6path_call_s"] >= 60.0:
        row["left_out"] = "a call takes a minute or more"
        sym.free()
        return row
    row["rectangle_ms"], rect = median_ms(lambda: SglSolver(sym, "rectangle", return_stats=True))
    row["pentagon_ms"], row["pentagon"] = median_ms(lambda: SglSolver(sym, "pentagon", return_stats=True))
    row["sgl6_raw_ZR_ms"], raw = median_ms(lambda: sgl6_raw(sym, ("Z", "R"), return_stats=True))
    raw = dict(zip(SGL6_RAW, raw))
    assert raw["R"] == rect, (raw["R"], rect)
    row["rectangle"], row["Z"] = rect, raw["Z"]
    row["Z_kernel_over_rectangle"] = round(row["sgl6_raw_ZR_ms"] / row["rectangle_ms"], 3)
    row["6path_ms"], row["6path"] = median_ms(lambda: sgl6(sym, "6path", return_stats=True))
    assert row["6path"] == first
    row["dumbbell_ms"], row["dumbbell"] = median_ms(lambda: sgl6(sym, "dumbbell", return_stats=True))
    row["pentagon_share_of_6path"] = round(row["pentagon_ms"] / row["6path_ms"], 3)
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgl6_kernel_ms.json"))
    a = ap.parse_args()
    rows = []
    for sc in a.scales:
        rows.append(run(sc, a.edge_factor))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls on one handle (scripts/sgl6_bench.py)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
