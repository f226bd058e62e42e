#!/usr/bin/env python
"""Measures the local 4-cycle counts (gm_rect_local) beside their two comparators on the same handle -- SglSolver("rectangle"), the count
alone, and sgl6_raw("Z"), the same pruned walk made once -- and writes profiles/rect_local_kernel_ms.json (the table of DESIGN.md "Local
4-cycle counts"; GM_LIB_PATH selects another build of the library for an A/B run).  R-MAT scale 18 and 20, edge factor 16; every figure is
gm_stats.kernel_ms, the median of the last three of five calls on one handle: the two comparators, then rect_local with both outputs, the
entries only, the vertices only.  Every run checks sum entries / 8 (sum R_v / 4) against the rectangle count.  A graph is a process of its
own under a time limit; the first step that fails or runs out of time ends the measurement, and what was not measured says so.

    python scripts/rect_local_bench.py [--scales 18 20] [--step-seconds 300] [--out profiles/rect_local_kernel_ms.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, KEEP = 5, 3


def median_ms(call):
    """call() -> kernel_ms; the median of the last KEEP of CALLS calls"""
    return round(statistics.median([call() for _ in range(CALLS)][-KEEP:]), 4)


def step(scale, edge_factor, seed=42):
    import numpy as np

    from graphminer_amd import SglSolver, rect_local, sgl6_raw
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    rectangles = SglSolver(sym, "rectangle")
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "nv": sym.nv, "entries": sym.ne, "rectangles": rectangles}
    row["rectangle_solver_ms"] = median_ms(lambda: SglSolver(sym, "rectangle", return_stats=True)[1].kernel_ms)
    row["sgl6_z_ms"] = median_ms(lambda: sgl6_raw(sym, ["Z"], return_stats=True)[1].kernel_ms)

    def call(**kw):
        total, rv, ent, st = rect_local(sym, return_stats=True, **kw)
        assert total == rectangles, (total, rectangles)
        if ent is not None:
            s = int(ent.sum(dtype=np.uint64))
            assert s == (8 * rectangles) % 2 ** 64, (s, rectangles)
        if rv is not None:
            assert int(rv.sum(dtype=np.uint64)) == (4 * rectangles) % 2 ** 64
        return st.kernel_ms

    row["both_ms"] = median_ms(lambda: call())
    row["entries_only_ms"] = median_ms(lambda: call(vertex=False))
    row["vertices_only_ms"] = median_ms(lambda: call(entries=False))
    row["local_over_rectangle_solver"] = round(row["both_ms"] / row["rectangle_solver_ms"], 2)
    row["local_over_sgl6_z"] = round(row["both_ms"] / row["sgl6_z_ms"], 2)
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rect_local_kernel_ms.json"))
    ap.add_argument("--step", type=int, metavar="SCALE", help="run one step in this process and print its row")
    a = ap.parse_args()
    if a.step is not None:
        print("ROW " + json.dumps(step(a.step, a.edge_factor)), flush=True)
        return 0
    rows, stopped = [], None
    for sc in a.scales:
        label = f"rmat{sc}_ef{a.edge_factor}"
        if stopped:
            rows.append({"graph": f"{label}_s42", "not_measured": f"after {stopped}"})
            continue
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--edge-factor", str(a.edge_factor), "--step", str(sc)],
                               capture_output=True, text=True, timeout=a.step_seconds)
            line = [x for x in r.stdout.splitlines() if x.startswith("ROW ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"exit {r.returncode}: {(r.stdout + r.stderr)[-400:]}")
            rows.append(json.loads(line[-1][4:]))
        except (subprocess.TimeoutExpired, RuntimeError) as e:
            stopped = f"{label} ({type(e).__name__})"
            rows.append({"graph": f"{label}_s42", "not_measured": str(e)[:300]})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls on one handle (scripts/rect_local_bench.py); the ratios are rect_local "
                    "with both outputs over SglSolver(\"rectangle\") and over sgl6_raw(\"Z\") (the same pruned walk, one pass) on that handle",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
