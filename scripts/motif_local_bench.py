#!/usr/bin/env python
"""Measures the local motif counts (gm_motif_local) beside their inputs on the same handle and writes profiles/motif_local_kernel_ms.json
(the table of DESIGN.md "Local motif counts"; GM_LIB_PATH selects another build of the library for an A/B run).  R-MAT scale 18 and 20,
edge factor 16; every figure is gm_stats.kernel_ms, the median of the last three of five calls on one handle: tc_local,
rect_local(entries=False), clique_local(4, entries=False) and MotifSolver(4), the weighted triangle pass of the 5-vertex forms with and
without its walk (sgl6_raw "B" and "D": their difference is wtri_kernel, the same walk reading only), then motif_local at k = 4, k = 3 and
k = 4 without the orbit array.  Every motif_local call checks its counts against MotifSolver.  Derived: own_ms = k = 4 minus the three
input calls (the credit pass, its way back, the gathers and the finish), its share of the inputs' sum, and own_ms over the wtri walk.  A
graph is a process of its own under a time limit; the first step that fails or runs out of time ends the measurement, and what was not
measured says so.

    python scripts/motif_local_bench.py [--scales 18 20] [--step-seconds 300] [--out profiles/motif_local_kernel_ms.json]"""
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
    from graphminer_amd import MotifSolver, clique_local, motif_local, rect_local, sgl6_raw, tc_local
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    want = {3: MotifSolver(sym, 3), 4: MotifSolver(sym, 4)}
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "nv": sym.nv, "entries": sym.ne, "motif4": want[4]}
    row["tc_local_ms"] = median_ms(lambda: tc_local(sym, entries=False, return_stats=True)[3].kernel_ms)
    row["rect_local_ms"] = median_ms(lambda: rect_local(sym, entries=False, return_stats=True)[3].kernel_ms)
    row["clique_local4_ms"] = median_ms(lambda: clique_local(sym, 4, entries=False, return_stats=True)[3].kernel_ms)
    row["motif_solver4_ms"] = median_ms(lambda: MotifSolver(sym, 4, return_stats=True)[1].kernel_ms)
    row["wtri_pass_ms"] = median_ms(lambda: sgl6_raw(sym, ["B"], return_stats=True)[1].kernel_ms)
    row["wtri_pass_without_walk_ms"] = median_ms(lambda: sgl6_raw(sym, ["D"], return_stats=True)[1].kernel_ms)

    def call(k, **kw):
        counts, _orb, st = motif_local(sym, k, return_stats=True, **kw)
        assert counts == want[k], (k, counts, want[k])
        return st.kernel_ms

    row["k4_ms"] = median_ms(lambda: call(4))
    row["k3_ms"] = median_ms(lambda: call(3))
    row["k4_counts_only_ms"] = median_ms(lambda: call(4, orbits=False))
    inputs = row["tc_local_ms"] + row["rect_local_ms"] + row["clique_local4_ms"]
    row["inputs_sum_ms"] = round(inputs, 4)
    row["own_ms"] = round(row["k4_ms"] - inputs, 4)
    row["own_over_inputs"] = round(row["own_ms"] / inputs, 3)
    row["wtri_walk_ms"] = round(row["wtri_pass_ms"] - row["wtri_pass_without_walk_ms"], 4)
    row["own_over_wtri_walk"] = round(row["own_ms"] / row["wtri_walk_ms"], 2) if row["wtri_walk_ms"] > 0 else None
    row["k4_over_motif_solver4"] = round(row["k4_ms"] / row["motif_solver4_ms"], 2)
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motif_local_kernel_ms.json"))
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
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls on one handle (scripts/motif_local_bench.py); own_ms = k4_ms minus the "
                    "three input calls (tc_local, rect_local, clique_local(4), vertices only) = the credit pass, its way back, the gathers and "
                    "the finish; wtri_walk_ms = sgl6_raw B minus D, the weighted pass's walk over the same triangles, reading only",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
