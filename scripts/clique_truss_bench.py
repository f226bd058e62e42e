#!/usr/bin/env python
"""Measures the k-clique truss decomposition (gm_clique_truss_decompose) on the graphs scripts/clique_core_bench.py uses and writes
profiles/clique_truss_kernel_ms.json (the table of DESIGN.md "k-clique trusses").  R-MAT scale 18 and 20, edge factor 16, k = 3, 4.
  total_ms             gm_stats.kernel_ms of the decomposition on one handle, the median of the last two of three calls: the initial count,
                       every mark and peel kernel, the host's read-back per round
  truss_decompose_ms   k = 3 only, the comparator: gm_truss_decompose on the same handle, measured the same way -- the same trussness
                       (theta + 2) by the triangle peel over 32-bit supports
Every run checks c_max against theta, and at k = 3 theta + 2 against the comparator's trussness.  A (graph, k) step is a process of its own
under a time limit; the first step that fails or runs out of time ends the measurement, and what was not measured says so.  No time is
asserted.

    python scripts/clique_truss_bench.py [--scales 18 20] [--ks 3 4] [--step-seconds 300] [--out profiles/clique_truss_kernel_ms.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, KEEP = 3, 2


def median_ms(call):
    """call() -> kernel_ms; the median of the last KEEP of CALLS calls"""
    return round(statistics.median([call() for _ in range(CALLS)][-KEEP:]), 4)


def step(scale, edge_factor, k, seed=42):
    import numpy as np

    from graphminer_amd import clique_truss_decompose, truss_decompose
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "k": k, "nv": sym.nv, "entries": sym.ne}
    kept = {}

    def decompose():
        theta, rnd, c_max, rounds, st = clique_truss_decompose(sym, k, return_stats=True)
        assert c_max == int(theta.max()) and int(rnd.max()) == rounds - 1, (c_max, rounds)
        row.update(c_max=c_max, rounds=rounds)
        kept["theta"] = theta
        return st.kernel_ms

    row["total_ms"] = median_ms(decompose)
    row["ms_per_round"] = round(row["total_ms"] / row["rounds"], 4)
    if k == 3:
        def triangles():
            tau, k_max, rounds, st = truss_decompose(sym, return_stats=True)
            assert np.array_equal(kept["theta"] + np.uint64(2), tau.astype(np.uint64)), "theta + 2 is the trussness"
            row.update(truss_decompose_k_max=k_max, truss_decompose_rounds=rounds)
            return st.kernel_ms

        row["truss_decompose_ms"] = median_ms(triangles)
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--ks", type=int, nargs="*", default=[3, 4])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clique_truss_kernel_ms.json"))
    ap.add_argument("--step", type=int, nargs=2, metavar=("SCALE", "K"), help="run one step in this process and print its row")
    a = ap.parse_args()
    if a.step:
        print("ROW " + json.dumps(step(a.step[0], a.edge_factor, a.step[1])), flush=True)
        return 0
    rows, stopped = [], None
    for sc in a.scales:
        for k in a.ks:
            label = f"rmat{sc}_ef{a.edge_factor} k={k}"
            if stopped:
                rows.append({"graph": f"rmat{sc}_ef{a.edge_factor}_s42", "k": k, "not_measured": f"after {stopped}"})
                continue
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--edge-factor", str(a.edge_factor), "--step", str(sc), str(k)],
                                   capture_output=True, text=True, timeout=a.step_seconds)
                line = [x for x in r.stdout.splitlines() if x.startswith("ROW ")]
                if r.returncode != 0 or not line:
                    raise RuntimeError(f"exit {r.returncode}: {(r.stdout + r.stderr)[-400:]}")
                rows.append(json.loads(line[-1][4:]))
            except (subprocess.TimeoutExpired, RuntimeError) as e:
                stopped = f"{label} ({type(e).__name__})"
                rows.append({"graph": f"rmat{sc}_ef{a.edge_factor}_s42", "k": k, "not_measured": str(e)[:300]})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "total_ms = gm_stats.kernel_ms of gm_clique_truss_decompose, median of the last 2 of 3 calls on one handle "
                    "(scripts/clique_truss_bench.py); truss_decompose_ms (k = 3) = gm_truss_decompose on the same handle, measured the same "
                    "way.  First measurement: no earlier figure exists",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
