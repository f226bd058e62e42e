#!/usr/bin/env python
"""Measures the local k-clique counts (gm_clique_local) beside their comparator, CliqueSolver on the oriented copy of the same graph --
the count without the attribution -- and writes profiles/clique_local_kernel_ms.json (the table of DESIGN.md "Local k-clique counts";
GM_LIB_PATH selects another build of the library for an A/B run).  R-MAT scale 18 and 20, edge factor 16, k = 4 and 5; every figure is
gm_stats.kernel_ms, the median of the last three of five calls on one handle: CliqueSolver, then clique_local with both outputs, the
entries only, the vertices only.  Every run checks sum entries == k (k - 1) * CliqueSolver's count.  A (graph, k) step is a process of its
own under a time limit; the first step that fails or runs out of time ends the measurement, and what was not measured says so.

    python scripts/clique_local_bench.py [--scales 18 20] [--ks 4 5] [--step-seconds 300] [--out profiles/clique_local_kernel_ms.json]"""
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


def step(scale, edge_factor, k, seed=42):
    import numpy as np

    from graphminer_amd import CliqueSolver, clique_local
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    with sym.orient() as dag:
        cliques = CliqueSolver(dag, k)
        solver_ms = median_ms(lambda: CliqueSolver(dag, k, return_stats=True)[1].kernel_ms)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "k": k, "nv": sym.nv, "entries": sym.ne, "cliques": cliques, "clique_solver_ms": solver_ms}

    def call(**kw):
        total, kv, ent, st = clique_local(sym, k, return_stats=True, **kw)
        assert total == cliques, (total, cliques)
        if ent is not None:
            s = int(ent.sum(dtype=np.uint64))
            assert s == k * (k - 1) * cliques, (s, k, cliques)
        if kv is not None:
            assert int(kv.sum(dtype=np.uint64)) == k * cliques
        return st.kernel_ms

    row["both_ms"] = median_ms(lambda: call())
    row["entries_only_ms"] = median_ms(lambda: call(vertex=False))
    row["vertices_only_ms"] = median_ms(lambda: call(entries=False))
    row["local_over_solver"] = round(row["both_ms"] / solver_ms, 2)
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--ks", type=int, nargs="*", default=[4, 5])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clique_local_kernel_ms.json"))
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
    doc = {"_what": "gm_stats.kernel_ms, median of the last 3 of 5 calls on one handle (scripts/clique_local_bench.py); "
                    "local_over_solver = clique_local with both outputs / CliqueSolver on the oriented copy of the same graph",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
