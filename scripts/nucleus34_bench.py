#!/usr/bin/env python
"""Measures the triangle nuclei (gm_tri_clique4_local / gm_nucleus34_decompose) on the graphs scripts/clique_truss_bench.py uses and writes
profiles/nucleus34_kernel_ms.json (the table of DESIGN.md "Triangle nuclei").  R-MAT scale 18 and 20, edge factor 16.
  index_ms             the triangle index, built by the first call on a fresh handle: gm_stats.kernel_ms of that first gm_tri_clique4_local
                       minus count_ms
  count_ms             gm_stats.kernel_ms of gm_tri_clique4_local with the index in place, the median of the last two of three further calls
  total_ms             gm_stats.kernel_ms of gm_nucleus34_decompose on the same handle, the median of the last two of three calls: the
                       initial count, every mark and peel kernel, the host's read-back per round
  ms_per_round         (total_ms - count_ms) / rounds
  clique_truss_ms      context, not a bound: gm_clique_truss_decompose(k = 4) on the same handle, measured the same way -- the same
                       4-cliques peeled by edge
Every run checks c_max against theta and the rounds against the per-triangle rounds.  A graph is a process of its own under a time limit; the
first step that fails or runs out of time ends the measurement, and what was not measured says so.  No time is asserted.

    python scripts/nucleus34_bench.py [--scales 18 20] [--step-seconds 300] [--out profiles/nucleus34_kernel_ms.json]"""
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


def step(scale, edge_factor, seed=42):
    from graphminer_amd import clique_truss_decompose, nucleus34_decompose, tri_clique4_local
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "nv": sym.nv, "entries": sym.ne}

    def local():
        total, k4, st = tri_clique4_local(sym, return_stats=True)
        assert int(k4.sum(dtype="uint64")) == 4 * total
        row.update(triangles=int(k4.shape[0]), cliques4=total)
        return st.kernel_ms

    first = local()  # (builds the index)
    row["count_ms"] = median_ms(local)
    row["index_ms"] = round(first - row["count_ms"], 4)

    def decompose():
        theta, rnd, c_max, rounds, st = nucleus34_decompose(sym, return_stats=True)
        assert c_max == int(theta.max()) and int(rnd.max()) == rounds - 1, (c_max, rounds)
        row.update(c_max=c_max, rounds=rounds)
        return st.kernel_ms

    row["total_ms"] = median_ms(decompose)
    row["ms_per_round"] = round((row["total_ms"] - row["count_ms"]) / row["rounds"], 4)

    def by_edge():
        theta, rnd, c_max, rounds, st = clique_truss_decompose(sym, 4, return_stats=True)
        row.update(clique_truss_c_max=c_max, clique_truss_rounds=rounds)
        return st.kernel_ms

    row["clique_truss_ms"] = median_ms(by_edge)
    sym.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nucleus34_kernel_ms.json"))
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
        except subprocess.TimeoutExpired:
            stopped = f"{label} (time limit)"
            rows.append({"graph": f"{label}_s42", "not_measured": f"the step did not finish within its time limit of {a.step_seconds} s"})
        except RuntimeError as e:
            stopped = f"{label} (failed)"
            rows.append({"graph": f"{label}_s42", "not_measured": str(e)[:300]})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "gm_stats.kernel_ms, medians of the last 2 of 3 calls on one handle (scripts/nucleus34_bench.py): count_ms = "
                    "gm_tri_clique4_local with the index in place, index_ms = the first call on the fresh handle minus count_ms, total_ms = "
                    "gm_nucleus34_decompose, ms_per_round = (total_ms - count_ms) / rounds, clique_truss_ms = gm_clique_truss_decompose(k = 4) "
                    "on the same handle as context.  First measurement: no earlier figure exists",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
