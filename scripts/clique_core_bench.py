#!/usr/bin/env python
"""Measures the k-clique core decomposition (gm_clique_core_decompose) on the graphs scripts/clique_local_bench.py uses and writes
profiles/clique_core_kernel_ms.json (the table of DESIGN.md "k-clique cores").  R-MAT scale 18 and 20, edge factor 16, k = 2, 3, 4.
  total_ms          gm_stats.kernel_ms of the decomposition on one handle, the median of the last two of three calls: the initial count, every
                    mark and peel kernel, the host's read-back per round
  the split         ONE further decomposition in a process of its own under `rocprofv3 --kernel-trace`: the kernels' own durations summed
                    by name -- initial_count_kernel_ms (gm_clique_local's kernels), mark_kernel_ms (core_mark_kernel), peel_kernel_ms
                    (core_peel*_kernel), other_kernel_ms (core_init_kernel, core_out_kernel) -- and between_kernels_ms = total_ms minus
                    their sum: the read-backs, the memsets and the launch gaps of the rounds.  Tracing slows the host, so the traced run
                    gives the kernels' durations only; total_ms comes from the runs without it.
Every run checks c_max against the core numbers and the densest state against the rounds.  A (graph, k) step is a process of its own under
a time limit; the first step that fails or runs out of time ends the measurement, and what was not measured says so.

    python scripts/clique_core_bench.py [--scales 18 20] [--ks 2 3 4] [--step-seconds 300] [--out profiles/clique_core_kernel_ms.json]"""
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
    from graphminer_amd import clique_core_decompose
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    row = {"graph": f"rmat{scale}_ef{edge_factor}_s{seed}", "k": k, "nv": sym.nv, "entries": sym.ne}

    def decompose():
        core, rnd, c_max, rounds, dense, st = clique_core_decompose(sym, k, return_stats=True)
        assert c_max == int(core.max()) and int(rnd.max()) == rounds - 1, (c_max, rounds)
        assert dense[1] == int((rnd >= dense[0]).sum()), dense
        row.update(c_max=c_max, rounds=rounds, dense_round=dense[0], dense_vertices=dense[1], dense_cliques=dense[2])
        return st.kernel_ms

    row["total_ms"] = median_ms(decompose)
    row["ms_per_round"] = round(row["total_ms"] / row["rounds"], 4)
    sym.free()
    return row


def traced(scale, edge_factor, k, seed=42):
    """what the traced process runs: the graph and one decomposition"""
    from graphminer_amd import clique_core_decompose
    from graphminer_amd.rmat import rmat_csr_device

    sym, _rp, _col = rmat_csr_device(scale, edge_factor, seed)
    rounds = clique_core_decompose(sym, k)[3]
    sym.free()
    print(f"TRACED rounds {rounds}", flush=True)


SPLIT = (("peel_kernel_ms", ("core_peel",)), ("mark_kernel_ms", ("core_mark_kernel",)), ("other_kernel_ms", ("core_init_kernel", "core_out_kernel")),
         ("initial_count_kernel_ms", ("kcl_local_", "local_map_kernel", "local_vertex_kernel")))


def kernel_split(scale, edge_factor, k, seconds):
    """the kernels' durations of one traced decomposition by name, in ms"""
    import csv
    import glob
    import shutil
    import tempfile

    out = tempfile.mkdtemp(prefix="core_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--edge-factor", str(edge_factor), "--traced-step", str(scale), str(k)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            raise RuntimeError(f"exit {r.returncode}, {len(files)} trace files: {(r.stdout + r.stderr)[-300:]}")
        ns = {key: 0 for key, _ in SPLIT}
        calls = {key: 0 for key, _ in SPLIT}
        for path in files:
            with open(path, newline="") as f:
                for rec in csv.DictReader(f):
                    for key, names in SPLIT:
                        if any(n in rec["Kernel_Name"] for n in names):
                            ns[key] += int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])
                            calls[key] += 1
                            break
        res = {key: round(v / 1e6, 4) for key, v in ns.items()}
        res["mark_kernel_launches"] = calls["mark_kernel_ms"]
        res["peel_kernel_launches"] = calls["peel_kernel_ms"]
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--ks", type=int, nargs="*", default=[2, 3, 4])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--step-seconds", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clique_core_kernel_ms.json"))
    ap.add_argument("--step", type=int, nargs=2, metavar=("SCALE", "K"), help="run one step in this process and print its row")
    ap.add_argument("--traced-step", type=int, nargs=2, metavar=("SCALE", "K"), help="what runs under the kernel trace: one decomposition")
    a = ap.parse_args()
    if a.traced_step:
        traced(a.traced_step[0], a.edge_factor, a.traced_step[1])
        return 0
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
                row = json.loads(line[-1][4:])
                try:
                    row.update(kernel_split(sc, a.edge_factor, k, a.step_seconds))
                    row["between_kernels_ms"] = round(row["total_ms"] - sum(row[key] for key, _ in SPLIT), 4)
                except (OSError, KeyError, ValueError) as e:  # (no rocprofv3 here, or a trace this script cannot read)
                    row["split_not_measured"] = f"{type(e).__name__}: {str(e)[:200]}"
                except (subprocess.TimeoutExpired, RuntimeError) as e:  # (the traced process failed: nothing more is started)
                    row["split_not_measured"] = f"{type(e).__name__}: {str(e)[:200]}"
                    stopped = f"{label}, traced ({type(e).__name__})"
                rows.append(row)
            except (subprocess.TimeoutExpired, RuntimeError) as e:
                stopped = f"{label} ({type(e).__name__})"
                rows.append({"graph": f"rmat{sc}_ef{a.edge_factor}_s42", "k": k, "not_measured": str(e)[:300]})
            print(json.dumps(rows[-1]), flush=True)
    doc = {"_what": "total_ms = gm_stats.kernel_ms of gm_clique_core_decompose, median of the last 2 of 3 calls on one handle "
                    "(scripts/clique_core_bench.py); *_kernel_ms = the kernels' own durations of one further decomposition under rocprofv3 "
                    "--kernel-trace, summed by kernel name; between_kernels_ms = total_ms minus their sum (read-backs, memsets, launch gaps). "
                    "First measurement: no earlier figure exists",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
