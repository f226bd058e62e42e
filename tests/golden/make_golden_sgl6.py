#!/usr/bin/env python3
"""Generate tests/golden/sgl6.json: the two 6-vertex patterns of the reference's sgl solver, 6path and dumbbell (src/sgl/omp_base.cc:46-50),
from the REAL binary oracle/_ref/sgl_omp_base (built by oracle/ref/Makefile where the reference lies).

    python tests/golden/make_golden_sgl6.py [--limit SECONDS]

Graphs: those of sgl5.json -- the two data fixtures and the seeded R-MAT graphs of golden.json.  The reference's loop nests count one tuple
at a time.  citeseer, cora, rmat6_ef4_s1 and rmat8_ef8_s42 are never left out, for both patterns; an entry of the three larger R-MAT
graphs is only kept when the binary finishes within the limit (default 600 s, 8 threads), the entries left out are listed under
"_omitted", and a graph none of whose entries finished gets no record.  The file is rewritten after every graph.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from graphminer_amd.rmat import rmat_csr_numpy  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
PATTERNS = ("6path", "dumbbell")
RMATS = [(6, 4, 1, False), (8, 8, 42, False), (10, 16, 42, True), (12, 8, 7, True), (14, 16, 42, True)]  # (.., may be left out)


def count(prefix, pat, limit):
    env = dict(os.environ, OMP_NUM_THREADS="8")
    try:
        out = subprocess.run([os.path.join(REF, "sgl_omp_base"), prefix, pat], check=True, capture_output=True, text=True, env=env,
                             timeout=limit).stdout
    except subprocess.TimeoutExpired:
        return None
    m = re.findall(r"total_num = (\d+)", out)
    assert m, out
    return int(m[-1])


def main():
    limit = float(sys.argv[sys.argv.index("--limit") + 1]) if "--limit" in sys.argv else 600.0
    path = os.path.join(ROOT, "tests", "golden", "sgl6.json")
    gold = {"_limit_seconds": limit, "_omitted": []}

    def graph(name, prefix, meta, optional):
        r = dict(meta)
        for pat in PATTERNS:
            c = count(prefix, pat, limit if optional else None)
            if c is None:
                gold["_omitted"].append(f"{name}:{pat}")
            else:
                r[pat] = c
            print(name, pat, c, flush=True)
        if any(pat in r for pat in PATTERNS):  # (a graph none of whose entries finished is left out as a whole)
            gold[name] = r
        with open(path, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")

    for name in ("citeseer", "cora"):
        graph(name, os.path.join(ROOT, "tests", "fixtures", name, "graph"), {"kind": "fixture"}, False)
    with tempfile.TemporaryDirectory() as td:
        for scale, ef, seed, optional in RMATS:
            g = rmat_csr_numpy(scale, ef, seed)
            d = os.path.join(td, g.name)
            os.makedirs(d)
            g.save(os.path.join(d, "graph"))
            graph(g.name, os.path.join(d, "graph"), {"kind": "rmat", "scale": scale, "edge_factor": ef, "seed": seed}, optional)


if __name__ == "__main__":
    main()
