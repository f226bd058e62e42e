"""Differential test: CPU oracle vs the REAL reference binaries on freshly seeded graphs. The reference's answers on these graphs are
recorded in tests/golden/oracle_vs_ref.json (tests/golden/make_golden.py --vs-ref, from oracle/_ref as oracle/ref/Makefile builds it
from the reference's sources); wherever those binaries are built they are run as well and must still print the recorded answers."""
import json
import os
import re

import pytest

import oracle as O
from common import ROOT, csr_sha, random_graph
from graphminer_amd.rmat import rmat_csr_numpy

CASES = [("rmat", 9, 8, 3), ("rmat", 11, 6, 11), ("rand", 500, 4000, 5), ("rand", 3000, 9000, 6)]


def gold(key):
    with open(os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.json")) as f:
        return json.load(f)[key]


def _last_int(lines, pat):
    for ln in reversed(lines):
        m = re.search(pat, ln)
        if m:
            return int(m.group(1))
    raise AssertionError(lines)


def case_graph(case):
    return rmat_csr_numpy(case[1], case[2], case[3]) if case[0] == "rmat" else random_graph(case[1], case[2], case[3])


def case_key(case):
    return "_".join(map(str, case))


def ref_answers(prefix):
    """what the reference binaries print for the graph at `prefix` (tc, diamond, rectangle, 4- / 5-cliques, 3-motif)"""
    out = {"tc": _last_int(O.run_ref("tc_omp_base", prefix), r"total_num_triangles = (\d+)"),
           "diamond": _last_int(O.run_ref("sgl_omp_base", prefix, "diamond"), r"total_num = (\d+)"),
           "rectangle": _last_int(O.run_ref("sgl_omp_base", prefix, "rectangle"), r"total_num = (\d+)")}
    for k in (4, 5):
        out[f"clique{k}"] = _last_int(O.run_ref("clique_omp_base", prefix, k), rf"num_{k}-cliques = (\d+)")
    out["motif3"] = [int(re.search(r": (\d+)", ln).group(1)) for ln in O.run_ref("motif_omp_base", prefix, 3) if ln.startswith("pattern")]
    return out


@pytest.mark.parametrize("case", CASES)
def test_all_solvers_agree_with_reference(tmp_path, case):
    g = case_graph(case)
    if not (0 < g.max_degree < g.V()):
        pytest.skip("reference loader asserts 0 < max_degree < nv")
    want = gold(case_key(case))
    assert csr_sha(g) == want["csr_sha256"]  # the graph the answers were recorded on
    if O.ref_binary("tc_omp_base") is not None:  # the live reference, where it is built
        prefix = str(tmp_path / "g" / "graph")
        g.save(prefix)
        assert ref_answers(prefix) == {k: v for k, v in want.items() if k != "csr_sha256"}
    sym = O.OGraph(g.row_ptr, g.col_idx)
    dag = O.orient(sym)
    assert O.tc(dag) == want["tc"]
    assert O.diamond(sym) == want["diamond"]
    assert O.rectangle(sym) == want["rectangle"]
    for k in (4, 5):
        assert O.clique(dag, k) == want[f"clique{k}"]
    assert O.motif3(sym) == want["motif3"]


def test_oracle_cli_prints_the_reference_result_line(tmp_path):
    """config 1: tc_omp_base on citeseer -> 'total_num_triangles = 1166' (CPU-only plumbing)."""
    import subprocess

    exe = os.path.join(ROOT, "oracle", "bin", "tc_omp_base")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "bin/tc_omp_base"], stdout=subprocess.DEVNULL)
    prefix = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")
    mine = subprocess.run([exe, prefix], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    ref = gold("citeseer_tc_omp_base")
    if O.ref_binary("tc_omp_base") is not None:
        live = O.run_ref("tc_omp_base", prefix)
        assert [live[0], live[-1]] == [ref["first_line"], ref["last_line"]]
    assert mine[-1] == ref["last_line"] == "total_num_triangles = 1166"
    assert mine[0] == ref["first_line"]  # banner line, src/triangle/main.cc:13
