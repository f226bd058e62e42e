"""bin/cliquelist_gpu_base on citeseer: the two result lines, the file of raw int32 rows against the Python mirror and tests/clique_list_ref.py,
a window given by first / cap, a bad k."""
import os
import subprocess

import numpy as np
import pytest

from clique_list_ref import clique_list_ref
from common import ROOT, load_graph
from graphminer_amd import clique_list

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "cliquelist_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def run(*args, ok=True):
    r = subprocess.run([EXE, PREFIX, *map(str, args)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-400:], r.stderr[-400:], flush=True)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout.strip().splitlines(), r.stderr


def test_app_citeseer(tmp_path):
    out = tmp_path / "out.bin"
    lines, _ = run(4, out)
    assert lines[-2:] == ["total_num_cliques = 255", "cliques_written = 255"], lines[-2:]
    rows = np.fromfile(out, dtype="<i4").reshape(-1, 4)
    with load_graph("citeseer").to_device(0) as sym:
        mirror = clique_list(sym, 4)[0]
    want = clique_list_ref(load_graph("citeseer"), 4)
    print(f"file: {rows.shape} rows, mirror {mirror.shape}, reference {want.shape}", flush=True)
    assert np.array_equal(rows, mirror) and np.array_equal(rows, want)
    lines, _ = run(4, out, 200, 30)
    assert lines[-2:] == ["total_num_cliques = 255", "cliques_written = 30"], lines[-2:]
    assert np.array_equal(np.fromfile(out, dtype="<i4").reshape(-1, 4), rows[200:230])
    lines, _ = run(4, out, 250, 500)
    assert lines[-2:] == ["total_num_cliques = 255", "cliques_written = 5"], lines[-2:]
    assert np.array_equal(np.fromfile(out, dtype="<i4").reshape(-1, 4), rows[250:])
    # count only
    assert run(5)[0][-2:] == ["total_num_cliques = 46", "cliques_written = 0"]


@pytest.mark.parametrize("k", [2, 9, 13])
def test_app_bad_k(k):
    lines, err = run(k, ok=False)
    print(f"k = {k}: stderr {err!r}", flush=True)
    assert "cliquelist_gpu_base" in err and not any(line.startswith("total_num_cliques") for line in lines)
