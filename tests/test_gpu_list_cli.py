"""bin/tclist_gpu_base on citeseer: the two result lines, the file of raw int32 triples against tests/list_ref.py, a window."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, load_graph
from list_ref import list_ref, sort_rows

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "tclist_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def run(*args):
    r = subprocess.run([EXE, PREFIX, *map(str, args)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-400:], r.stderr[-400:], flush=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


def test_app_citeseer(tmp_path):
    out = tmp_path / "out.bin"
    lines = run(out)
    assert lines[-2:] == ["total_num_triangles = 1166", "triangles_written = 1166"], lines[-2:]
    tri = np.fromfile(out, dtype="<i4").reshape(-1, 3)
    want = list_ref(load_graph("citeseer"))
    print(f"file: {tri.shape} rows, reference {want.shape}", flush=True)
    assert np.array_equal(sort_rows(tri), want)
    lines = run(out, 1000, 500)
    assert lines[-2:] == ["total_num_triangles = 1166", "triangles_written = 166"], lines[-2:]
    window = np.fromfile(out, dtype="<i4").reshape(-1, 3)
    assert np.array_equal(window, tri[1000:])
    # count only
    assert run()[-2:] == ["total_num_triangles = 1166", "triangles_written = 0"]
