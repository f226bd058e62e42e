"""bin/rectlocal_gpu_base on citeseer: the three result lines and the two files of raw uint64 against the Python call (rect_local) and
tests/rect_local_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import rect_local_ref as R
from common import GOLDEN, ROOT, load_graph

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "rectlocal_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def run(*args):
    r = subprocess.run([EXE, PREFIX, *map(str, args)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-400:], r.stderr[-400:], flush=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [line for line in r.stdout.splitlines() if line.strip()]


def test_app_citeseer(tmp_path):
    from graphminer_amd import rect_local

    g = load_graph("citeseer")
    with g.to_device(0) as sym:
        total, want_rv, want_ent = rect_local(sym)
    ref_ent, ref_rv = R.rect_local(g)
    assert total == GOLDEN["citeseer"]["rectangle"] and np.array_equal(want_ent, ref_ent) and np.array_equal(want_rv, ref_rv)
    want_lines = [f"max_vertex_rectangles = {int(want_rv.max())}", f"max_edge_rectangles = {int(want_ent.max())}", f"total_num = {total}"]
    out = tmp_path / "out"
    lines = run(out)
    assert lines[-3:] == want_lines, lines[-3:]
    rv = np.fromfile(str(out) + ".vertex.u64", dtype="<u8")
    ent = np.fromfile(str(out) + ".entry.u64", dtype="<u8")
    print(f"files: {rv.shape} vertices, {ent.shape} entries; the Python call {want_rv.shape}, {want_ent.shape}", flush=True)
    assert np.array_equal(rv, want_rv) and np.array_equal(ent, want_ent)
    # without an out prefix: the three lines, no files
    assert run()[-3:] == want_lines
