"""bin/motiflocal_gpu_base on citeseer: the `orbit <o>: sum = S max = M` lines, the `pattern <i>: <count>` lines of motif_gpu_base as the
last lines, and the raw orbit-major file -- against the Python call on the same graph (itself checked against the references by
tests/test_gpu_motif_local.py)."""
import os
import subprocess

import numpy as np
import pytest

from common import GOLDEN, ROOT, load_graph
from graphminer_amd import motif_local

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "motiflocal_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def run(*args):
    r = subprocess.run([EXE, PREFIX, *map(str, args)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1200:], r.stderr[-400:], flush=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [line for line in r.stdout.splitlines() if line.strip()]


@pytest.mark.parametrize("k", [3, 4])
def test_app_citeseer(tmp_path, k):
    g = load_graph("citeseer")
    with g.to_device(0) as sym:
        counts, orb = motif_local(sym, k)
    assert counts == GOLDEN["citeseer"][f"motif{k}"]
    no, nc = orb.shape[0], len(counts)
    want_lines = [f"orbit {o}: sum = {int(orb[o].sum(dtype=np.uint64))} max = {int(orb[o].max())}" for o in range(no)]
    want_lines += [f"num_patterns: {nc}"] + [f"pattern {i}: {c}" for i, c in enumerate(counts)]
    out = tmp_path / "out"
    lines = run(k, out)
    assert lines[-len(want_lines):] == want_lines, lines[-len(want_lines):]
    raw = np.fromfile(str(out) + ".orbits.u64", dtype="<u8")
    print(f"file: {raw.shape} values; the Python call {orb.shape}", flush=True)
    assert raw.size == orb.size and np.array_equal(raw.reshape(orb.shape), orb)
    # without an out prefix: the same lines, no file
    assert run(k)[-len(want_lines):] == want_lines


def test_app_refuses_other_k():
    r = subprocess.run([EXE, PREFIX, "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "motiflocal_gpu_base" in r.stderr, (r.stdout, r.stderr)
