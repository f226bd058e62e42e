"""nucleus34_gpu_base (apps/gm_cli.cc) on citeseer against the Python calls: the decomposition with its three files read back, and the
c-nucleus query with its files.  Every value is printed before it is asserted."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, load_graph
from graphminer_amd import nucleus34, nucleus34_decompose, tc_list, tri_clique4_local

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "nucleus34_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def fields(stdout):
    return {k.strip(): v.strip() for k, v in (line.split("=", 1) for line in stdout.splitlines() if " = " in line)}


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_file(path, dtype, want):
    got = np.fromfile(path, dtype=dtype).reshape((-1,) + want.shape[1:])
    check(os.path.basename(path), (got.shape, bool(np.array_equal(got, want))), (want.shape, True))


def test_decomposition_query_and_files(tmp_path):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    with load_graph("citeseer").to_device(0) as sym:
        T, rows = tc_list(sym)
        total, _ = tri_clique4_local(sym)
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)
        c = max(1, c_max // 2)
        ntri, ncl, cnt, rounds_c = nucleus34(sym, c)
    out = str(tmp_path / "nuclei")
    r = subprocess.run([EXE, PREFIX, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = fields(r.stdout)
    check("last line", r.stdout.strip().splitlines()[-1], f"max_nucleus = {c_max}")
    check("(T, 4-cliques, rounds)", (int(f["total_num_triangles"]), int(f["total_num_cliques"]), int(f["rounds"])), (T, total, rounds))
    check_file(out + ".tri.bin", "<i4", rows)
    check_file(out + ".theta.bin", "<u4", theta)
    check_file(out + ".round.bin", "<u4", rnd)
    out = str(tmp_path / "set")
    r = subprocess.run([EXE, PREFIX, str(c), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = fields(r.stdout)
    check(f"c = {c} (T, 4-cliques, triangles, cliques, rounds)",
          (int(f["total_num_triangles"]), int(f["total_num_cliques"]), int(f["nucleus_triangles"]), int(f["nucleus_cliques"]), int(f["rounds"])),
          (T, total, ntri, ncl, rounds_c))
    check_file(out + ".tri.bin", "<i4", rows)
    check_file(out + ".cnt.bin", "<u4", cnt)
    check("no round file with c", os.path.exists(out + ".round.bin"), False)
    r = subprocess.run([EXE, PREFIX], capture_output=True, text=True, timeout=300)  # (no files: the numbers alone)
    assert r.returncode == 0, r.stdout + r.stderr
    check("without an out prefix, last line", r.stdout.strip().splitlines()[-1], f"max_nucleus = {c_max}")


def test_usage():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    check("without a graph", r.returncode, 1)
