"""cliquetruss_gpu_base (apps/gm_cli.cc) on citeseer at k = 3 and k = 4 against the Python calls: the decomposition with its two files read
back, and the (k, c)-truss query with its file.  Every value is printed before it is asserted."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, load_graph
from graphminer_amd import clique_ktruss, clique_truss_decompose

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "cliquetruss_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def fields(stdout):
    return {k.strip(): v.strip() for k, v in (line.split("=", 1) for line in stdout.splitlines() if " = " in line)}


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


@pytest.mark.parametrize("k", [3, 4])
def test_decomposition_query_and_files(tmp_path, k):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    with load_graph("citeseer").to_device(0) as sym:
        theta, rnd, c_max, rounds = clique_truss_decompose(sym, k)
        c = max(1, c_max // 2)
        edges, ncl, cnt, rounds_c = clique_ktruss(sym, k, c)
    out = str(tmp_path / "trusses")
    r = subprocess.run([EXE, PREFIX, str(k), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = fields(r.stdout)
    check("last line", r.stdout.strip().splitlines()[-1], f"max_truss = {c_max}")
    check("rounds", int(f["rounds"]), rounds)
    got_theta, got_rnd = np.fromfile(out + ".theta.bin", dtype="<u8"), np.fromfile(out + ".round.bin", dtype="<u4")
    check("theta.bin", (got_theta.shape, bool(np.array_equal(got_theta, theta))), (theta.shape, True))
    check("round.bin", (got_rnd.shape, bool(np.array_equal(got_rnd, rnd))), (rnd.shape, True))
    r = subprocess.run([EXE, PREFIX, str(k), str(c), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = fields(r.stdout)
    check(f"c = {c} (edges, cliques, rounds)", (int(f["truss_edges"]), int(f["truss_cliques"]), int(f["rounds"])), (edges, ncl, rounds_c))
    got_cnt = np.fromfile(out + ".cnt.bin", dtype="<u8")
    check("cnt.bin", (got_cnt.shape, bool(np.array_equal(got_cnt, cnt))), (cnt.shape, True))


def test_usage():
    r = subprocess.run([EXE, PREFIX], capture_output=True, text=True, timeout=300)
    check("without k", r.returncode, 1)
    r = subprocess.run([EXE, PREFIX, "9"], capture_output=True, text=True, timeout=300)
    check("k = 9", r.returncode, 1)
