"""cliquecore_gpu_base (apps/gm_cli.cc) on citeseer at k = 3 against tests/clique_core_ref.py: the decomposition with its two files read back,
and the (k, c)-core query.  Every value is printed before it is asserted."""
import os
import subprocess

import numpy as np
import pytest

import clique_core_ref as R
from common import ROOT, load_graph

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "graphminer_amd", "bin", "cliquecore_gpu_base")
PREFIX = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")


def fields(stdout):
    return {k.strip(): v.strip() for k, v in (line.split("=", 1) for line in stdout.splitlines() if " = " in line)}


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def test_decomposition_and_its_files(tmp_path):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    d = R.decompose(load_graph("citeseer"), 3)
    out = str(tmp_path / "cores")
    r = subprocess.run([EXE, PREFIX, "3", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = fields(r.stdout)
    check("last line", r.stdout.strip().splitlines()[-1], f"max_core = {d.c_max}")
    check("rounds", int(f["rounds"]), d.rounds)
    check("dense", (int(f["dense_round"]), int(f["dense_vertices"]), int(f["dense_cliques"])), d.dense)
    check("density", f["dense_density"], f"{d.dense[2] / d.dense[1]:.6f}")
    core, rnd = np.fromfile(out + ".core.bin", dtype="<u8"), np.fromfile(out + ".round.bin", dtype="<u4")
    check("core.bin", (core.shape, bool(np.array_equal(core, d.core))), (d.core.shape, True))
    check("round.bin", (rnd.shape, bool(np.array_equal(rnd, d.round))), (d.round.shape, True))


def test_core_query_and_usage(tmp_path):
    g = load_graph("citeseer")
    for c in (2, 12, 13):
        _, nvert, ncl, rounds = R.kcore(g, 3, c)
        r = subprocess.run([EXE, PREFIX, "3", str(c)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        f = fields(r.stdout)
        check(f"c = {c} (vertices, cliques, rounds)", (int(f["core_vertices"]), int(f["core_cliques"]), int(f["rounds"])), (nvert, ncl, rounds))
    r = subprocess.run([EXE, PREFIX], capture_output=True, text=True, timeout=300)
    check("without k", r.returncode, 1)
    r = subprocess.run([EXE, PREFIX, "9"], capture_output=True, text=True, timeout=300)
    check("k = 9", r.returncode, 1)
