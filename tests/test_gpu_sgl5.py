"""The six 5-vertex patterns of the reference's sgl solver beyond house / pentagon (hourglass, taileddiamond, taileddiamond2, closedhouse,
semihouse, 5path) on the GPU: closed forms of eleven raw sums (gm_sgl5_raw / gm_sgl5_finish, csrc/gm_wtri.hip) against
tests/golden/sgl5.json (the reference's sgl_omp_base) and against the numpy forms of tests/sgl5_ref.py, through every path of the
support-weighted triangle pass: both LDS stage sizes, rows beyond the 2048-entry stage, the numbering switch, supports past 16 bits,
closedhouse sets past their LDS capacity.  Every value is printed before it is asserted."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import sgl5_ref as R5
import twin_graphs as T
from common import GOLDEN, ROOT, load_graph
from graphminer_amd import SglSolver, _lib
from graphminer_amd.solvers import sgl5_finish, sgl5_raw

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
HSET_FALLBACK = 0x800000
with open(os.path.join(ROOT, "tests", "golden", "sgl5.json")) as f:
    SGL5 = json.load(f)
GRAPHS = [k for k in SGL5 if not k.startswith("_")]
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def numpy_raw(name):
    return R5.raw_sums(load_graph(name))


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


@pytest.mark.parametrize("name", GRAPHS)
def test_goldens(dev, name):
    sym = load_graph(name).to_device(dev)
    for pat in R5.PATTERNS:
        if pat in SGL5[name]:
            check(f"{name} {pat}", SglSolver(sym, pat), SGL5[name][pat])
    assert any(pat in SGL5[name] for pat in R5.PATTERNS)


def test_drop_in_binary_citeseer(dev):
    exe = os.path.join(ROOT, "graphminer_amd", "bin", "sgl_gpu_base")
    prefix = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")
    for pat in R5.PATTERNS:
        r = subprocess.run([exe, prefix, pat], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        check(f"sgl_gpu_base {pat}", r.stdout.strip().splitlines()[-1], f"total_num = {SGL5['citeseer'][pat]}")
    r = subprocess.run([os.path.join(ROOT, "graphminer_amd", "bin", "sgl_multigpu"), prefix, "hourglass", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Not implemented" not in r.stdout, r.stdout + r.stderr  # (the one-GPU path at every n_gpu)
    check("sgl_multigpu hourglass", r.stdout.strip().splitlines()[-1], f"total_num = {SGL5['citeseer']['hourglass']}")


@pytest.mark.parametrize("name", SMALL)
def test_raw_sums(dev, name):
    sym = load_graph(name).to_device(dev)
    want = numpy_raw(name)
    got, st = sgl5_raw(sym, "all", return_stats=True)
    for k, v in zip(R5.RAW, got):
        check(f"{name} raw {k}", v, want[k])
    assert st.tasks == load_graph(name).E() and st.kernel_ms > 0
    # a pattern fills what it needs and zeroes the rest
    got = dict(zip(R5.RAW, sgl5_raw(sym, "hourglass")))
    assert got == {k: (want[k] if k in ("H", "D") else 0) for k in R5.RAW}
    got = dict(zip(R5.RAW, sgl5_raw(sym, "5path")))
    assert got == {k: (want[k] if k in ("P", "S", "T", "R") else 0) for k in R5.RAW}


@pytest.mark.parametrize("name", ["citeseer", "rmat10_ef16_s42"])
def test_numbering_and_fallback_lookup(dev, name):
    sym = load_graph(name).to_device(dev)
    for pat in R5.PATTERNS:
        check(f"{name} {pat} as numbered", SglSolver(sym, pat, tune=t6(AS_NUMBERED)), SGL5[name][pat])
    for pat in ("taileddiamond", "semihouse"):  # the weighted pass with every lookup through the set's global-memory fallback
        check(f"{name} {pat} fallback", SglSolver(sym, pat, tune=t6(HSET_FALLBACK)), SGL5[name][pat])


def k_n(dev, n):
    return T.graph("complete", (n,)).to_device(dev)


K_PATTERNS = ("hourglass", "taileddiamond", "taileddiamond2", "semihouse")
NEEDS = {"hourglass": ("H", "D"), "taileddiamond": ("A", "K4"), "taileddiamond2": ("W",), "semihouse": ("B", "K4")}


def test_stage_2048(dev, devopt):
    """K_1300: DAG rows of up to 1299 entries -- the 2048-entry stage of the weighted pass (the goldens run on the 1024-entry one); with
    GM_TCT_SPLIT_ALWAYS both kernels in one launch, each on the hosts of its own table"""
    n = 1300
    want = R5.complete_raw(n)
    g = T.graph("complete", (n,))
    for split in (None, "1"):
        devopt("GM_TCT_SPLIT_ALWAYS", split)
        sym = g.to_device(dev)  # (a fresh handle: the option is read when its tables are built)
        for pat in K_PATTERNS if split is None else ("taileddiamond", "semihouse"):
            raw = dict(zip(R5.RAW, sgl5_raw(sym, pat)))
            for k in NEEDS[pat]:
                check(f"K_{n} split={split} {pat} raw {k}", raw[k], want[k])
            check(f"K_{n} split={split} {pat}", sgl5_finish(pat, [raw[k] for k in R5.RAW]), R5.finish(pat, want))


def test_rows_beyond_the_stage(dev):
    """K_2060: the DAG rows of 2049 .. 2059 entries host nothing -- their out-edges are the wave-per-edge kernel's"""
    n = 2060
    want = R5.complete_raw(n)
    sym = k_n(dev, n)
    for pat in K_PATTERNS:
        check(f"K_{n} {pat}", SglSolver(sym, pat), R5.finish(pat, want))


def test_closedhouse_beyond_lds_capacity(dev):
    """B_1500 with a path among four pages: the spine edge's common neighbours (1500 > the 1024-key LDS set) go to the global scratch"""
    from graphminer_amd.rmat import csr_from_pairs

    n, s, d = T.pairs("book", (1500,))
    s = np.concatenate([s, np.array([2, 3, 4])]).astype(np.uint64)
    d = np.concatenate([d, np.array([3, 4, 5])]).astype(np.uint64)
    g = csr_from_pairs(n, s, d)
    want = R5.raw_sums(g, need=("Q",))["Q"]
    assert want != 0
    check("book + path closedhouse", SglSolver(g.to_device(dev), "closedhouse"), want)


def test_supports_beyond_16_bits(dev):
    """B_70000: t(spine) = 70,000 > 65,535 and C(T_v, 2) of the spine ends > 2^32"""
    g = T.graph("book", (70000,))
    want = R5.raw_sums(g, need=("T", "D", "W", "H", "S"))
    assert want["H"] > 2**32
    sym = g.to_device(dev)
    for pat, keys in (("hourglass", "HD"), ("taileddiamond2", "W")):
        raw = dict(zip(R5.RAW, sgl5_raw(sym, pat)))
        for k in keys:  # (hourglass itself is 0 on a book: H = 2 D)
            check(f"B_70000 {pat} raw {k}", raw[k], want[k])
        check(f"B_70000 {pat}", SglSolver(sym, pat), R5.finish(pat, want))


def test_refusals(dev, capsys):
    import ctypes as C

    sym = load_graph("citeseer").to_device(dev)
    lib = _lib.load()
    la = _lib.gm_launch()
    la.rank, la.world = 0, 2
    total, raw = C.c_uint64(5), (C.c_uint64 * 11)()
    assert lib.gm_sgl(sym.handle, b"hourglass", C.byref(la), C.byref(total), None) == _lib.GM_ERR_UNSUPPORTED and total.value == 0
    assert lib.gm_sgl5_raw(sym.handle, b"all", C.byref(la), raw, None) == _lib.GM_ERR_UNSUPPORTED
    assert lib.gm_sgl5_raw(sym.handle, b"diamond", None, raw, None) == _lib.GM_ERR_INVALID
    for pat in (b"6path", b"dumbbell"):
        total = C.c_uint64(5)
        assert lib.gm_sgl(sym.handle, pat, None, C.byref(total), None) == _lib.GM_ERR_UNSUPPORTED and total.value == 0


def test_diamond_unchanged(dev):
    name = "rmat10_ef16_s42"
    sym = load_graph(name).to_device(dev)
    check("diamond before", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
    for pat in ("taileddiamond", "hourglass"):
        check(pat, SglSolver(sym, pat), SGL5[name][pat])
    check("diamond after", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
    check("finish of raw", sgl5_finish("semihouse", sgl5_raw(sym, "semihouse")), SGL5[name]["semihouse"])
