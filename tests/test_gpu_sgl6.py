"""6path and dumbbell on the GPU (gm_sgl6_need / gm_sgl6_raw / gm_sgl6_finish / gm_sgl6, csrc/gm_wrect.hip) against tests/golden/sgl6.json (the
reference's sgl_omp_base) and against the numpy forms of tests/sgl6_ref.py: the nine raw sums one by one, the degree-weighted 4-cycle kernel
across several LDS ranges and on the graph as numbered, counters past 16 and 32 bits, rows beyond the workgroup's threads (K_n, and the
graded dense stage cell of tests/dense_graded.py with unequal degrees and supports), the hub corner, the neighbours' arrays, the refusals
and the app.  Every value is printed before it is asserted."""
import ctypes as C
import functools
import json
import os
import subprocess

import pytest

import dense_graded as DG
import sgl6_ref as R6
import twin_graphs as T
from common import GOLDEN, ROOT, load_graph, sup_core_info
from graphminer_amd import SglSolver, _lib
from graphminer_amd.solvers import sgl6, sgl6_finish, sgl6_need, sgl6_raw, tc_local

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
with open(os.path.join(ROOT, "tests", "golden", "sgl6.json")) as f:
    SGL6 = json.load(f)
with open(os.path.join(ROOT, "tests", "golden", "sgl5.json")) as f:
    SGL5 = json.load(f)
GRAPHS = [k for k in SGL6 if not k.startswith("_")]
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
    return R6.raw_sums(load_graph(name))


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def named(raw):
    return dict(zip(R6.RAW, raw))


@pytest.mark.parametrize("name", GRAPHS)
def test_goldens(dev, name):
    sym = load_graph(name).to_device(dev)
    for pat in R6.PATTERNS:
        if pat in SGL6[name]:
            check(f"{name} {pat}", sgl6(sym, pat), SGL6[name][pat])
    assert any(pat in SGL6[name] for pat in R6.PATTERNS)


@pytest.mark.parametrize("name", SMALL)
def test_raw_sums(dev, name):
    sym = load_graph(name).to_device(dev)
    want = numpy_raw(name)
    got, st = sgl6_raw(sym, "all", return_stats=True)
    for k, v in zip(R6.RAW, got):
        check(f"{name} raw {k}", v, want[k])
    assert st.tasks == load_graph(name).E() and st.kernel_ms > 0
    for pat in R6.PATTERNS:  # a pattern fills exactly its sums and zeroes the rest
        got = named(sgl6_raw(sym, pat))
        assert got == {k: (want[k] if k in R6.NEEDS[pat] else 0) for k in R6.RAW}, pat
    got = named(sgl6_raw(sym, ("Z",)))  # Z alone
    assert got == {k: (want[k] if k == "Z" else 0) for k in R6.RAW}
    got = named(sgl6_raw(sym, R6.mask(("R", "Y"))))  # (R without Z: the rectangle path)
    assert got == {k: (want[k] if k in ("R", "Y") else 0) for k in R6.RAW}


@pytest.mark.parametrize("width", [None, 16, 100, 256])
def test_ranges_and_numbering(dev, devopt, width):
    """rmat10 (1024 ids): with 16 / 100 / 256 ids per LDS range the centres span up to 64 / 11 / 4 ranges; both numberings; the R of the new
    kernel against the rectangle path"""
    name = "rmat10_ef16_s42"
    want = numpy_raw(name)
    devopt("GM_WRECT_RANGE", None if width is None else str(width))
    sym = load_graph(name).to_device(dev)  # (a fresh handle: the option is read when the plan is built)
    rect = SglSolver(sym, "rectangle")
    check(f"{name} rectangle path", rect, want["R"])
    for tune in (None, t6(AS_NUMBERED)):
        got = named(sgl6_raw(sym, ("Z", "R"), tune=tune))
        check(f"{name} width {width} tune {tune} Z", got["Z"], want["Z"])
        check(f"{name} width {width} tune {tune} R", got["R"], rect)
        check(f"{name} width {width} tune {tune} 6path", sgl6(sym, "6path", tune=tune), SGL6[name]["6path"])


def test_counter_widths(dev):
    """K_{2,70000}: one end with n = 70,000 > 65,535 2-paths, C(n, 2) > 2^31, Z > 2^47 (default numbering only: as numbered the walk is
    about 5 * 10^9 arrivals).  K_{3,3000}: every sum, both patterns."""
    a, b = 2, 70000
    want = R6.kab_raw(a, b)
    assert want["R"] > 2**31 and want["Z"] > 2**47
    got = named(sgl6_raw(T.graph("kab", (a, b)).to_device(dev), ("Z", "R")))
    for k in ("Z", "R"):
        check(f"K_{a},{b} raw {k}", got[k], want[k])
    assert all(got[k] == 0 for k in R6.RAW if k not in ("Z", "R"))
    g = T.graph("kab", (3, 3000))
    want = R6.raw_sums(g)
    assert {k: want[k] for k in ("R", "Z", "C5")} == R6.kab_raw(3, 3000)
    assert all(want[k] == 0 for k in ("Y", "C5", "M", "B", "K4")) and want["X"] > 0
    sym = g.to_device(dev)
    got = named(sgl6_raw(sym, "all"))
    for k in R6.RAW:
        check(f"K_3,3000 raw {k}", got[k], want[k])
    for pat in R6.PATTERNS:
        check(f"K_3,3000 {pat}", sgl6(sym, pat), R6.finish(pat, want))


def test_long_rows(dev, devopt):
    """K_300: rows beyond 256 entries (a task per range of a centre), both patterns against the analytic values.  K_1100: rows beyond 1024
    entries, Z, R, M, X, Y against numpy; with 16 ids per range its 69 ranges share the 64 bits of a row's mask"""
    n = 300
    sym = T.graph("complete", (n,)).to_device(dev)
    for pat in R6.PATTERNS:
        check(f"K_{n} {pat}", sgl6(sym, pat), R6.complete_counts(n)[pat])
    n = 1100
    keys = ("Z", "R", "M", "X", "Y")
    g = T.graph("complete", (n,))
    want = R6.raw_sums(g, need=keys)
    got = named(sgl6_raw(g.to_device(dev), keys))
    for k in R6.RAW:
        check(f"K_{n} raw {k}", got[k], want[k])
    devopt("GM_WRECT_RANGE", "16")
    got = named(sgl6_raw(g.to_device(dev), ("Z", "R")))
    for k in ("Z", "R"):
        check(f"K_{n} 16 ids per range raw {k}", got[k], want[k])


def test_graded_stage_cell(dev, devopt):
    """graded(1500, 0.90) of tests/dense_graded.py beside K_1100 above, where every degree and support is the same: rows beyond 1024 entries
    with 173 distinct degrees and 322 distinct supports -- the degree-weighted Z and the per-entry X, M, Y against the dense reference, on
    the default copy and as numbered; Z, R again with 16 ids per LDS range (94 ranges share the 64 bits of a row's mask)"""
    keys = ("Z", "R", "M", "X", "Y")
    g, want = DG.cell("stage"), DG.reference("stage")["raw6"]
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            got = named(sgl6_raw(sym, keys, tune=tune))
            for k in R6.RAW:
                check(f"stage cell tune {tune} raw {k}", got[k], want[k] if k in keys else 0)
    devopt("GM_WRECT_RANGE", "16")
    with g.to_device(dev) as sym:  # (a fresh handle: the option is read when the plan is built)
        got = named(sgl6_raw(sym, ("Z", "R")))
        for k in ("Z", "R"):
            check(f"stage cell 16 ids per range raw {k}", got[k], want[k])


def test_hub_corner(dev, devopt):
    """X, M, Y read the supports, 2 T_v and the degrees the 5-vertex pass leaves on the DAG: here on a handle whose task lists leave the
    rows of the last 512 vertices to the matrix cores (the set-up of tests/test_gpu_supcorner.py; gm_sup_core_info proves the corner)"""
    devopt("GM_TOPO_MIN_ROW", "0")
    devopt("GM_SUP_CORE_H", "512")
    name = "rmat10_ef16_s42"
    want = numpy_raw(name)
    with load_graph(name).to_device(dev) as sym:
        got = named(sgl6_raw(sym, ("M", "X", "Y")))
        info = sup_core_info(sym)
        check("corner vertices", info["vertices"], 512)
        assert info["entries"] > 0
        for k in ("M", "X", "Y"):
            check(f"{name} corner raw {k}", got[k], want[k])


def test_neighbours_unharmed(dev):
    name = "rmat10_ef16_s42"
    sym = load_graph(name).to_device(dev)
    before = (SglSolver(sym, "diamond"), SglSolver(sym, "hourglass"), tc_local(sym, vertex=False, entries=False)[0])
    check("before", before, (GOLDEN[name]["diamond"], SGL5[name]["hourglass"], GOLDEN[name]["tc"]))
    for pat in R6.PATTERNS:
        check(f"{name} {pat}", sgl6(sym, pat), SGL6[name][pat])
    after = (SglSolver(sym, "diamond"), SglSolver(sym, "hourglass"), tc_local(sym, vertex=False, entries=False)[0])
    check("after", after, before)
    check("finish of raw", sgl6_finish("dumbbell", sgl6_raw(sym, "dumbbell")), SGL6[name]["dumbbell"])


def test_refusals(dev, devopt, capsys):
    import numpy as np
    import torch

    from graphminer_amd import Graph

    g = load_graph("citeseer")
    sym = g.to_device(dev)
    lib = _lib.load()
    total, raw = C.c_uint64(5), (C.c_uint64 * 9)()
    every = sgl6_need("all")
    la = _lib.gm_launch()
    la.rank, la.world = 0, 2
    assert lib.gm_sgl6(sym.handle, b"6path", C.byref(la), C.byref(total), None) == _lib.GM_ERR_UNSUPPORTED and total.value == 0
    assert lib.gm_sgl6_raw(sym.handle, every, C.byref(la), raw, None) == _lib.GM_ERR_UNSUPPORTED
    buf = torch.zeros(16, dtype=torch.int64, device=f"cuda:{dev}")
    la = _lib.gm_launch()
    la.d_counts = buf.data_ptr()
    assert lib.gm_sgl6_raw(sym.handle, every, C.byref(la), raw, None) == _lib.GM_ERR_UNSUPPORTED
    assert lib.gm_sgl6(sym.handle, b"dumbbell", C.byref(la), C.byref(total), None) == _lib.GM_ERR_UNSUPPORTED
    for name in (b"diamond", b"hourglass", b"all", b""):
        total = C.c_uint64(5)
        assert lib.gm_sgl6(sym.handle, name, None, C.byref(total), None) == _lib.GM_ERR_INVALID and total.value == 0
    assert lib.gm_sgl6(sym.handle, None, None, C.byref(total), None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6(sym.handle, b"6path", None, None, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6(None, b"6path", None, C.byref(total), None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_raw(sym.handle, 0, None, raw, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_raw(sym.handle, 1 << 9, None, raw, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_raw(sym.handle, every, None, None, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_raw(None, every, None, raw, None) == _lib.GM_ERR_INVALID
    # a handle of "2^31 entries or more" (the developer option gives a small graph such a handle)
    devopt("GM_BIG_NE", "1")
    big = g.to_device(dev)
    devopt("GM_BIG_NE", None)
    assert lib.gm_sgl6_raw(big.handle, every, None, raw, None) == _lib.GM_ERR_TOO_LARGE
    assert lib.gm_sgl6(big.handle, b"6path", None, C.byref(total), None) == _lib.GM_ERR_TOO_LARGE
    # unsorted rows
    rev = g.col_idx.copy()
    for v in range(g.V()):
        a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
        rev[a:b] = rev[a:b][::-1]
    with Graph(row_ptr=g.row_ptr.copy(), col_idx=rev, name="citeseer_descending").to_device(dev) as d:
        for need in (every, R6.mask(("K4",)), R6.mask(("Z",))):
            assert lib.gm_sgl6_raw(d.handle, need, None, raw, None) == _lib.GM_ERR_INVALID and b"ascending" in lib.gm_last_error()
    # no edges: GM_OK with zeros
    empty = Graph(row_ptr=np.zeros(6, np.int64), col_idx=np.zeros(0, np.int32), name="empty5")
    with empty.to_device(dev) as d:
        raw[3] = 7
        assert lib.gm_sgl6_raw(d.handle, every, None, raw, None) == _lib.GM_OK and list(raw) == [0] * 9
        total = C.c_uint64(5)
        assert lib.gm_sgl6(d.handle, b"6path", None, C.byref(total), None) == _lib.GM_OK and total.value == 0
    # gm_sgl keeps its answer for the two names, also after gm_sgl6 has run on the handle
    check("citeseer 6path", sgl6(sym, "6path"), SGL6["citeseer"]["6path"])
    for pat in (b"6path", b"dumbbell"):
        total = C.c_uint64(5)
        assert lib.gm_sgl(sym.handle, pat, None, C.byref(total), None) == _lib.GM_ERR_UNSUPPORTED and total.value == 0
    assert SglSolver(sym, "6path") == 0 and "Not implemented" in capsys.readouterr().out


def test_app_citeseer(dev):
    exe = os.path.join(ROOT, "graphminer_amd", "bin", "sgl6_gpu_base")
    prefix = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")
    for pat in R6.PATTERNS:
        r = subprocess.run([exe, prefix, pat], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        check(f"sgl6_gpu_base {pat}", r.stdout.strip().splitlines()[-1], f"total_num = {SGL6['citeseer'][pat]}")
    r = subprocess.run([exe, prefix, "diamond"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
