"""The six 5-vertex patterns of the reference's sgl solver beyond house / pentagon (hourglass, taileddiamond, taileddiamond2, closedhouse,
semihouse, 5path) on the GPU: closed forms of eleven raw sums (gm_sgl5_raw / gm_sgl5_finish, csrc/gm_wtri.hip) against
tests/golden/sgl5.json (the reference's sgl_omp_base) and against the numpy forms of tests/sgl5_ref.py, through every path of the
support-weighted triangle pass: both LDS stage sizes, rows beyond the 2048-entry stage, the numbering switch, supports past 16 bits,
closedhouse sets past their LDS capacity.  The K_n cells prove that every triangle is visited once; the graded dense cells beside them
(tests/dense_graded.py: supports and degrees that differ from entry to entry, a dense float64 reference) prove that every support and degree
is read at its own entry -- on both stages, beyond the stage, in the hub-corner branch -- and closedhouse sits on both sides of its LDS cap.
Every value is printed before it is asserted."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import dense_graded as DG
import planted_squares as P
import sgl5_ref as R5
import twin_graphs as T
from common import GOLDEN, ROOT, gm_constant, load_graph, sup_core_info
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


# ---- the graded dense cells (tests/dense_graded.py): the same paths with supports and degrees that differ from entry to entry ---------------
WEIGHTED = ("T", "D", "W", "A", "B", "H", "S")  # the seven sums of the support pass and the weighted pass
STAGE_VARIANTS = {"default": (None, None, DG.DENSE5), "as-numbered": (t6(AS_NUMBERED), None, DG.DENSE5), "set-fallback": (t6(HSET_FALLBACK), None, ("A", "B")),
                  "split-always": (None, "1", WEIGHTED)}


@functools.lru_cache(maxsize=None)
def cell_rows(name):
    f = DG.row_facts(DG.cell(name), gm_constant("tct_stage_max"))
    print(f"{name} graded{DG.CELLS[name]}: longest DAG row {f['longest']}, rows in (1024, stage] {f['stage']}, beyond {f['beyond']}", flush=True)
    return f


def check_sums(label, sym, keys, want, tune=None):
    got = dict(zip(R5.RAW, sgl5_raw(sym, keys, tune=tune)))
    for k in keys:
        check(f"{label} raw {k}", got[k], want[k])
    assert all(got[k] == 0 for k in R5.RAW if k not in keys), label


@pytest.mark.parametrize("variant", list(STAGE_VARIANTS))
def test_graded_stage_cell(dev, devopt, variant):
    """graded(1500, 0.90): 344 DAG rows of 1025 .. 1263 entries on the 2048-entry stage, 322 distinct supports, 173 distinct degrees --
    beside K_1300 above, whose sums do not change when a support or a degree is read at a wrong entry.  The sums are asked for by name:
    the 4-cliques, the rectangles and closedhouse's sets of a graph this dense are not this test's business.  A fresh handle each."""
    tune, split, keys = STAGE_VARIANTS[variant]
    f = cell_rows("stage")
    assert f["stage"] >= 64 and f["beyond"] == 0
    devopt("GM_TCT_SPLIT_ALWAYS", split)
    with DG.cell("stage").to_device(dev) as sym:
        check_sums(f"stage cell {variant}", sym, keys, DG.reference("stage")["raw5"], tune=tune)


def test_graded_beyond_cell(dev):
    """graded(2200, 0.975): 69 DAG rows beyond the 2048-entry stage -- their out-edges are the wave-per-edge kernels' (sup_long_kernel,
    wtri_edge_kernel with its row list); beside K_2060 above"""
    f = cell_rows("beyond")
    assert f["beyond"] >= 64
    with DG.cell("beyond").to_device(dev) as sym:
        check_sums("beyond cell", sym, WEIGHTED, DG.reference("beyond")["raw5"])


@pytest.mark.parametrize("name,keys", [("stage", DG.DENSE5), ("beyond", WEIGHTED)])
def test_graded_cells_with_shuffled_ids(dev, name, keys):
    """the sums do not depend on the numbering; the DAG the pass builds from a shuffled graph breaks its degree ties elsewhere"""
    h, _ = P.shuffled(DG.cell(name), seed=13)
    with h.to_device(dev) as sym:
        check_sums(f"{name} cell shuffled", sym, keys, DG.reference(name)["raw5"])


@pytest.mark.parametrize("name,h", [("rmat10_ef16_s42", 512), ("corner", 1024)])
def test_hub_corner(dev, devopt, name, h):
    """the branch `corner_from < nv` of the weighted pass: the task lists leave the rows of the last h vertices out, the supports of their
    edges come from the matrix cores, and wtri_edge_kernel walks their out-edges from the rows themselves (no row list, the tail of N+(u)
    beyond v).  gm_sup_core_info proves that the handle has that corner.  On the stage cell itself the library declines a corner: it takes
    whole 512-vertex chunks that start at a word of the core bitmap's rows, so nv - h must be a multiple of 32; the "corner" cell is the
    stage cell's recipe on 1504 vertices (longest DAG row 1,266: everything on the 2048-entry stage)."""
    devopt("GM_TOPO_MIN_ROW", "0")
    devopt("GM_SUP_CORE_H", str(h))
    if name in DG.CELLS:
        f = cell_rows(name)
        assert f["stage"] >= 64 and f["beyond"] == 0
        g, want = DG.cell(name), DG.reference(name)["raw5"]
    else:
        g, want = load_graph(name), numpy_raw(name)
    with g.to_device(dev) as sym:  # (a fresh handle: the options are read when its tables are built)
        check_sums(f"{name} corner {h}", sym, WEIGHTED, want)
        info = sup_core_info(sym)
        check(f"{name} corner vertices", info["vertices"], h)
        print(f"{name} corner entries {info['entries']}", flush=True)
        assert info["entries"] > 0
        check_sums(f"{name} corner {h} again", sym, ("A", "B"), want)


def spine_graph(du, dv, seed):
    """two adjacent spine vertices 0 and 1 of du <= dv neighbours: du - 1 common pages, dv - du pages of vertex 1 alone, and 3 du seeded
    random edges among the common pages"""
    assert 3 <= du <= dv
    pages = np.arange(2, du + 1, dtype=np.int64)
    own = np.arange(du + 1, dv + 1, dtype=np.int64)
    rng = np.random.default_rng(seed)
    a, b = rng.integers(2, du + 1, 6 * du), rng.integers(2, du + 1, 6 * du)
    keys = np.unique(np.minimum(a, b)[a != b] * (dv + 1) + np.maximum(a, b)[a != b])
    keys = keys[rng.permutation(keys.size)[:3 * du]]
    assert keys.size == 3 * du
    s = np.concatenate([[0], np.zeros(pages.size, np.int64), np.ones(pages.size + own.size, np.int64), keys // (dv + 1)])
    return P._graph(dv + 1, s, np.concatenate([[1], pages, pages, own, keys % (dv + 1)]))


@pytest.mark.parametrize("du,dv,in_lds", [(-1, -1, True), (0, 0, True), (1, 1, False), (1, 400, False)])
def test_closedhouse_at_the_lds_cap(dev, du, dv, in_lds):
    """chouse_kernel keeps S = N(u) ^ N(v) in LDS while min(d(u), d(v)) <= chouse_lds_keys and in the global scratch beyond: spine edges
    with cap - 1, cap, cap + 1 keys on both sides, and one of cap + 1 and cap + 400 -- the shorter list decides.  The pages' own edges put
    hundreds of keys inside S"""
    cap = gm_constant("chouse_lds_keys")
    du, dv = cap + du, cap + dv
    g = spine_graph(du, dv, seed=du)
    deg = np.diff(g.row_ptr)
    want = R5.raw_sums(g, need=("Q",))["Q"]
    print(f"spine degrees {int(deg[0])}, {int(deg[1])} against the cap {cap}; largest page degree {int(deg[2:].max())}", flush=True)
    assert (int(deg[0]), int(deg[1])) == (du, dv) and int(deg[2:].max()) < cap - 1
    assert (min(int(deg[0]), int(deg[1])) <= cap) is in_lds and want > 0
    with g.to_device(dev) as sym:
        check(f"closedhouse spine {du}, {dv}", SglSolver(sym, "closedhouse"), want)


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
    assert lib.gm_sgl5_raw_need(sym.handle, 0b11000, C.byref(la), raw, None) == _lib.GM_ERR_UNSUPPORTED  # the same by bit mask
    assert lib.gm_sgl5_raw_need(sym.handle, 0, None, raw, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl5_raw_need(sym.handle, 1 << 11, None, raw, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl5_raw_need(None, 1, None, raw, None) == _lib.GM_ERR_INVALID
    assert sgl5_raw(sym, ("A", "B", "P")) == [v if k in "ABP" else 0 for k, v in numpy_raw("citeseer").items()]
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
