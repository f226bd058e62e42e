"""Local triangle counts on the GPU (gm_tc_local, csrc/gm_local.hip): the triangles at every vertex and the support of every entry, in the
caller's numbering and entry order, against the plain Python forms of tests/truss_ref.py -- entry by entry, vertex by vertex -- and the
total against TCSolver, through every path of the support pass at the smallest shape that reaches it: as numbered, the hash sets' fallback
lookup, the 2048-entry stage, rows beyond the stage, a support past 16 bits, the hub corner on the matrix cores, a shuffled numbering.
On the stage and beyond it the K_n cells (every support n - 2) stand beside the graded dense cells of tests/dense_graded.py, whose supports
differ from entry to entry and come from a dense float64 reference.  Every value is printed before it is asserted."""
import ctypes as C
import functools
import json
import os
from math import comb

import numpy as np
import pytest

import dense_graded as DG
import planted_squares as P
import truss_ref as TR
import twin_graphs as T
from common import GOLDEN, ROOT, gm_constant, load_graph
from graphminer_amd import SglSolver, TCSolver, _lib, tc_local

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
HSET_FALLBACK = 0x800000
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
with open(os.path.join(ROOT, "tests", "golden", "sgl5.json")) as f:
    SGL5 = json.load(f)


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def ref(name):
    g = load_graph(name)
    return TR.supports(g), TR.vertex_triangles(g)


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_arrays(label, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    print(f"{label}: {len(want)} values, {bad.size} differ, first at {bad[:5].tolist()}: got {np.asarray(got)[bad[:5]].tolist()} "
          f"want {np.asarray(want)[bad[:5]].tolist()}", flush=True)
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, label


def both_directions_equal(g, sup):
    src = np.repeat(np.arange(g.V(), dtype=np.int64), np.diff(g.row_ptr))
    dst = g.col_idx.astype(np.int64)
    o = np.argsort(np.minimum(src, dst) * g.V() + np.maximum(src, dst), kind="stable")
    return bool((sup[o][0::2] == sup[o][1::2]).all())


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs(dev, name):
    g = load_graph(name)
    want_sup, want_tv = ref(name)
    with g.to_device(dev) as sym:
        total, tv, sup, st = tc_local(sym, return_stats=True)
        check_arrays(f"{name} supports", sup, want_sup)
        check_arrays(f"{name} T_v", tv, want_tv)
        check(f"{name} total", total, GOLDEN[name]["motif3"][1])
        check(f"{name} both directions", both_directions_equal(g, sup), True)
        check(f"{name} stats.tasks", st.tasks, g.E())
        assert st.kernel_ms > 0
        with sym.orient() as dag:
            check(f"{name} total against TCSolver", total, TCSolver(dag))
        # either output left out; a second call on the same handle
        total, tv, sup = tc_local(sym, vertex=False)
        check(f"{name} supports only", (total, tv), (GOLDEN[name]["motif3"][1], None))
        check_arrays(f"{name} supports only", sup, want_sup)
        total, tv, sup = tc_local(sym, entries=False)
        check(f"{name} vertices only", (total, sup), (GOLDEN[name]["motif3"][1], None))
        check_arrays(f"{name} vertices only", tv, want_tv)
        check(f"{name} neither", tc_local(sym, vertex=False, entries=False), (GOLDEN[name]["motif3"][1], None, None))


@pytest.mark.parametrize("name", ["citeseer", "rmat10_ef16_s42"])
@pytest.mark.parametrize("bit", [AS_NUMBERED, HSET_FALLBACK])
def test_as_numbered_and_fallback_lookup(dev, name, bit):
    want_sup, want_tv = ref(name)
    with load_graph(name).to_device(dev) as sym:
        total, tv, sup = tc_local(sym, tune=t6(bit))
        check_arrays(f"{name} tune[6]={bit:#x} supports", sup, want_sup)
        check_arrays(f"{name} tune[6]={bit:#x} T_v", tv, want_tv)
        check(f"{name} tune[6]={bit:#x} total", total, GOLDEN[name]["motif3"][1])
        # the default numbering after the other one on the same handle
        total, tv, sup = tc_local(sym)
        check_arrays(f"{name} default after {bit:#x} supports", sup, want_sup)
        check_arrays(f"{name} default after {bit:#x} T_v", tv, want_tv)


@pytest.mark.parametrize("n", [1300, 2060])
def test_complete_graphs_on_the_big_stage_and_beyond(dev, n):
    """K_1300: DAG rows of up to 1299 entries, the 2048-entry stage; K_2060: the rows of 2049 .. 2059 entries are sup_long_kernel's"""
    g = T.graph("complete", (n,))
    with g.to_device(dev) as sym:
        total, tv, sup = tc_local(sym)
    check(f"K_{n} supports", np.unique(sup).tolist(), [n - 2])
    check(f"K_{n} T_v", np.unique(tv).tolist(), [comb(n - 1, 2)])
    check(f"K_{n} total", total, comb(n, 3))
    assert sup.shape == (g.E(),) and tv.shape == (n,)


@pytest.mark.parametrize("name", ["stage", "beyond"])
def test_graded_cells_entry_by_entry(dev, name):
    """the graded dense cells of tests/dense_graded.py beside the two K_n above, whose supports are all n - 2: 322 / 173 distinct supports
    on DAG rows of the 2048-entry stage (graded(1500, 0.90)) and beyond it (graded(2200, 0.975): sup_long_kernel), every entry and every
    vertex against the dense reference -- on the default copy, as numbered, and with shuffled ids"""
    g, ref = DG.cell(name), DG.reference(name)
    f = DG.row_facts(g, gm_constant("tct_stage_max"))
    print(f"{name} cell: longest DAG row {f['longest']}, rows in (1024, stage] {f['stage']}, beyond {f['beyond']}, distinct supports {f['supports']}", flush=True)
    assert (f["stage"] >= 64 and f["beyond"] == 0) if name == "stage" else f["beyond"] >= 64
    total_want = int(ref["tv"].sum()) // 3
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            total, tv, sup = tc_local(sym, tune=tune)
            check_arrays(f"{name} cell tune={tune} supports", sup, ref["sup"])
            check_arrays(f"{name} cell tune={tune} T_v", tv, ref["tv"])
            check(f"{name} cell tune={tune} total", total, total_want)
    h, newid = P.shuffled(g, seed=17)
    want_tv = np.empty_like(ref["tv"])
    want_tv[newid] = ref["tv"]
    with h.to_device(dev) as sym:
        total, tv, sup = tc_local(sym)
        check_arrays(f"{name} cell shuffled supports", sup, P.entries_to(g, newid, ref["sup"]))
        check_arrays(f"{name} cell shuffled T_v", tv, want_tv)
        check(f"{name} cell shuffled total", total, total_want)


def test_graded_stage_cell_rank_shares_and_diamond(dev):
    """the stage cell: the shares of two and of three ranks of the support pass add up, entry by entry, to the one-rank array (the idiom of
    tests/test_gpu_supcorner.py), whose multiset is the dense reference's; the diamond count is sum C(t, 2) of the dense supports"""
    import torch

    from graphminer_amd.solvers import diamond_support_partial, diamond_support_size

    def supports(s, world):
        n = diamond_support_size(s, world)
        bufs = [torch.full((n,), 5, dtype=torch.int32, device=f"cuda:{dev}") for _ in range(world)]
        for r in range(world):
            diamond_support_partial(s, bufs[r].data_ptr(), n, rank=r, world=world)
        return torch.stack(bufs).sum(0, dtype=torch.int64)

    g, ref = DG.cell("stage"), DG.reference("stage")
    t = ref["sup"].astype(np.int64)
    with g.to_device(dev) as sym:
        one = supports(sym, 1)
        for world in (2, 3):
            diff = int((supports(sym, world)[: one.numel()] != one).sum())
            print(f"stage cell world {world}: {diff} of {one.numel()} entries differ from the one-rank array", flush=True)
            assert diff == 0, world
        got = np.sort(one.cpu().numpy()[: g.E() // 2])  # one entry per undirected edge, in the DAG's order: compared as a multiset
        src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
        check_arrays("stage cell one-rank supports, sorted", got, np.sort(t[src < g.col_idx]))
        check("stage cell diamond", SglSolver(sym, "diamond"), int((t * (t - 1) // 2).sum()) // 2)


def test_support_beyond_16_bits(dev):
    n = 70000
    g = T.graph("book", (n,))
    with g.to_device(dev) as sym:
        total, tv, sup = tc_local(sym)
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    spine = (src < 2) & (g.col_idx < 2)
    check(f"B_{n} spine", sup[spine].tolist(), [n, n])
    check(f"B_{n} pages", np.unique(sup[~spine]).tolist(), [1])
    check(f"B_{n} T_v", (tv[:2].tolist(), np.unique(tv[2:]).tolist()), ([n, n], [1]))
    check(f"B_{n} total", total, n)


def test_hub_corner(dev, devopt):
    """the set-up of tests/test_gpu_supcorner.py: the supports of the last 512 vertices' edges come from the matrix cores"""
    devopt("GM_TOPO_MIN_ROW", "0")
    devopt("GM_SUP_CORE_H", "512")
    name = "rmat10_ef16_s42"
    want_sup, want_tv = ref(name)
    with load_graph(name).to_device(dev) as sym:  # (a fresh handle: the options are read when its tables are built)
        total, tv, sup = tc_local(sym)
        info = (C.c_int64 * 4)()
        _lib.check(_lib.load().gm_sup_core_info(sym.handle, info), "gm_sup_core_info")
        check("corner vertices", int(info[0]), 512)
        assert int(info[1]) > 0
        check_arrays("corner supports", sup, want_sup)
        check_arrays("corner T_v", tv, want_tv)
        check("corner total", total, GOLDEN[name]["motif3"][1])
        check("diamond on the same handle", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])


@pytest.mark.parametrize("family,params,seed", [("split", (6, 5), 3), ("multipartite", (4, 7), 11), ("book", (90,), 5)])
def test_shuffled_numbering(dev, family, params, seed):
    g = T.graph(family, params, order="random", seed=seed)
    assert not np.array_equal(T.numbering(*T.pairs(family, params), "random", seed), np.arange(g.V()))
    want_sup, want_tv = TR.supports(g), TR.vertex_triangles(g)
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            total, tv, sup = tc_local(sym, tune=tune)
            check_arrays(f"{family}{params} shuffled tune={tune} supports", sup, want_sup)
            check_arrays(f"{family}{params} shuffled tune={tune} T_v", tv, want_tv)
            check(f"{family}{params} total", total, int(want_tv.sum()) // 3)


def test_other_solvers_keep_their_results(dev):
    name = "rmat10_ef16_s42"
    want_sup, _ = ref(name)
    with load_graph(name).to_device(dev) as sym:
        check("diamond before", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
        check("hourglass before", SglSolver(sym, "hourglass"), SGL5[name]["hourglass"])
        check_arrays("supports between", tc_local(sym)[2], want_sup)
        check("diamond after", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
        check("hourglass after", SglSolver(sym, "hourglass"), SGL5[name]["hourglass"])
        check_arrays("supports after", tc_local(sym)[2], want_sup)
    with load_graph(name).to_device(dev) as sym:  # the local counts first on a fresh handle
        check_arrays("supports first", tc_local(sym)[2], want_sup)
        check("diamond after a first tc_local", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])


def test_refusals_and_the_empty_graph(dev):
    import torch

    from graphminer_amd import Graph

    lib = _lib.load()
    total = C.c_uint64(5)
    with load_graph("citeseer").to_device(dev) as sym:
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("world = 2", lib.gm_tc_local(sym.handle, C.byref(la), None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        buf = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = buf.data_ptr()
        check("d_counts", lib.gm_tc_local(sym.handle, C.byref(la), None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        total, tv, sup = tc_local(sym)
        check("no edges", (total, tv.tolist(), sup.tolist()), (0, [0, 0, 0], []))
