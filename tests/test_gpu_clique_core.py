"""k-clique cores on the GPU (gm_clique_kcore / gm_clique_core_decompose, csrc/gm_kcl_core.hip) against the plain Python rounds of
tests/clique_core_ref.py and the closed forms of tests/core_gadgets.py: per vertex, with the rounds, the densest state and the clique
totals -- on the five small graphs, on the shapes where a CONCURRENT round goes wrong (a whole clique in one frontier, two adjacent
frontier vertices over shared survivors, tens of thousands of decrements on one counter), and with a hub whose surviving neighbourhood
lies on both sides of every length at which the peel kernel changes path.  Every value is printed before it is asserted."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

import clique_core_ref as R
import core_gadgets as G
import truss_ref as TR
import twin_graphs as T
from common import kcl_row_constants, load_graph
from graphminer_amd import Graph, SglSolver, _lib, clique_core_decompose, clique_kcore, clique_local, ktruss
from graphminer_amd._lib import dev_live_blocks
from graphminer_amd.rmat import csr_from_pairs

pytestmark = pytest.mark.gpu
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
REMOVED = R.REMOVED
AS_NUMBERED = [0, 0, 0, 0, 0, 0, 0x200]  # tune[6] & GM_T6_AS_NUMBERED


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_arrays(label, got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got != want) if got.shape == want.shape else np.zeros(0, np.int64)
    print(f"{label}: {want.shape} values, {bad.size} differ, first at {bad[:5].tolist()}: got {got[bad[:5]].tolist()} "
          f"want {want[bad[:5]].tolist()}", flush=True)
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, label


@functools.lru_cache(maxsize=None)
def ref_decompose(name, k):
    return R.decompose(load_graph(name), k)


def check_decompose(label, sym, k, want, **kw):
    core, rnd, c_max, rounds, dense, st = clique_core_decompose(sym, k, return_stats=True, **kw)
    check_arrays(f"{label} k={k} core numbers", core, want.core)
    check_arrays(f"{label} k={k} rounds per vertex", rnd, want.round)
    check(f"{label} k={k} c_max", c_max, want.c_max)
    check(f"{label} k={k} c_max against the core numbers", c_max, int(core.max()) if core.size else 0)
    check(f"{label} k={k} rounds", rounds, want.rounds)
    check(f"{label} k={k} dense (round, vertices, cliques)", dense, want.dense)
    assert rounds >= 1 and st.tasks == sym.ne
    return core, rnd, c_max, rounds, dense


def check_kcore(label, sym, k, c, want, **kw):
    """want = (per vertex, vertices, cliques, rounds)"""
    nvert, ncl, cnt, rounds, st = clique_kcore(sym, k, c, return_stats=True, **kw)
    check_arrays(f"{label} k={k} c={c} per vertex", cnt, want[0])
    check(f"{label} k={k} c={c} (vertices, cliques, rounds)", (nvert, ncl, rounds), tuple(want[1:]))
    inside = cnt != REMOVED
    check(f"{label} k={k} c={c} cliques x k against the counts inside", ncl * k, sum(int(x) for x in cnt[inside]))
    check(f"{label} k={k} c={c} vertices against the counts", nvert, int(inside.sum()))
    assert rounds >= 1 and st.tasks == sym.ne
    return cnt


def induced(g, keep):
    """the subgraph of g induced by the vertices keep[v], renumbered in order"""
    newid = np.cumsum(keep) - 1
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    dst = np.asarray(g.col_idx).astype(np.int64)
    sel = keep[src] & keep[dst] & (src < dst)
    return csr_from_pairs(int(keep.sum()), newid[src[sel]].astype(np.uint64), newid[dst[sel]].astype(np.uint64))


# ---- 1. the decomposition on the small graphs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(n, k) for n in SMALL for k in (2, 3, 4)] + [(n, 5) for n in SMALL[:4]])
def test_decompose_small_graphs(dev, name, k):
    g = load_graph(name)
    with g.to_device(dev) as sym:
        core, rnd, c_max, rounds, dense = check_decompose(name, sym, k, ref_decompose(name, k))
    if (name, k) == ("citeseer", 3):
        check("citeseer k=3 (c_max, rounds, dense vertices, dense triangles)", (c_max, rounds) + dense[1:], (12, 52, 15, 113))
        sub = induced(g, rnd >= dense[0])
        with sub.to_device(dev) as s2:
            check("the dense set's cliques against gm_clique_local on the induced subgraph", clique_local(s2, 3, entries=False)[0], dense[2])


# ---- 2. the (k, c)-core ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(n, k) for n in ("citeseer", "rmat8_ef8_s42") for k in (3, 4)])
def test_kcore_small_graphs(dev, name, k):
    g = load_graph(name)
    d = ref_decompose(name, k)
    positive = np.unique(d.core[d.core > 0])
    middle = int(positive[positive.size // 2])
    with g.to_device(dev) as sym:
        for c in (0, 1, middle, d.c_max, d.c_max + 1):
            cnt = check_kcore(name, sym, k, c, R.kcore(g, k, c))
            check_arrays(f"{name} k={k} c={c} the core is the vertices of core number >= c", cnt != REMOVED, d.core >= c)
        check(f"{name} k={k} the ({k}, c_max + 1)-core is empty", int((cnt != REMOVED).sum()), 0)


# ---- 3. shapes where a concurrent round goes wrong ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(5, 3), (65, 3), (130, 3), (65, 4), (20, 8)])
def test_whole_clique_in_one_frontier(dev, n, k):
    """K_n: every vertex is in the frontier, S_v runs through every length from n - 1 down to 0, nobody survives to take a decrement, and the
    destroyed total must land on C(n, k) exactly"""
    g = T.graph("complete", (n,))
    each = comb(n - 1, k - 1)
    want = R.Decomposition(np.full(n, each, np.uint64), np.ones(n, np.uint32), each, 2, [(n, comb(n, k)), (0, 0)], (1, n, comb(n, k)))
    with g.to_device(dev) as sym:
        check_decompose(f"K_{n}", sym, k, want)
        check_kcore(f"K_{n}", sym, k, each, (np.full(n, each, np.uint64), n, comb(n, k), 1))
        check_kcore(f"K_{n}", sym, k, each + 1, (np.full(n, REMOVED, np.uint64), 0, 0, 2))


def test_two_adjacent_frontier_vertices_over_shared_survivors(dev):
    """the small two-hub gadget: the cliques that hold both hubs must be taken once"""
    a, p, m, seed = 12, 0.4, 10, 12
    for k in (3, 4):
        want = G.expected(a, p, m, seed, k, hubs=2)
        g = G.hub_gadget(a, p, m, seed, hubs=2)
        check(f"two hubs a={a} k={k} closed forms against the plain reference", R.kcore(g, k, want["c"])[1:], (want["vertices"], want["cliques"], 2))
        with g.to_device(dev) as sym:
            check_kcore(f"two hubs a={a}", sym, k, want["c"], (want["cnt"], want["vertices"], want["cliques"], want["rounds"]))
            check_decompose(f"two hubs a={a}", sym, k, R.decompose(g, k))


def test_many_decrements_on_one_counter_windmill(dev):
    """35,000 triangles on one centre, k = 3: as many waves take one each from the centre's counter in round 1, the centre leaves in round 2"""
    t = 35000
    g = G.windmill(t)
    with g.to_device(dev) as sym:
        core, rnd, c_max, rounds, dense = clique_core_decompose(sym, 3)
        check("windmill (core numbers, c_max, rounds)", (np.unique(core).tolist(), c_max, rounds), ([1], 1, 3))
        check("windmill rounds per vertex", (int(rnd[0]), np.unique(rnd[1:]).tolist()), (2, [1]))
        check("windmill dense", dense, (1, 2 * t + 1, t))
        nvert, ncl, cnt, rounds = clique_kcore(sym, 3, 1)
        check("windmill (3, 1)-core", (nvert, ncl, int(cnt[0]), np.unique(cnt[1:]).tolist(), rounds), (2 * t + 1, t, t, [1], 1))
        nvert, ncl, cnt, rounds = clique_kcore(sym, 3, 2)
        check("windmill (3, 2)-core", (nvert, ncl, np.unique(cnt).tolist(), rounds), (0, 0, [REMOVED], 3))


def test_many_decrements_on_one_counter_star(dev):
    """k = 2 on a star of 70,000 leaves: 70,000 decrements on the centre's degree"""
    n = 70000
    g = G.star(n)
    with g.to_device(dev) as sym:
        core, rnd, c_max, rounds, dense = clique_core_decompose(sym, 2)
        check("star (core numbers, c_max, rounds)", (np.unique(core).tolist(), c_max, rounds), ([1], 1, 3))
        check("star rounds per vertex", (int(rnd[0]), np.unique(rnd[1:]).tolist()), (2, [1]))
        check("star dense", dense, (1, n + 1, n))
        nvert, ncl, cnt, rounds = clique_kcore(sym, 2, 2)
        check("star 2-core", (nvert, ncl, np.unique(cnt).tolist(), rounds), (0, 0, [REMOVED], 3))


# ---- 4. path cells: a hub of `a` survivors on both sides of every boundary ----------------------------------------------------------------
def gadget_cells():
    """(a, p, m) by the boundary the hub's |S_v| = a lies at: both sides of each, and one past a word per lane of the wide kernel"""
    rc = kcl_row_constants()
    density = {"regs2": (0.2, 40), "regs8": (0.1, 100), "regs12": (0.07, 120), "lds": (0.05, 120)}
    cells = []
    for key, (p, m) in density.items():
        cells += [(rc[key], p, m), (rc[key] + 1, p, m)]
    return cells + [(rc["lanes"] + 1, 0.005, 150)], rc


def run_gadget(dev, a, p, m, k, hubs=1):
    want = G.expected(a, p, m, a, k, hubs)  # (asserts that the hubs leave alone and that A + Z survives, from the closed forms)
    check(f"a={a} k={k} hubs={hubs}: at least three different decrements", len(want["decrements"]) >= 3, True)
    g = G.hub_gadget(a, p, m, a, hubs)
    with g.to_device(dev) as sym:
        check_kcore(f"gadget a={a} hubs={hubs}", sym, k, want["c"], (want["cnt"], want["vertices"], want["cliques"], want["rounds"]))


@pytest.mark.parametrize("k", [3, 4])
def test_hub_gadget_at_every_boundary(dev, k):
    cells, rc = gadget_cells()
    check("the boundaries", (rc["regs2"], rc["regs8"], rc["regs12"], rc["lds"], rc["lanes"]), (64, 256, 384, 512, 2048))
    for a, p, m in cells:
        run_gadget(dev, a, p, m, k)


@pytest.mark.parametrize("k", [5, 6])
def test_hub_gadget_deeper_descents(dev, k):
    rc = kcl_row_constants()
    for a, p, m in ((rc["regs2"] + 1, 0.3, 40), (rc["regs8"] + 1, 0.15, 60)):
        run_gadget(dev, a, p, m, k)


def test_two_hub_gadget_on_the_workgroup_and_wide_paths(dev):
    rc = kcl_row_constants()
    for a, p, m in ((rc["regs2"] + 1, 0.2, 40), (rc["lds"] + 1, 0.05, 120)):
        run_gadget(dev, a, p, m, 3, hubs=2)


# ---- 5. the contract -----------------------------------------------------------------------------------------------------------------------
def raw_kcore(sym, k, c, la=None, buf=None):
    n, m, rounds = C.c_uint64(5), C.c_uint64(5), C.c_int32(5)
    rc = _lib.load().gm_clique_kcore(sym.handle if sym is not None else None, k, c, C.byref(la) if la is not None else None,
                                     buf.data_ptr() if buf is not None else None, C.byref(n), C.byref(m), C.byref(rounds), None)
    return rc, int(n.value), int(m.value), int(rounds.value)


def raw_decompose(sym, k, la=None, core=None, rnd=None):
    cmax, rounds, dense = C.c_uint64(5), C.c_int32(5), _lib.gm_core_dense()
    rc = _lib.load().gm_clique_core_decompose(sym.handle if sym is not None else None, k, C.byref(la) if la is not None else None,
                                              core.data_ptr() if core is not None else None, rnd.data_ptr() if rnd is not None else None,
                                              C.byref(cmax), C.byref(rounds), C.byref(dense), None)
    return rc, int(cmax.value), int(rounds.value)


def test_refusals(dev, devopt):
    import torch

    g = load_graph("citeseer")
    buf = torch.zeros(g.V(), dtype=torch.int64, device=f"cuda:{dev}")
    check("kcore, a null handle", raw_kcore(None, 3, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
    check("decompose, a null handle", raw_decompose(None, 3, core=buf)[0], _lib.GM_ERR_INVALID)
    with g.to_device(dev) as sym:
        for k in (-1, 0, 1, 13, 100):
            check(f"kcore k = {k}", raw_kcore(sym, k, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
            check(f"decompose k = {k}", raw_decompose(sym, k, core=buf)[0], _lib.GM_ERR_INVALID)
        for k in (9, 12):
            check(f"kcore k = {k}", raw_kcore(sym, k, 1, buf=buf)[0], _lib.GM_ERR_UNSUPPORTED)
            check(f"decompose k = {k}", raw_decompose(sym, k, core=buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose without a core array", raw_decompose(sym, 3)[0], _lib.GM_ERR_INVALID)
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("kcore world = 2", raw_kcore(sym, 3, 1, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose world = 2", raw_decompose(sym, 3, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        counts = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = counts.data_ptr()
        check("kcore d_counts", raw_kcore(sym, 3, 1, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose d_counts", raw_decompose(sym, 3, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("nothing was written", bool((buf.cpu().numpy() == 0).all()), True)
        # the arrays may be left out: the numbers alone
        want = R.kcore(g, 3, 2)
        check("kcore without an array", raw_kcore(sym, 3, 2), (_lib.GM_OK,) + tuple(want[1:]))
        check("decompose without a round array", raw_decompose(sym, 3, core=buf), (_lib.GM_OK, 12, 52))
        check_arrays("... its core numbers", buf.cpu().numpy().view(np.uint64), ref_decompose("citeseer", 3).core)
    devopt("GM_BIG_NE", "1")  # a handle of "2^31 entries or more" (the developer option gives a small graph such a handle)
    big = g.to_device(dev)
    devopt("GM_BIG_NE", None)
    with big:
        check("kcore, a big handle", raw_kcore(big, 3, 1, buf=buf)[0], _lib.GM_ERR_TOO_LARGE)
        check("decompose, a big handle", raw_decompose(big, 3, core=buf)[0], _lib.GM_ERR_TOO_LARGE)
    rev = g.col_idx.copy()
    for v in range(g.V()):
        a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
        rev[a:b] = rev[a:b][::-1]
    with Graph(row_ptr=g.row_ptr.copy(), col_idx=rev, name="citeseer_descending").to_device(dev) as sym:
        check("kcore, unsorted rows", raw_kcore(sym, 3, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
        assert b"ascending" in _lib.load().gm_last_error()
        check("decompose, unsorted rows", raw_decompose(sym, 2, core=buf)[0], _lib.GM_ERR_INVALID)


def test_graphs_without_edges_and_isolated_vertices(dev):
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        for k in (2, 3):
            core, rnd, c_max, rounds, dense = clique_core_decompose(sym, k)
            check(f"no edges k={k}", (core.tolist(), rnd.tolist(), c_max, rounds, dense), ([0, 0, 0], [1, 1, 1], 0, 2, (1, 3, 0)))
            check(f"no edges k={k} c=0", (lambda r: (r[0], r[1], r[2].tolist(), r[3]))(clique_kcore(sym, k, 0)), (3, 0, [0, 0, 0], 1))
            check(f"no edges k={k} c=1", (lambda r: (r[0], r[1], r[2].tolist(), r[3]))(clique_kcore(sym, k, 1)), (0, 0, [REMOVED] * 3, 2))
    # vertices 0 and 4 are isolated, 1-2-3 is a triangle
    g = csr_from_pairs(5, np.array([1, 1, 2], dtype=np.uint64), np.array([2, 3, 3], dtype=np.uint64))
    with g.to_device(dev) as sym:
        for k, inner in ((2, 2), (3, 1)):
            core, rnd, c_max, rounds, dense = check_decompose("triangle + 2 isolated", sym, k, R.decompose(g, k))
            check(f"triangle + 2 isolated k={k}", (core.tolist(), rnd.tolist(), c_max, rounds), ([0, inner, inner, inner, 0], [1, 3, 3, 3, 1], inner, 4))
            check_kcore("triangle + 2 isolated", sym, k, 1, R.kcore(g, k, 1))
        check("a 4-clique core of a triangle", clique_core_decompose(sym, 4)[2:], (0, 2, (1, 5, 0)))


def test_beside_other_solvers_and_twice(dev):
    """before and after gm_sgl("diamond"), gm_clique_local and gm_ktruss on the same handle, whose results do not change; two calls in a row
    and a call on the graph as numbered give identical arrays"""
    name, k = "rmat8_ef8_s42", 4
    g = load_graph(name)
    want = ref_decompose(name, k)
    with g.to_device(dev) as sym:
        first = check_decompose(name + " on a fresh handle", sym, k, want)
        others = (SglSolver(sym, "diamond"), clique_local(sym, k), ktruss(sym, 4))
        again = check_decompose(name + " after the other solvers", sym, k, want)
        for x, y in zip(first[:2], again[:2]):
            check_arrays("two calls, identical arrays", x, y)
        numbered = check_decompose(name + " as numbered", sym, k, want, tune=AS_NUMBERED)
        check_arrays("as numbered, identical core numbers", numbered[0], first[0])
        check_arrays("as numbered, identical rounds", numbered[1], first[1])
        mid = int(np.unique(want.core)[-2])
        a = check_kcore(name, sym, k, mid, R.kcore(g, k, mid))
        b = check_kcore(name + " as numbered", sym, k, mid, R.kcore(g, k, mid), tune=AS_NUMBERED)
        check_arrays("kcore twice, identical arrays", a, b)
        after = (SglSolver(sym, "diamond"), clique_local(sym, k), ktruss(sym, 4))
        check("diamond unchanged", after[0], others[0])
        check("gm_clique_local total unchanged", after[1][0], others[1][0])
        check_arrays("gm_clique_local per vertex unchanged", after[1][1], others[1][1])
        check_arrays("gm_clique_local per entry unchanged", after[1][2], others[1][2])
        check("gm_ktruss unchanged", (after[2][0], after[2][2]), (others[2][0], others[2][2]))
        check_arrays("gm_ktruss per entry unchanged", after[2][1], others[2][1])
        check_arrays("gm_ktruss against its reference", after[2][1], TR.ktruss(g, 4)[0])
        check_decompose(name + " k=2 on the same handle", sym, 2, ref_decompose(name, 2))


def test_every_block_goes_back_with_the_handle(dev):
    a, p, m = kcl_row_constants()["lds"] + 1, 0.05, 120  # (the wide path: the heavy list and the scratch slots are allocated too)
    g = G.hub_gadget(a, p, m, a)
    want = G.expected(a, p, m, a, 3)
    before = dev_live_blocks()
    sym = g.to_device(dev)
    assert dev_live_blocks() > before
    for _ in range(2):
        check_kcore("gadget", sym, 3, want["c"], (want["cnt"], want["vertices"], want["cliques"], want["rounds"]))
        clique_core_decompose(sym, 2)
    sym.free()
    check("live device blocks after the handle is freed", dev_live_blocks(), before)
