"""k-clique trusses on the GPU (gm_clique_ktruss / gm_clique_truss_decompose, csrc/gm_kcl_truss.hip) against the plain Python rounds of
tests/clique_truss_ref.py, the existing k-truss at k = 3 and the closed forms of tests/truss_gadgets.py: per entry, with the rounds and the
clique totals -- on the five small graphs, on the shapes where a CONCURRENT round goes wrong (a whole clique in one frontier, two frontier
edges over shared survivors, two disjoint frontier edges of one 4-clique, tens of thousands of decrements on one counter), and with a hub
edge whose surviving common neighbours lie on both sides of every length at which the peel kernel changes path.  The blocked cells
(DESIGN.md "k-clique trusses: blocked cells") put blocked spokes and blocked pairs on the workgroup path and in the wide kernel: K_n one
past every boundary, the split gadget, three hubs in a triangle, matrix rows of more than 64 words, rows longer than four lists.  Every
value is printed before it is asserted."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

import clique_truss_ref as R
import truss_gadgets as G
import truss_ref as TR
import twin_graphs as T
from common import kcl_row_constants, load_graph
from graphminer_amd import (Graph, SglSolver, _lib, clique_kcore, clique_ktruss, clique_local, clique_truss_decompose, ktruss, truss_decompose)
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


def endpoints(g):
    return np.repeat(np.arange(g.V(), dtype=np.int64), np.diff(g.row_ptr)), np.asarray(g.col_idx).astype(np.int64)


def reverse_entries(g):
    """per entry (u, v) the index of (v, u)"""
    src, dst = endpoints(g)
    order = np.lexsort((src, dst))  # the entries sorted by (dst, src): the i-th of them is the reverse of entry i
    return order


def check_both_directions(label, g, arr):
    check(f"{label}: both directions of every edge equal", bool(np.array_equal(arr, arr[reverse_entries(g)])), True)


@functools.lru_cache(maxsize=None)
def ref_decompose(name, k):
    return R.decompose(load_graph(name), k)


def check_decompose(label, g, sym, k, want, **kw):
    theta, rnd, c_max, rounds, st = clique_truss_decompose(sym, k, return_stats=True, **kw)
    check_arrays(f"{label} k={k} theta", theta, want.theta)
    check_arrays(f"{label} k={k} rounds per entry", rnd, want.round)
    check(f"{label} k={k} c_max", c_max, want.c_max)
    check(f"{label} k={k} c_max against theta", c_max, int(theta.max()) if theta.size else 0)
    check(f"{label} k={k} rounds", rounds, want.rounds)
    check_both_directions(f"{label} k={k} theta", g, theta)
    check_both_directions(f"{label} k={k} round", g, rnd)
    assert rounds >= 1 and st.tasks == sym.ne
    return theta, rnd, c_max, rounds


def check_ktruss(label, g, sym, k, c, want, **kw):
    """want = (per entry, edges, cliques, rounds)"""
    edges, ncl, cnt, rounds, st = clique_ktruss(sym, k, c, return_stats=True, **kw)
    check_arrays(f"{label} k={k} c={c} per entry", cnt, want[0])
    check(f"{label} k={k} c={c} (edges, cliques, rounds)", (edges, ncl, rounds), tuple(want[1:]))
    inside = cnt != REMOVED
    check(f"{label} k={k} c={c} cliques x C(k, 2) against the counts inside", ncl * comb(k, 2) * 2, sum(int(x) for x in cnt[inside]))
    check(f"{label} k={k} c={c} edges against the counts", 2 * edges, int(inside.sum()))
    check_both_directions(f"{label} k={k} c={c}", g, cnt)
    assert rounds >= 1 and st.tasks == sym.ne
    return cnt


def edge_subgraph(g, keep):
    """the graph of the entries keep[e] of g, on the same vertices: its entries are g's kept entries, in g's order"""
    src, dst = endpoints(g)
    sel = keep & (src < dst)
    return csr_from_pairs(g.V(), src[sel].astype(np.uint64), dst[sel].astype(np.uint64))


# ---- 1. the decomposition on the small graphs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(n, k) for n in SMALL for k in (3, 4)] + [(n, 5) for n in SMALL[:4]])
def test_decompose_small_graphs(dev, name, k):
    g = load_graph(name)
    with g.to_device(dev) as sym:
        check_decompose(name, g, sym, k, ref_decompose(name, k))


# ---- 2. k = 3 against the existing k-truss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_k3_is_the_ordinary_truss(dev, name):
    g = load_graph(name)
    with g.to_device(dev) as sym:
        tau, k_max, _ = truss_decompose(sym)
        theta, _, c_max, _ = clique_truss_decompose(sym, 3)
        check_arrays(f"{name} theta + 2 against gm_truss_decompose", theta + np.uint64(2), tau.astype(np.uint64))
        check(f"{name} c_max + 2 against k_max", c_max + 2, k_max)
        for c in (1, max(1, c_max // 2), c_max):
            edges3, sup, rounds3 = ktruss(sym, c + 2)
            edges, ncl, cnt, rounds = clique_ktruss(sym, 3, c)
            wide = np.where(sup == TR.REMOVED, REMOVED, sup.astype(np.uint64)).astype(np.uint64)
            check_arrays(f"{name} c={c} against gm_ktruss({c + 2}) widened", cnt, wide)
            check(f"{name} c={c} (edges, rounds) against gm_ktruss", (edges, rounds), (edges3, rounds3))


# ---- 3. the (k, c)-truss ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(n, k) for n in ("citeseer", "rmat8_ef8_s42") for k in (3, 4)])
def test_ktruss_small_graphs(dev, name, k):
    g = load_graph(name)
    d = ref_decompose(name, k)
    positive = np.unique(d.theta[d.theta > 0])
    middle = int(positive[positive.size // 2])
    with g.to_device(dev) as sym:
        for c in (0, 1, middle, d.c_max, d.c_max + 1):
            cnt = check_ktruss(name, g, sym, k, c, R.ktruss(g, k, c))
            inside = cnt != REMOVED
            check_arrays(f"{name} k={k} c={c} the truss is the edges of theta >= c", inside, d.theta >= c)
            if inside.any():
                with edge_subgraph(g, inside).to_device(dev) as sub:
                    total, _, ent = clique_local(sub, k, vertex=False)
                check_arrays(f"{name} k={k} c={c} the counts against gm_clique_local on the surviving edges", cnt[inside], ent)
        check(f"{name} k={k} the ({k}, c_max + 1)-truss is empty", int(inside.sum()), 0)


# ---- 4. shapes where a concurrent round goes wrong ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(5, 3), (65, 3), (65, 4), (20, 8)] + [(key, 3) for key in ("regs2", "regs8", "regs12", "lds")] +
                         [(key, 4) for key in ("regs2", "regs8", "regs12", "lds")])
def test_whole_clique_in_one_frontier(dev, n, k):
    """K_n: every edge is in the frontier, S_e runs through every length from n - 2 down to 0, nobody survives to take a decrement, and the
    destroyed total must land on C(n, k) exactly (the call checks it).  The survivors of (u, v) are the ids above v: every spoke to a lower
    id is blocked, so the blocked entries are the low ids of the streamed row, on every path n - 2 reaches.  n = a boundary's name: n - 2,
    the longest S_e, lies one past it"""
    if isinstance(n, str):
        key, n = n, kcl_row_constants()[n] + 3
        check(f"K_{n}: the longest S_e, one past {key}", n - 2, kcl_row_constants()[key] + 1)
    g = T.graph("complete", (n,))
    each, ne = comb(n - 2, k - 2), n * (n - 1)
    want = R.Decomposition(np.full(ne, each, np.uint64), np.ones(ne, np.uint32), each, 2)
    with g.to_device(dev) as sym:
        check_decompose(f"K_{n}", g, sym, k, want)
        check_ktruss(f"K_{n}", g, sym, k, each, (np.full(ne, each, np.uint64), ne // 2, comb(n, k), 1))
        check_ktruss(f"K_{n}", g, sym, k, each + 1, (np.full(ne, REMOVED, np.uint64), 0, 0, 2))


def test_two_frontier_edges_sharing_a_vertex_over_shared_survivors(dev):
    """the gadget with three hubs: (h1, h2) and (h1, h3) leave in the same round, and every spoke (h1, w) takes from both"""
    a, p, seed = 12, 0.4, 12
    for k in (3, 4):
        m = G.booster(a, p, seed, k)
        g = G.hub_edge_gadget(a, p, m, seed, hubs=3)
        c = G.expected(G.hub_edge_gadget(a, p, m, seed), a, p, m, seed, k)["c"]
        want = R.ktruss(g, k, c)
        gone = np.flatnonzero(want[0] == REMOVED)
        src, dst = endpoints(g)
        h1 = a + 3 * m
        check(f"k={k}: the reference removes the two hub edges, in one round", (sorted(zip(src[gone].tolist(), dst[gone].tolist())), want[3]),
              ([(h1, h1 + 1), (h1, h1 + 2), (h1 + 1, h1), (h1 + 2, h1)], 2))
        with g.to_device(dev) as sym:
            check_ktruss(f"three hubs a={a}", g, sym, k, c, want)
            check_decompose(f"three hubs a={a}", g, sym, k, R.decompose(g, k))


TRIANGLE_IDS = ["regs2-k3", "regs2-k4", "lds-k3", "lds-k4"]


@pytest.mark.parametrize("cell", range(len(TRIANGLE_IDS)), ids=TRIANGLE_IDS)
def test_three_hubs_in_a_triangle_on_the_long_paths(dev, cell):
    """the three-hub gadget with the edge (h2, h3): three frontier edges over the same a survivors.  (h1, h2), the lowest entry, keeps h3 --
    a + 1 survivors, the cliques with two or three hubs are its own --; for (h1, h3) and (h2, h3) the spoke to the third hub is blocked, at
    the END of the streamed row, behind a kept entries.  The closed forms (tests/test_clique_truss_host.py holds them against the reference
    at a = 12); on the workgroup path the reference itself too"""
    rc = kcl_row_constants()
    a, p, k = G.triangle_cells(rc)[cell]
    check(f"{TRIANGLE_IDS[cell]}: a one past the boundary", a, rc[TRIANGLE_IDS[cell].split("-")[0]] + 1)
    m = G.booster(a, p, a, k, 3, True)
    g = G.hub_edge_gadget(a, p, m, a, 3, True)
    exp = G.expected(g, a, p, m, a, k, 3, True)
    src, dst = endpoints(g)
    gone = np.flatnonzero(exp["cnt"] == REMOVED)
    h1 = a + 3 * m
    check(f"a={a} k={k}: the three hub edges leave", sorted(zip(src[gone].tolist(), dst[gone].tolist())),
          sorted((h1 + i, h1 + j) for i in range(3) for j in range(3) if i != j))
    check(f"a={a} k={k}: the hubs' rows end with the other hubs", [g.col_idx[g.row_ptr[h + 1] - 1] for h in (h1, h1 + 1, h1 + 2)], [h1 + 2, h1 + 2, h1 + 1])
    want = (exp["cnt"], exp["edges"], exp["cliques"], exp["rounds"])
    if a <= rc["regs2"] + 1:
        ref = R.ktruss(g, k, exp["c"])
        check_arrays(f"a={a} k={k}: the closed forms against the reference", want[0], ref[0])
        check(f"a={a} k={k}: (edges, cliques, rounds) against the reference", want[1:], tuple(ref[1:]))
    with g.to_device(dev) as sym:
        check_ktruss(f"hubs in a triangle a={a} m={m}", g, sym, k, exp["c"], want)
        if a <= rc["regs2"] + 1:
            check_decompose(f"hubs in a triangle a={a} m={m}", g, sym, k, R.decompose(g, k))


SPLIT_IDS = ["regs2-k4", "regs2-k5", "regs8-k4", "regs12-k4", "lds-k4"]
SPLIT_DECOMPOSE = ("regs2-k4", "regs2-k5")  # (where the plain reference finishes in seconds)


@pytest.mark.parametrize("cell", range(len(SPLIT_IDS)), ids=SPLIT_IDS)
def test_split_gadget_blocked_pairs_inside_a_long_list(dev, cell):
    """the hub edge e with the edges X ACROSS the two halves of its survivors in the same frontier, at lower entries, all four spokes of each
    alive: the cliques {w, x, h1, h2, ..} are the account of (w, x), and from e only the pair filter of the matrix hides them -- the
    workgroup path's ktr_build_msym in three register widths and the wide kernel's own build.  Exactly e and X leave, in two rounds; what
    stays has its count in G' = G - e - X, by the closed forms per half and by gm_clique_local on the surviving edges"""
    rc = kcl_row_constants()
    a, p, q, k = G.split_cells(rc)[cell]
    check(f"{SPLIT_IDS[cell]}: a one past the boundary, k", (a, k), (rc[SPLIT_IDS[cell].split("-")[0]] + 1, int(SPLIT_IDS[cell][-1])))
    m = G.split_booster(a, p, q, a, k)
    g = G.split_hub_edge_gadget(a, p, q, m, a)
    want = G.split_expected(g, a, p, q, m, a, k)  # (asserts, from the closed forms: X below c, everything else of G' at or above it)
    check(f"a={a} k={k}: X has at least 8 edges, one of them over the first and the last word of a row",
          (want["x"] >= 8, want["x_words"]), (True, (0, want["words"] - 1)))
    check(f"a={a} k={k}: at least three different spoke decrements", len(want["spoke_decrements"]) >= 3, True)
    with g.to_device(dev) as sym:
        cnt = check_ktruss(f"split gadget a={a} m={m}", g, sym, k, want["c"], (want["cnt"], want["edges"], want["cliques"], want["rounds"]))
        inside = cnt != REMOVED
        check(f"a={a} k={k}: e and X are what left", int((~inside).sum()), 2 * (want["x"] + 1))
        with edge_subgraph(g, inside).to_device(dev) as sub:
            _, _, ent = clique_local(sub, k, vertex=False)
        check_arrays(f"split gadget a={a} k={k} the counts against gm_clique_local on the surviving edges", cnt[inside], ent)
        if SPLIT_IDS[cell] in SPLIT_DECOMPOSE:
            check_decompose(f"split gadget a={a} m={m}", g, sym, k, R.decompose(g, k))


def test_two_disjoint_frontier_edges_of_one_4_clique(dev):
    """{0, 1, 2, 3} is a 4-clique whose other four edges each lie in a K_6 of their own: at k = 4 and c = 2 the frontier of round 1 is (0, 1)
    and (2, 3).  (0, 1) accounts the clique; from (2, 3) it must be invisible -- S is {0, 1}, and only the pair filter of the matrix hides it"""
    src, dst, nxt = [0, 2], [1, 3], 4
    for x, y in ((0, 2), (0, 3), (1, 2), (1, 3)):
        ids = [x, y, nxt, nxt + 1, nxt + 2, nxt + 3]
        nxt += 4
        for i in range(6):
            for j in range(i + 1, 6):
                src.append(ids[i])
                dst.append(ids[j])
    g = csr_from_pairs(nxt, np.array(src, dtype=np.uint64), np.array(dst, dtype=np.uint64))
    want = R.ktruss(g, 4, 2)
    gs, gd = endpoints(g)
    gone = np.flatnonzero(want[0] == REMOVED)
    check("the reference: (0, 1) and (2, 3) leave, in one round, and the 4 x 15 + 1 cliques lose one",
          (sorted(zip(gs[gone].tolist(), gd[gone].tolist())), want[2], want[3]), ([(0, 1), (1, 0), (2, 3), (3, 2)], 60, 2))
    check("the reference: the other four edges of the clique keep their K_6", sorted(set(want[0][want[0] != REMOVED].tolist())), [6])
    with g.to_device(dev) as sym:
        check_ktruss("one 4-clique, two frontier edges", g, sym, 4, 2, want)
        check_decompose("one 4-clique, two frontier edges", g, sym, 4, R.decompose(g, 4))
        check_decompose("one 4-clique, two frontier edges", g, sym, 3, R.decompose(g, 3))


@pytest.mark.parametrize("t,k", [(35000, 3), (70000, 3), (35000, 4)])
def test_many_decrements_on_one_counter(dev, t, k):
    """a book of t pages: in round 1 every page leaves and as many waves take one each from the spine's counter; the spine leaves in round 2"""
    g = G.book(t, k)
    with g.to_device(dev) as sym:
        theta, rnd, c_max, rounds = clique_truss_decompose(sym, k)
        check("book (theta, c_max, rounds)", (np.unique(theta).tolist(), c_max, rounds), ([1], 1, 3))
        check("book rounds per entry: the spine and its reverse in round 2", (int(rnd[0]), int((rnd == 2).sum()), int((rnd == 1).sum())), (2, 2, g.E() - 2))
        edges, ncl, cnt, rounds = clique_ktruss(sym, k, 1)
        check(f"book ({k}, 1)-truss", (edges, ncl, int(cnt[0]), np.unique(cnt[1:]).tolist(), rounds), (g.E() // 2, t, t, [1, t], 1))
        edges, ncl, cnt, rounds = clique_ktruss(sym, k, 2)
        check(f"book ({k}, 2)-truss", (edges, ncl, np.unique(cnt).tolist(), rounds), (0, 0, [REMOVED], 3))


# ---- 5. path cells: a hub edge of `a` survivors on both sides of every boundary -------------------------------------------------------------
def gadget_cells():
    """(a, p) by the boundary |S_e| = a lies at: both sides of each; the last one is the wide kernel's"""
    rc = kcl_row_constants()
    density = {"regs2": 0.2, "regs8": 0.1, "regs12": 0.07, "lds": 0.05}
    return [(rc[key] + more, p) for key, p in density.items() for more in (0, 1)] + [(520, 0.05)], rc


def run_gadget(dev, a, p, k, least_m=0, before=None):
    m = max(G.booster(a, p, a, k), least_m)
    g = G.hub_edge_gadget(a, p, m, a)
    if before:
        before(g)
    want = G.expected(g, a, p, m, a, k)  # (asserts that the hub edge leaves alone and that everything else survives, from the closed forms)
    if k >= 4:
        check(f"a={a} k={k}: at least three different spoke decrements", len(want["spoke_decrements"]) >= 3, True)
    with g.to_device(dev) as sym:
        check_ktruss(f"hub-edge gadget a={a} m={m}", g, sym, k, want["c"], (want["cnt"], want["edges"], want["cliques"], want["rounds"]))


@pytest.mark.parametrize("k", [3, 4])
def test_hub_edge_gadget_at_every_boundary(dev, k):
    cells, rc = gadget_cells()
    check("the boundaries", (rc["regs2"], rc["regs8"], rc["regs12"], rc["lds"]), (64, 256, 384, 512))
    for a, p in cells:
        run_gadget(dev, a, p, k)


def test_hub_edge_gadget_deeper_descents(dev):
    """k = 5 and 6: pair decrements that differ, on the wave and the workgroup path"""
    rc = kcl_row_constants()
    for k, a, p in ((5, rc["regs2"], 0.3), (5, rc["regs2"] + 1, 0.3), (6, rc["regs2"] + 1, 0.35)):
        run_gadget(dev, a, p, k)


@pytest.mark.parametrize("cell", [0, 1], ids=["lanes+1", "lanes+65"])
def test_hub_edge_gadget_beyond_the_first_64_words_of_a_row(dev, cell):
    """the wide kernel walks the set pairs of a position through its matrix row 64 words at a time: position `lanes` = 64 x 32 is the first
    of the second group.  At a = lanes + 1 every pair of that position is met from a position of the first group, in its second step; at
    a = lanes + 65 the positions from `lanes` on have pairs among themselves, whose walk STARTS in the second group"""
    rc = kcl_row_constants()
    a, p, k = G.second_group_cells(rc)[cell]
    check("a against lanes", a - rc["lanes"], (1, 65)[cell])
    one, both = G.a_edges_from(a, p, a, rc["lanes"])
    print(f"a={a} p={p}: {one} edges of A reach position {rc['lanes']} or beyond, {both} lie there with both ends", flush=True)
    assert one >= 1 and (cell == 0 or both >= 1)
    run_gadget(dev, a, p, k)


def test_hub_edge_gadget_with_rows_longer_than_four_lists(dev):
    """the workgroup path, every survivor's row longer than 4 |S_e|: the pair walk streams S_e against the row (the other branch of
    ktr_walk_pairs), for the matrix and again for the pair decrements"""
    rc = kcl_row_constants()
    a, p, k, least_m = G.long_row_cell(rc)

    def rows(g):
        shortest = int(np.diff(g.row_ptr)[:a].min())
        print(f"a={a}: the shortest row of a survivor {shortest}, 4 |S_e| = {4 * a}", flush=True)
        assert rc["regs2"] < a <= rc["lds"] and shortest > 4 * a

    run_gadget(dev, a, p, k, least_m, rows)


# ---- 6. the contract -----------------------------------------------------------------------------------------------------------------------
def raw_ktruss(sym, k, c, la=None, buf=None):
    n, m, rounds = C.c_uint64(5), C.c_uint64(5), C.c_int32(5)
    rc = _lib.load().gm_clique_ktruss(sym.handle if sym is not None else None, k, c, C.byref(la) if la is not None else None,
                                      buf.data_ptr() if buf is not None else None, C.byref(n), C.byref(m), C.byref(rounds), None)
    return rc, int(n.value), int(m.value), int(rounds.value)


def raw_decompose(sym, k, la=None, theta=None, rnd=None):
    cmax, rounds = C.c_uint64(5), C.c_int32(5)
    rc = _lib.load().gm_clique_truss_decompose(sym.handle if sym is not None else None, k, C.byref(la) if la is not None else None,
                                               theta.data_ptr() if theta is not None else None, rnd.data_ptr() if rnd is not None else None,
                                               C.byref(cmax), C.byref(rounds), None)
    return rc, int(cmax.value), int(rounds.value)


def test_refusals(dev, devopt):
    import torch

    g = load_graph("citeseer")
    buf = torch.zeros(g.E(), dtype=torch.int64, device=f"cuda:{dev}")
    check("ktruss, a null handle", raw_ktruss(None, 3, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
    check("decompose, a null handle", raw_decompose(None, 3, theta=buf)[0], _lib.GM_ERR_INVALID)
    with g.to_device(dev) as sym:
        for k in (-1, 0, 1, 2, 13, 100):
            check(f"ktruss k = {k}", raw_ktruss(sym, k, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
            check(f"decompose k = {k}", raw_decompose(sym, k, theta=buf)[0], _lib.GM_ERR_INVALID)
        for k in (9, 12):
            check(f"ktruss k = {k}", raw_ktruss(sym, k, 1, buf=buf)[0], _lib.GM_ERR_UNSUPPORTED)
            check(f"decompose k = {k}", raw_decompose(sym, k, theta=buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose without a theta array", raw_decompose(sym, 3)[0], _lib.GM_ERR_INVALID)
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("ktruss world = 2", raw_ktruss(sym, 3, 1, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose world = 2", raw_decompose(sym, 3, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        counts = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = counts.data_ptr()
        check("ktruss d_counts", raw_ktruss(sym, 3, 1, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose d_counts", raw_decompose(sym, 3, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        with sym.orient() as dag:
            check("ktruss, an oriented copy", raw_ktruss(dag, 3, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
            check("decompose, an oriented copy", raw_decompose(dag, 3, theta=buf)[0], _lib.GM_ERR_INVALID)
        check("nothing was written", bool((buf.cpu().numpy() == 0).all()), True)
        # the arrays may be left out: the numbers alone
        want = R.ktruss(g, 3, 2)
        check("ktruss without an array", raw_ktruss(sym, 3, 2), (_lib.GM_OK,) + tuple(want[1:]))
        d = ref_decompose("citeseer", 3)
        check("decompose without a round array", raw_decompose(sym, 3, theta=buf), (_lib.GM_OK, d.c_max, d.rounds))
        check_arrays("... its theta", buf.cpu().numpy().view(np.uint64), d.theta)
    devopt("GM_BIG_NE", "1")  # a handle of "2^31 entries or more" (the developer option gives a small graph such a handle)
    big = g.to_device(dev)
    devopt("GM_BIG_NE", None)
    with big:
        check("ktruss, a big handle", raw_ktruss(big, 3, 1, buf=buf)[0], _lib.GM_ERR_TOO_LARGE)
        check("decompose, a big handle", raw_decompose(big, 3, theta=buf)[0], _lib.GM_ERR_TOO_LARGE)
    rev = g.col_idx.copy()
    for v in range(g.V()):
        a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
        rev[a:b] = rev[a:b][::-1]
    with Graph(row_ptr=g.row_ptr.copy(), col_idx=rev, name="citeseer_descending").to_device(dev) as sym:
        check("ktruss, unsorted rows", raw_ktruss(sym, 3, 1, buf=buf)[0], _lib.GM_ERR_INVALID)
        assert b"ascending" in _lib.load().gm_last_error()
        check("decompose, unsorted rows", raw_decompose(sym, 4, theta=buf)[0], _lib.GM_ERR_INVALID)


def test_graphs_without_edges_and_c_zero(dev):
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        for k in (3, 4):
            theta, rnd, c_max, rounds = clique_truss_decompose(sym, k)
            check(f"no edges k={k}", (theta.tolist(), rnd.tolist(), c_max, rounds), ([], [], 0, 1))
            check(f"no edges k={k} c=1", (lambda r: (r[0], r[1], r[2].tolist(), r[3]))(clique_ktruss(sym, k, 1)), (0, 0, [], 1))
    # a triangle and a pendant edge: at k = 3 the pendant edge has theta 0, at k = 4 everything has
    g = csr_from_pairs(5, np.array([1, 1, 2, 3], dtype=np.uint64), np.array([2, 3, 3, 4], dtype=np.uint64))
    with g.to_device(dev) as sym:
        for k in (3, 4):
            check_decompose("triangle + pendant edge", g, sym, k, R.decompose(g, k))
            check_ktruss("triangle + pendant edge", g, sym, k, 0, R.ktruss(g, k, 0))
            check_ktruss("triangle + pendant edge", g, sym, k, 1, R.ktruss(g, k, 1))
        check("c = 0 removes nothing", clique_ktruss(sym, 3, 0)[0], 4)


def test_beside_other_solvers_and_twice(dev):
    """before and after gm_sgl("diamond"), gm_clique_local, gm_ktruss and gm_clique_kcore on the same handle, whose results do not change;
    two calls in a row and a call on the graph as numbered give identical arrays"""
    name, k = "rmat8_ef8_s42", 4
    g = load_graph(name)
    want = ref_decompose(name, k)
    with g.to_device(dev) as sym:
        first = check_decompose(name + " on a fresh handle", g, sym, k, want)
        others = (SglSolver(sym, "diamond"), clique_local(sym, k), ktruss(sym, 4), clique_kcore(sym, k, 3))
        again = check_decompose(name + " after the other solvers", g, sym, k, want)
        for x, y in zip(first[:2], again[:2]):
            check_arrays("two calls, identical arrays", x, y)
        numbered = check_decompose(name + " as numbered", g, sym, k, want, tune=AS_NUMBERED)
        check_arrays("as numbered, identical theta", numbered[0], first[0])
        check_arrays("as numbered, identical rounds", numbered[1], first[1])
        mid = int(np.unique(want.theta)[-2])
        a = check_ktruss(name, g, sym, k, mid, R.ktruss(g, k, mid))
        b = check_ktruss(name + " as numbered", g, sym, k, mid, R.ktruss(g, k, mid), tune=AS_NUMBERED)
        check_arrays("ktruss twice, identical arrays", a, b)
        after = (SglSolver(sym, "diamond"), clique_local(sym, k), ktruss(sym, 4), clique_kcore(sym, k, 3))
        check("diamond unchanged", after[0], others[0])
        check("gm_clique_local total unchanged", after[1][0], others[1][0])
        check_arrays("gm_clique_local per vertex unchanged", after[1][1], others[1][1])
        check_arrays("gm_clique_local per entry unchanged", after[1][2], others[1][2])
        check("gm_ktruss unchanged", (after[2][0], after[2][2]), (others[2][0], others[2][2]))
        check_arrays("gm_ktruss per entry unchanged", after[2][1], others[2][1])
        check_arrays("gm_ktruss against its reference", after[2][1], TR.ktruss(g, 4)[0])
        check("gm_clique_kcore unchanged", (after[3][0], after[3][1], after[3][3]), (others[3][0], others[3][1], others[3][3]))
        check_arrays("gm_clique_kcore per vertex unchanged", after[3][2], others[3][2])
        check_decompose(name + " k=3 on the same handle", g, sym, 3, ref_decompose(name, 3))


def test_every_block_goes_back_with_the_handle(dev):
    a, p, k = 520, 0.05, 4  # (the wide path: the heavy list and the scratch slots are allocated too)
    m = G.booster(a, p, a, k)
    g = G.hub_edge_gadget(a, p, m, a)
    want = G.expected(g, a, p, m, a, k)
    before = dev_live_blocks()
    sym = g.to_device(dev)
    assert dev_live_blocks() > before
    for _ in range(2):
        check_ktruss("gadget", g, sym, k, want["c"], (want["cnt"], want["edges"], want["cliques"], want["rounds"]))
    sym.free()
    check("live device blocks after the handle is freed", dev_live_blocks(), before)
