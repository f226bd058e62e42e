"""The helpers of the k-clique truss tests against each other, without a GPU: the round reference (tests/clique_truss_ref.py) against the
one-edge-at-a-time peeling that recounts from scratch, against the ordinary trussness at k = 3, and against the closed forms of the
hub-edge gadget (tests/truss_gadgets.py)."""
from math import comb

import numpy as np
import pytest

import clique_truss_ref as R
import truss_gadgets as G
import truss_ref as TR
import twin_graphs as T
from common import load_graph, random_graph
from graphminer_amd.rmat import csr_from_pairs


def subset(g, n):
    """the subgraph of g induced by its first n vertices"""
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    dst = np.asarray(g.col_idx).astype(np.int64)
    sel = (src < dst) & (dst < n)
    return csr_from_pairs(n, src[sel].astype(np.uint64), dst[sel].astype(np.uint64))


def small_graphs():
    for name, n in (("citeseer", 150), ("cora", 120), ("rmat6_ef4_s1", 64), ("rmat8_ef8_s42", 48), ("rmat10_ef16_s42", 40)):
        yield f"{name}[:{n}]", subset(load_graph(name), n)
    for seed, (n, m) in enumerate([(8, 20), (12, 40), (16, 70), (20, 90)]):
        yield f"random({n}, {m}, {seed})", random_graph(n, m, seed)
    yield "K_6", T.graph("complete", (6,))


@pytest.mark.parametrize("k", [3, 4, 5])
def test_rounds_equal_sequential_peeling(k):
    for name, g in small_graphs():
        d = R.decompose(g, k)
        seq = R.sequential_truss(g, k)
        print(f"{name} k={k}: {g.E() // 2} edges, c_max {d.c_max} rounds {d.rounds}; sequential max {int(seq.max()) if seq.size else 0}", flush=True)
        assert np.array_equal(d.theta, seq), name
        assert d.c_max == (int(d.theta.max()) if d.theta.size else 0) and d.rounds >= 1
        # the (k, c)-truss is the set of the edges of theta >= c, with the counts of the graph of those edges
        for c in sorted({0, 1, d.c_max // 2, d.c_max, d.c_max + 1}):
            cnt, edges, ncl, rounds = R.ktruss(g, k, c)
            inside = cnt != R.REMOVED
            assert np.array_equal(inside, d.theta >= c) and 2 * edges == int(inside.sum()), (name, c)
            assert int(sum(int(x) for x in cnt[inside])) == 2 * comb(k, 2) * ncl and rounds >= 1, (name, c)
        assert R.ktruss(g, k, d.c_max + 1)[1:3] == (0, 0), name


def test_k3_is_the_ordinary_truss_decomposition():
    for name in ("citeseer", "rmat8_ef8_s42"):
        g = load_graph(name)
        d = R.decompose(g, 3)
        tau, k_max, _ = TR.trussness(g)
        print(f"{name}: c_max {d.c_max} against k_max {k_max}", flush=True)
        assert np.array_equal(d.theta + np.uint64(2), tau.astype(np.uint64)) and d.c_max + 2 == k_max, name
        for c in (1, 2):
            cnt, edges, _, rounds = R.ktruss(g, 3, c)
            sup, n_edges, rounds3 = TR.ktruss(g, c + 2)
            assert np.array_equal(cnt, np.where(sup == TR.REMOVED, R.REMOVED, sup.astype(np.uint64)).astype(np.uint64)), (name, c)
            assert (edges, rounds) == (n_edges, rounds3), (name, c)


@pytest.mark.parametrize("n,k", [(5, 3), (7, 4), (9, 5), (10, 8)])
def test_complete_graph_is_one_frontier(n, k):
    d = R.decompose(T.graph("complete", (n,)), k)
    each = comb(n - 2, k - 2)
    assert (np.unique(d.theta).tolist(), np.unique(d.round).tolist(), d.c_max, d.rounds) == ([each], [1], each, 2)


@pytest.mark.parametrize("k", [3, 4, 5])
def test_gadget_closed_forms(k):
    a, p, seed = 12, 0.4, 5
    m = G.booster(a, p, seed, k)
    g = G.hub_edge_gadget(a, p, m, seed)
    want = G.expected(g, a, p, m, seed, k)
    cnt, edges, ncl, rounds = R.ktruss(g, k, want["c"])
    print(f"a={a} k={k} m={m}: c {want['c']} edges {edges} cliques {ncl} rounds {rounds} spoke decrements {want['spoke_decrements']} "
          f"pair decrements {want['pair_decrements']}", flush=True)
    assert np.array_equal(cnt, want["cnt"])
    assert (edges, ncl, rounds) == (want["edges"], want["cliques"], want["rounds"])
    assert len(want["spoke_decrements"]) >= (3 if k >= 4 else 1) and len(want["pair_decrements"]) >= (3 if k >= 5 else 1)
    if m > 2:  # one booster less: the closed forms themselves say that the hub edge is no longer alone
        with pytest.raises(AssertionError):
            G.expected(G.hub_edge_gadget(a, p, m - 1, seed), a, p, m - 1, seed, k)


def held_against_the_reference(label, g, k, want):
    cnt, edges, ncl, rounds = R.ktruss(g, k, want["c"])
    bad = np.flatnonzero(cnt != want["cnt"])
    print(f"{label} k={k}: c {want['c']}; the reference: edges {edges} cliques {ncl} rounds {rounds}, the closed forms: {want['edges']} "
          f"{want['cliques']} {want['rounds']}; {bad.size} of {cnt.size} entries differ", flush=True)
    assert bad.size == 0, label
    assert (edges, ncl, rounds) == (want["edges"], want["cliques"], want["rounds"]), label
    return cnt


@pytest.mark.parametrize("k", [3, 4, 5])
def test_split_gadget_closed_forms(k):
    """e and X leave in one frontier and G' = G - e - X is two one-sided gadgets: expected per half against the rounds of the reference"""
    for a in range(12, 17):
        p, q, seed = 0.5, 0.5, a
        m = G.split_booster(a, p, q, seed, k)
        g = G.split_hub_edge_gadget(a, p, q, m, seed)
        want = G.split_expected(g, a, p, q, m, seed, k)
        cnt = held_against_the_reference(f"split gadget a={a} m={m}", g, k, want)
        assert int((cnt == R.REMOVED).sum()) == 2 * (want["x"] + 1) and want["x"] >= 8
        d = R.decompose(g, k)
        assert np.array_equal(d.theta < want["c"], cnt == R.REMOVED), "in the decomposition e and X are what lies below c"
        if m > 2:  # one booster less: the closed forms themselves say that something else of G' falls below c
            with pytest.raises(AssertionError):
                G.split_expected(G.split_hub_edge_gadget(a, p, q, m - 1, seed), a, p, q, m - 1, seed, k)


@pytest.mark.parametrize("k", [3, 4, 5])
def test_three_hub_closed_forms(k):
    """three hubs, in a triangle and with (h2, h3) left out: the closed forms extended by the number of hubs against the reference"""
    a, p, seed = 12, 0.4, 12
    for triangle in (True, False):
        m = G.booster(a, p, seed, k, 3, triangle)
        g = G.hub_edge_gadget(a, p, m, seed, 3, triangle)
        want = G.expected(g, a, p, m, seed, k, 3, triangle)
        cnt = held_against_the_reference(f"three hubs a={a} m={m} triangle={triangle}", g, k, want)
        assert int((cnt == R.REMOVED).sum()) == (6 if triangle else 4)


def test_preconditions_of_the_gpu_cells():
    """every gadget cell of tests/test_gpu_clique_truss.py: split_expected / expected assert, from the closed forms alone, that exactly the
    hub edge(s) and X enter the first frontier and that everything else ends at or above c -- pure arithmetic, no GPU"""
    from common import kcl_row_constants

    rc = kcl_row_constants()
    for a, p, q, k in G.split_cells(rc):
        m = G.split_booster(a, p, q, a, k)
        want = G.split_expected(G.split_hub_edge_gadget(a, p, q, m, a), a, p, q, m, a, k)
        assert want["x"] >= 8 and want["x_words"] == (0, want["words"] - 1) and want["x_most"] < want["c"]
        assert len(want["spoke_decrements"]) >= 3
    for a, p, k in G.triangle_cells(rc):
        m = G.booster(a, p, a, k, 3, True)
        want = G.expected(G.hub_edge_gadget(a, p, m, a, 3, True), a, p, m, a, k, 3, True)
        assert int((want["cnt"] == R.REMOVED).sum()) == 6
    for i, (a, p, k) in enumerate(G.second_group_cells(rc)):
        m = G.booster(a, p, a, k)
        want = G.expected(G.hub_edge_gadget(a, p, m, a), a, p, m, a, k)
        one, both = G.a_edges_from(a, p, a, rc["lanes"])
        print(f"a={a}: {one} edges of A reach position {rc['lanes']}, {both} with both ends", flush=True)
        assert a > rc["lanes"] and one >= 1 and (i == 0 or both >= 1) and len(want["spoke_decrements"]) >= 3
    a, p, k, least_m = G.long_row_cell(rc)
    m = max(G.booster(a, p, a, k), least_m)
    g = G.hub_edge_gadget(a, p, m, a)
    G.expected(g, a, p, m, a, k)
    assert int(np.diff(g.row_ptr)[:a].min()) > 4 * a and rc["regs2"] < a <= rc["lds"]


def test_book_takes_every_page_from_the_spine_in_one_round():
    for k in (3, 4):
        d = R.decompose(G.book(6, k), k)
        assert (np.unique(d.theta).tolist(), d.c_max, d.rounds) == ([1], 1, 3), k
        assert int(d.round[0]) == 2 and np.flatnonzero(d.round != 1).size == 2, k  # (entry 0 is the spine's: it and its reverse leave in round 2)
