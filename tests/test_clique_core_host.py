"""The helpers of the k-clique core tests against each other, without a GPU: the round reference (tests/clique_core_ref.py) against the
one-vertex-at-a-time peeling that recounts from scratch, against a textbook core decomposition at k = 2, and against the closed forms of
the hub gadget (tests/core_gadgets.py)."""
from fractions import Fraction

import numpy as np
import pytest

import clique_core_ref as R
import core_gadgets as G
import twin_graphs as T
from common import load_graph, random_graph


def textbook_core_numbers(g):
    """the ordinary core decomposition: repeatedly remove a vertex of the smallest remaining degree"""
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col_idx, dtype=np.int64)
    n = rp.size - 1
    deg = [int(rp[v + 1] - rp[v]) for v in range(n)]
    gone, core, level = [False] * n, [0] * n, 0
    for _ in range(n):
        v = min((x for x in range(n) if not gone[x]), key=lambda x: deg[x])
        level = max(level, deg[v])
        core[v], gone[v] = level, True
        for w in col[rp[v]:rp[v + 1]].tolist():
            if not gone[w]:
                deg[w] -= 1
    return np.array(core, dtype=np.uint64)


def small_graphs():
    yield "rmat6_ef4_s1", load_graph("rmat6_ef4_s1")
    for seed, (n, m) in enumerate([(12, 40), (20, 90), (30, 200)]):
        yield f"random({n}, {m}, {seed})", random_graph(n, m, seed)
    yield "K_6", T.graph("complete", (6,))


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_rounds_equal_sequential_peeling(k):
    for name, g in small_graphs():
        d = R.decompose(g, k)
        seq = R.sequential_core(g, k)
        print(f"{name} k={k}: c_max {d.c_max} rounds {d.rounds} dense {d.dense}; sequential max {int(seq.max())}", flush=True)
        assert np.array_equal(d.core, seq), name
        assert d.c_max == int(d.core.max()) and d.rounds == len(d.states) and int(d.round.min()) >= 1
        # the (k, c)-core is the set of the vertices of core number >= c, with the counts of that induced subgraph
        for c in sorted({0, 1, d.c_max // 2, d.c_max, d.c_max + 1}):
            cnt, nvert, ncl, rounds = R.kcore(g, k, c)
            inside = cnt != R.REMOVED
            assert np.array_equal(inside, d.core >= c) and nvert == int(inside.sum()), (name, c)
            assert int(sum(int(x) for x in cnt[inside])) == k * ncl and rounds >= 1, (name, c)


def test_k2_is_the_ordinary_core_decomposition():
    for name in ("citeseer", "rmat8_ef8_s42"):
        g = load_graph(name)
        d = R.decompose(g, 2)
        want = textbook_core_numbers(g)
        print(f"{name}: degeneracy {d.c_max} against {int(want.max())}", flush=True)
        assert np.array_equal(d.core, want), name


def test_figures_of_the_round_scheme():
    """citeseer at k = 3: the largest core number, the rounds and the densest state; K_n is one frontier; a windmill takes two"""
    d = R.decompose(load_graph("citeseer"), 3)
    print("citeseer k=3:", d.c_max, d.rounds, d.dense, flush=True)
    assert (d.c_max, d.rounds, d.dense[1:]) == (12, 52, (15, 113))
    d = R.decompose(T.graph("complete", (7,)), 4)
    assert (np.unique(d.core).tolist(), np.unique(d.round).tolist(), d.rounds, d.dense) == ([20], [1], 2, (1, 7, 35))
    d = R.decompose(G.windmill(5), 3)
    assert (np.unique(d.core).tolist(), d.round.tolist(), d.rounds) == ([1], [2] + [1] * 10, 3)
    d = R.decompose(G.star(6), 2)
    assert (np.unique(d.core).tolist(), d.round.tolist(), d.rounds) == ([1], [2] + [1] * 6, 3)


def test_dense_is_the_argmax_of_the_states():
    for name, g in small_graphs():
        for k in (2, 3):
            d = R.decompose(g, k)
            best = None
            for r, (nv, nc) in enumerate(d.states, start=1):
                if nv > 0 and (best is None or Fraction(nc, nv) > Fraction(best[2], best[1])):
                    best = (r, nv, nc)
            print(f"{name} k={k}: dense {d.dense} of {len(d.states)} states", flush=True)
            assert d.dense == (best if best is not None else (1, 0, 0)), name
            # the state of round r is {v : round[v] >= r}
            for r, (nv, _) in enumerate(d.states, start=1):
                assert nv == int((d.round >= r).sum()), (name, r)


@pytest.mark.parametrize("k,hubs", [(3, 1), (4, 1), (3, 2), (4, 2)])
def test_gadget_closed_forms(k, hubs):
    a, p, m, seed = 20, 0.3, 14, 5
    want = G.expected(a, p, m, seed, k, hubs)
    g = G.hub_gadget(a, p, m, seed, hubs)
    cnt, nvert, ncl, rounds = R.kcore(g, k, want["c"])
    print(f"a={a} k={k} hubs={hubs}: c {want['c']} vertices {nvert} cliques {ncl} rounds {rounds} decrements {want['decrements']}", flush=True)
    assert np.array_equal(cnt, want["cnt"])
    assert (nvert, ncl, rounds) == (want["vertices"], want["cliques"], want["rounds"])
    assert len(want["decrements"]) >= 3
