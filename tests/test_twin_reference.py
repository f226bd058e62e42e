"""The twin-graph reference (tests/twin_graphs.py) against the CPU oracle: every closed form on a grid of small sizes and several
numberings, every interpolation at sizes outside the points it was fitted on, and the k-cliques of complete multipartite graphs."""
from math import comb

import numpy as np
import pytest

import twin_graphs as T

ORDERS = [("natural", 0), ("degree", 0), ("hubs_first", 0), ("random", 1), ("random", 2)]
GRIDS = {
    "kab": [(a, b) for a in (1, 2, 3, 4, 5) for b in (1, 2, 3, 5, 8, 13)],
    "book": [(n,) for n in (1, 2, 3, 4, 5, 7, 10, 15)],
    "complete": [(n,) for n in (1, 2, 3, 5, 8, 11)],
    "multipartite": [(r, s) for r in (3, 4, 6, 8) for s in (1, 2, 3)],
}


@pytest.mark.parametrize("family", sorted(GRIDS))
def test_closed_forms_equal_the_oracle(family):
    whats = sorted(T.CLOSED[family])
    checked = 0
    for params in GRIDS[family]:
        n = T.pairs(family, params)[0]
        for order, seed in ORDERS:
            g = T.graph(family, params, order, seed=seed + n)
            for what in whats:
                got, want = T.oracle_count(g, what), T.expected(family, params, what)
                assert got == want, (family, params, order, what, got, want)
                checked += 1
    assert checked > 100


def test_closed_forms_on_an_offset_block():
    """the same counts with the graph shifted inside a larger id space of isolated vertices"""
    for family, params in (("kab", (3, 7)), ("book", (9,)), ("split", (4, 5)), ("multipartite", (4, 3))):
        n = T.pairs(family, params)[0]
        for nv, off in ((n + 40, 0), (n + 40, 40), (n + 41, 17)):
            g = T.graph(family, params, "random", seed=nv + off, nv=nv, offset=off)
            assert g.row_ptr.size == nv + 1
            for what in ("tc", "diamond", "rectangle", "motif3", "motif4"):
                assert T.oracle_count(g, what) == T.expected(family, params, what), (family, params, nv, off, what)


# every (family, what) that expected() interpolates, and two checks per closed form: interpolation must agree with it
INTERP = [("split", (4,), w) for w in T.SGL + ("clique4",)] + [("complete", (), w) for w in T.SGL if w != "tc"]


@pytest.mark.parametrize("family,fixed,what", INTERP, ids=[f"{f}-{w}" for f, _, w in INTERP])
def test_interpolation_predicts_further_sizes(family, fixed, what):
    assert not T.has_closed_form(family, what)
    fit = T.fit_sizes(what)
    assert len(fit) == T.pattern_size(what) + 1
    beyond = [max(fit) + 1, max(fit) + 2, max(fit) + 4]
    for x in beyond:
        params = fixed + (x,)
        for order, seed in (("degree", 0), ("hubs_first", 0), ("random", x)):
            want = T.oracle_count(T.graph(family, params, order, seed=seed), what)
            assert T.expected(family, params, what) == want, (family, params, order, what)


@pytest.mark.parametrize("family,params", [("kab", (4, 9)), ("book", (11,)), ("multipartite", (5, 6))])
def test_interpolation_agrees_with_the_closed_forms(family, params):
    """interpolation fitted at small sizes gives the closed form at a size far outside them"""
    far = params[:-1] + (65536,)
    for what in sorted(T.CLOSED[family]):
        assert T.interpolate(family, far, what) == T.CLOSED[family][what](*far), (family, what)


def test_split_graph_counts_at_the_16_bit_boundary():
    """the values S_{4,65532} reaches (hub degrees 65535 and 65536): more than 2^32 rectangles, houses and pentagons"""
    p = (4, 65532)
    assert T.expected("split", p, "rectangle") == 12883918863
    assert T.expected("split", p, "house") == 206134051536
    assert T.expected("split", p, "pentagon") == 51533316288


@pytest.mark.parametrize("r", [3, 4, 5, 6, 7, 8])
def test_multipartite_cliques(r):
    for s in (1, 2, 3):
        g = T.graph("multipartite", (r, s), "random", seed=r * 10 + s)
        for k in range(3, 9):
            want = comb(r, k) * s ** k
            assert T.oracle_count(g, f"clique{k}") == want == T.expected("multipartite", (r, s), f"clique{k}"), (r, s, k)


def test_numberings_are_permutations():
    n, s, d = T.pairs("split", (4, 6))
    for order, seed in ORDERS:
        new = T.numbering(n, s, d, order, seed)
        assert sorted(new.tolist()) == list(range(n))
    deg = T.graph("kab", (3, 10), "degree")
    assert np.diff(deg.row_ptr)[-4:].tolist() == [3, 10, 10, 10]  # the hubs hold the top ids
    first = T.graph("kab", (3, 10), "hubs_first")
    assert np.diff(first.row_ptr)[:4].tolist() == [10, 10, 10, 3]
    assert T.top_offset("book", (5,), 1 << 24) + 7 == 1 << 24
