"""The CPU references of the local motif counts (tests/motif_local_ref.py) against each other, the goldens and closed forms -- no GPU.
(a) the enumeration of every connected induced 3- and 4-vertex subgraph and (b) the numpy composition from t(e), R_v, K_v and the
triangles agree vertex by vertex and orbit by orbit on seeded random graphs, rmat6_ef4_s1, citeseer and cora; (a)'s column sums are the
goldens' motif3 / motif4 (the reference's own binaries); both give the closed forms of K_n, C_n, a star, a path, K_{a,b}, the Petersen
graph and a book; the matrix-product inputs the GPU tests' dense cells use agree with (b) on a small instance; and the library declares
the call."""
import functools
from math import comb

import numpy as np
import pytest

import motif_local_ref as M
from common import GOLDEN, load_graph, random_graph
from planted_squares import _graph


def check_arrays(label, got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    print(f"{label}: shape {want.shape}, {len(bad)} differ, first at {bad[:5].tolist()}", flush=True)
    assert got.shape == want.shape and got.dtype == want.dtype and len(bad) == 0, label


@functools.lru_cache(maxsize=None)
def both(name):
    g = load_graph(name)
    return g, M.enumerate_orbits(g), M.compose(g)


@pytest.mark.parametrize("name", ["rmat6_ef4_s1", "citeseer", "cora"])
def test_enumeration_against_composition_and_goldens(name):
    g, a, b = both(name)
    check_arrays(f"{name} (a) against (b)", a, b)
    check_arrays(f"{name} k = 3 composition", M.compose(g, 3), a[:4])
    assert M.counts(a[:4]) == GOLDEN[name]["motif3"]
    assert M.counts(a) == GOLDEN[name]["motif4"]
    if name == "citeseer":
        assert M.counts(a) == [222630, 111153, 22900, 3094, 2200, 255]


@pytest.mark.parametrize("nv,ne,seed", [(8, 10, 1), (10, 30, 2), (12, 66, 3), (14, 40, 4), (40, 200, 5), (60, 600, 6)])
def test_enumeration_against_composition_random(nv, ne, seed):
    g = random_graph(nv, ne, seed)
    check_arrays(f"random {nv} {ne}", M.enumerate_orbits(g), M.compose(g))


def pairs_graph(nv, pairs):
    s, d = zip(*pairs)
    return _graph(nv, s, d)


def expect(label, g, want: dict):
    """want: {orbit: per-vertex values}; every orbit not named is zero everywhere"""
    nv = len(g.row_ptr) - 1
    full = np.zeros((15, nv), dtype=np.uint64)
    for o, vals in want.items():
        full[o] = np.asarray(vals, dtype=np.uint64)
    check_arrays(f"{label} enumeration", M.enumerate_orbits(g), full)
    check_arrays(f"{label} composition", M.compose(g), full)


def test_complete_graph():
    n = 9
    g = pairs_graph(n, [(i, j) for i in range(n) for j in range(i + 1, n)])
    expect("K_9", g, {0: [n - 1] * n, 3: [comb(n - 1, 2)] * n, 14: [comb(n - 1, 3)] * n})  # only orbits 0, 3 and 14


def test_cycle():
    n = 9
    g = pairs_graph(n, [(i, (i + 1) % n) for i in range(n)])
    expect("C_9", g, {0: [2] * n, 1: [2] * n, 2: [1] * n, 4: [2] * n, 5: [2] * n})


def test_star():
    m = 7
    g = pairs_graph(m + 1, [(0, i) for i in range(1, m + 1)])
    expect("K_1,7", g, {0: [m] + [1] * m, 1: [0] + [m - 1] * m, 2: [comb(m, 2)] + [0] * m, 6: [0] + [comb(m - 1, 2)] * m, 7: [comb(m, 3)] + [0] * m})


def test_path():
    n = 8
    g = pairs_graph(n, [(i, i + 1) for i in range(n - 1)])
    r = range(n)
    expect("P_8", g, {0: [1 if i in (0, n - 1) else 2 for i in r], 1: [(i >= 2) + (i <= n - 3) for i in r], 2: [int(0 < i < n - 1) for i in r],
                      4: [(i >= 3) + (i <= n - 4) for i in r], 5: [int(1 <= i <= n - 3) + int(2 <= i <= n - 2) for i in r]})


def test_complete_bipartite():
    a, b = 4, 6
    g = pairs_graph(a + b, [(i, a + j) for i in range(a) for j in range(b)])
    side = lambda x, y: [x] * a + [y] * b  # noqa: E731
    expect("K_4,6", g, {0: side(b, a), 1: side(b * (a - 1), a * (b - 1)), 2: side(comb(b, 2), comb(a, 2)),
                        6: side(b * comb(a - 1, 2), a * comb(b - 1, 2)), 7: side(comb(b, 3), comb(a, 3)),
                        8: side((a - 1) * comb(b, 2), (b - 1) * comb(a, 2))})


def test_petersen():
    edges = [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]
    g = pairs_graph(10, edges)
    expect("Petersen", g, {0: [3] * 10, 1: [6] * 10, 2: [3] * 10, 4: [12] * 10, 5: [12] * 10, 6: [3] * 10, 7: [1] * 10})


def test_book():
    n = 11
    g = pairs_graph(n + 2, [(0, 1)] + [(s, p) for s in (0, 1) for p in range(2, n + 2)])
    want = M.book_orbits(n)
    check_arrays("B_11 enumeration", M.enumerate_orbits(g), want)
    check_arrays("B_11 composition", M.compose(g), want)
    assert int(want[12, 2]) == n - 1 and int(want[13, 0]) == comb(n, 2)


def test_dense_inputs_against_the_composition():
    """the matrix-product inputs of the dense GPU cells on a small K_n with satellites: the same orbits as (b) and as the enumeration"""
    core = 14
    g = M.clique_with_satellites(core, 10, seed=3, lo=2, hi=6)
    got = M.compose_from(g, *M.dense_inputs(g, core))
    check_arrays("K_14 + 10 satellites, dense inputs against (b)", got, M.compose(g))
    check_arrays("K_14 + 10 satellites, dense inputs against (a)", got, M.enumerate_orbits(g))


def test_the_library_declares_the_call():
    from graphminer_amd import _lib

    assert "gm_motif_local" in [s[0] for s in _lib.SYMBOLS]
    from graphminer_amd import motif_local  # noqa: F401
