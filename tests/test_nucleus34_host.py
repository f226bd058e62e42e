"""The rounds of the triangle nuclei without a device (tests/nucleus34_ref.py): the whole-frontier rounds with the rule of the decrements give
the theta of a one-triangle-at-a-time peel that recounts from scratch, destroy every 4-clique exactly once, and land on the closed forms."""
from math import comb

import numpy as np
import pytest

import nucleus34_ref as R
from graphminer_amd.rmat import csr_from_pairs


def gnp(n, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    return csr_from_pairs(n, iu[keep].astype(np.uint64), ju[keep].astype(np.uint64))


def complete(n):
    iu, ju = np.triu_indices(n, 1)
    return csr_from_pairs(n, iu.astype(np.uint64), ju.astype(np.uint64))


def book(m):
    """the triangle {0, 1, 2} and m pairwise non-adjacent pages, each joined to all three corners"""
    pages = np.arange(3, 3 + m, dtype=np.uint64)
    s = np.concatenate([np.array([0, 0, 1], dtype=np.uint64)] + [np.full(m, c, dtype=np.uint64) for c in (0, 1, 2)])
    d = np.concatenate([np.array([1, 2, 2], dtype=np.uint64), pages, pages, pages])
    return csr_from_pairs(3 + m, s, d)


@pytest.mark.parametrize("p", [0.5, 0.7, 0.85])
def test_rounds_agree_with_the_one_at_a_time_peel(p):
    for seed in range(12):
        n = 5 + seed % 7
        g = gnp(n, p, 1000 * seed + int(100 * p))
        d = R.decompose(g)
        want = R.peel_one_at_a_time(g)
        total = len(R.cliques4(g))
        print(f"n={n} p={p} seed={seed}: {len(want)} triangles, {total} cliques, c_max {d.c_max}, rounds {d.rounds}, destroyed {d.destroyed}", flush=True)
        assert d.theta == want
        assert d.destroyed == total
        assert d.c_max == max(want.values(), default=0)
        assert sum(R.k4(g).values()) == 4 * total
        for c in range(d.c_max + 2):
            q = R.nucleus(g, c)
            inside = {t for t, v in q.cnt.items() if v != R.REMOVED}
            assert inside == {t for t, v in d.theta.items() if v >= c}
            assert sum(q.cnt[t] for t in inside) == 4 * q.cliques and q.triangles == len(inside)


@pytest.mark.parametrize("n", [3, 4, 5, 8, 11])
def test_complete_graph(n):
    d = R.decompose(complete(n))
    print(f"K_{n}: theta {set(d.theta.values())} rounds {d.rounds} destroyed {d.destroyed}", flush=True)
    assert set(d.theta.values()) == {n - 3} and len(d.theta) == comb(n, 3)
    assert (d.c_max, d.rounds, d.destroyed) == (n - 3, 2, comb(n, 4))
    assert set(d.round.values()) == {1}


@pytest.mark.parametrize("m", [2, 5, 40])
def test_book(m):
    g = book(m)
    assert R.k4(g)[(0, 1, 2)] == m
    d = R.decompose(g)
    print(f"book m={m}: theta {set(d.theta.values())} rounds {d.rounds} destroyed {d.destroyed}", flush=True)
    assert set(d.theta.values()) == {1} and len(d.theta) == 3 * m + 1
    assert (d.c_max, d.rounds, d.destroyed) == (1, 3, m)
    assert d.round[(0, 1, 2)] == 2 and sorted(set(d.round.values())) == [1, 2]


def test_no_triangles():
    g = csr_from_pairs(4, np.array([0, 1, 2], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint64))
    d = R.decompose(g)
    assert (d.theta, d.c_max, d.rounds, d.destroyed) == ({}, 0, 1, 0)
    assert R.nucleus(g, 1)[1:] == (0, 0, 1, 0)
