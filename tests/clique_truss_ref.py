"""Plain Python ground truth for the k-clique trusses on SMALL graphs (test helper; shares no code with the library).

  ktruss(g, k, c)        the (k, c)-truss by whole-frontier rounds: (per entry K_e inside the truss or REMOVED as np.uint64[ne], undirected
                         edges, cliques, rounds)
  decompose(g, k)        the clique trussness by the same rounds: a Decomposition (theta, round -- both per entry --, c_max, rounds)
  sequential_truss(g, k) theta per entry by removing ONE edge of the smallest count at a time and recounting from scratch

K_e(H) = the k-cliques, all of whose edges lie in the edge set H, that hold e.  Neighbourhoods are the Python-int bitsets of
clique_local_ref.py.  An undirected edge is the pair (u, v), u < v; the order of the canonical entries of a CSR with ascending rows is the
lexicographic order of these pairs.  A round: the frontier is every alive edge whose count is below the threshold; a k-clique none of whose
edges was removed before the round and that has a frontier edge is destroyed in the round -- accounted once, by its frontier edge of the
smallest canonical entry, and every edge of it outside the frontier loses one.  So frontier edge e works on the graph of the edges that are
not removed, without the frontier edges below e: with S = the common neighbours of its ends there, w in S takes the (k - 3)-cliques of
S & N(w) from (u, w) and (v, w), an adjacent pair w < x of S takes the (k - 4)-cliques of S & N(w) & N(x) from (w, x), and the (k - 2)-cliques
of S are destroyed.  The round that finds an empty frontier ends its level and counts; it is the last one when nothing is alive.
Decomposition: the level starts at the smallest count of the graph, the threshold is level + 1, an edge that enters gets theta = level and
round = the 1-based index of the round; from an empty frontier the level goes to the smallest alive count.  A self loop is not an edge:
REMOVED, theta 0, round 0."""
from __future__ import annotations

from collections import namedtuple
from math import comb

import numpy as np

from clique_local_ref import _bitsets, _count

REMOVED = 0xFFFFFFFFFFFFFFFF
Decomposition = namedtuple("Decomposition", "theta round c_max rounds")


def _members(s: int):
    while s:
        low = s & -s
        yield low.bit_length() - 1
        s ^= low


def edge_counts(nbr: list, k: int) -> dict:
    """{(u, v), u < v: K_e} of the graph whose edges are the bitsets nbr"""
    return {(u, v): _count(nbr, nbr[u] & nbr[v], k - 2) for u in range(len(nbr)) for v in _members(nbr[u] >> (u + 1) << (u + 1))}


def _per_entry(g, values: dict, loop_value: int, dtype) -> np.ndarray:
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    src = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp)).tolist()
    dst = np.asarray(g.col_idx, dtype=np.int64).tolist()
    return np.array([loop_value if u == v else values[(min(u, v), max(u, v))] for u, v in zip(src, dst)], dtype=dtype)


def _peel(nbr: list, k: int, cnt: dict, frontier: list) -> int:
    """one round's decrements on cnt (the frontier's own counts are not maintained) and the frontier's removal from nbr; returns the
    cliques destroyed.  frontier: ascending, so that nbr is at every edge the graph without the frontier edges below it"""
    inside = set(frontier)
    destroyed = 0
    for (u, v) in frontier:
        s = nbr[u] & nbr[v]
        destroyed += _count(nbr, s, k - 2)
        for w in _members(s):
            sw = s & nbr[w]
            ci = _count(nbr, sw, k - 3)
            for e in ((min(u, w), max(u, w)), (min(v, w), max(v, w))):
                if e not in inside:
                    cnt[e] -= ci
                    assert cnt[e] >= 0, ((u, v), e)
            if k >= 4:
                for x in _members(sw >> (w + 1) << (w + 1)):
                    if (w, x) not in inside:
                        cnt[(w, x)] -= _count(nbr, sw & nbr[x], k - 4)
                        assert cnt[(w, x)] >= 0, ((u, v), (w, x))
        nbr[u] &= ~(1 << v)
        nbr[v] &= ~(1 << u)
    return destroyed


def ktruss(g, k: int, c: int):
    assert k >= 3
    nbr = _bitsets(g)
    cnt = edge_counts(nbr, k)
    all_edges = list(cnt)
    total = sum(cnt.values()) // comb(k, 2)
    alive = dict.fromkeys(all_edges)
    rounds = 0
    while True:
        rounds += 1
        frontier = sorted(e for e in alive if cnt[e] < c)
        if not frontier:
            break
        total -= _peel(nbr, k, cnt, frontier)
        for e in frontier:
            del alive[e]
    assert sum(cnt[e] for e in alive) == comb(k, 2) * total
    vals = {e: cnt[e] if e in alive else REMOVED for e in all_edges}
    return _per_entry(g, vals, REMOVED, np.uint64), len(alive), total, rounds


def decompose(g, k: int) -> Decomposition:
    assert k >= 3
    nbr = _bitsets(g)
    cnt = edge_counts(nbr, k)
    total = sum(cnt.values()) // comb(k, 2)
    alive = dict.fromkeys(cnt)
    theta, rnd = {}, {}
    level, rounds = min(cnt.values(), default=0), 0
    while True:
        rounds += 1
        frontier = sorted(e for e in alive if cnt[e] < level + 1)
        if not frontier:
            if not alive:
                break
            level = min(cnt[e] for e in alive)
            continue
        for e in frontier:
            theta[e], rnd[e] = level, rounds
            del alive[e]
        total -= _peel(nbr, k, cnt, frontier)
    assert total == 0, total
    return Decomposition(_per_entry(g, theta, 0, np.uint64), _per_entry(g, rnd, 0, np.uint32), max(theta.values(), default=0), rounds)


def sequential_truss(g, k: int) -> np.ndarray:
    nbr = _bitsets(g)
    theta = {}
    level = 0
    while True:
        cnt = edge_counts(nbr, k)
        if not cnt:
            break
        (u, v) = min(cnt, key=lambda e: (cnt[e], e))
        level = max(level, cnt[(u, v)])
        theta[(u, v)] = level
        nbr[u] &= ~(1 << v)
        nbr[v] &= ~(1 << u)
    return _per_entry(g, theta, 0, np.uint64)
