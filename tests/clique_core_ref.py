"""Plain Python ground truth for the k-clique cores on SMALL graphs (test helper; shares no code with the library).

  kcore(g, k, c)        the (k, c)-core by whole-frontier rounds: (K_v inside the core or REMOVED as np.uint64[nv], vertices, cliques, rounds)
  decompose(g, k)       the core numbers by the same rounds: a Decomposition (core, round, c_max, rounds, states, dense)
  sequential_core(g, k) the core numbers by removing ONE vertex of the smallest count at a time and recounting from scratch

K_v(H) = the k-cliques of the induced subgraph H that hold v (k = 2: the degree).  Neighbourhoods are the Python-int bitsets of
clique_local_ref.py.  A round: the frontier is every alive vertex whose count is below the threshold; a k-clique none of whose members was
removed before the round and that has a frontier member is destroyed in the round -- accounted once, by its frontier member of the
smallest id, and every member outside the frontier loses one.  So frontier vertex v works on S_v = N(v) without the removed vertices and
without the frontier vertices below v: w in S_v outside the frontier loses the (k - 2)-cliques of S_v & N(w), and the (k - 1)-cliques of
S_v are destroyed.  The round that finds an empty frontier ends its level and counts; it is the last one when nothing is alive.
Decomposition: the level starts at the smallest count of the graph, the threshold is level + 1, a vertex that enters gets core = level and
round = the 1-based index of the round; from an empty frontier the level goes to the smallest alive count.  states[r - 1] = (vertices, cliques) at the start of round r; dense = the
(round, vertices, cliques) of the state with the most cliques per vertex (exact; a tie goes to the earliest round)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from clique_local_ref import _bitsets, _count

REMOVED = 0xFFFFFFFFFFFFFFFF
Decomposition = namedtuple("Decomposition", "core round c_max rounds states dense")


def vertex_counts(nbr: list, alive: int, k: int) -> list:
    """K_v of the subgraph induced by the bitset `alive`, for every v (0 outside it)"""
    return [_count(nbr, nbr[v] & alive, k - 1) if (alive >> v) & 1 else 0 for v in range(len(nbr))]


def _members(s: int):
    while s:
        low = s & -s
        yield low.bit_length() - 1
        s ^= low


def _peel(nbr: list, k: int, cnt: list, alive: int, frontier: int) -> int:
    """one round's decrements on cnt (the frontier's own counts are not maintained); returns the cliques destroyed"""
    destroyed = 0
    for v in _members(frontier):
        s = nbr[v] & alive & ~(frontier & ((1 << v) - 1))
        destroyed += _count(nbr, s, k - 1)
        for w in _members(s & ~frontier):
            cnt[w] -= _count(nbr, s & nbr[w], k - 2)
            assert cnt[w] >= 0, (v, w)
    return destroyed


def dense_state(states: list):
    """(round, vertices, cliques) of the densest of the states that hold a vertex; (1, 0, 0) when none does"""
    best = None
    for r, (nv, nc) in enumerate(states, start=1):
        if nv > 0 and (best is None or nc * best[1] > best[2] * nv):
            best = (r, nv, nc)
    return best if best is not None else (1, 0, 0)


def kcore(g, k: int, c: int):
    assert k >= 2
    nbr = _bitsets(g)
    n = len(nbr)
    alive = (1 << n) - 1
    cnt = vertex_counts(nbr, alive, k)
    total = sum(cnt) // k
    rounds = 0
    while True:
        rounds += 1
        frontier = sum(1 << v for v in _members(alive) if cnt[v] < c)
        if not frontier:
            break
        total -= _peel(nbr, k, cnt, alive, frontier)
        alive &= ~frontier
    if not alive:
        assert total == 0, total
    out = np.array([cnt[v] if (alive >> v) & 1 else REMOVED for v in range(n)], dtype=np.uint64)
    assert sum(cnt[v] for v in _members(alive)) == k * total
    return out, bin(alive).count("1"), total, rounds


def decompose(g, k: int) -> Decomposition:
    assert k >= 2
    nbr = _bitsets(g)
    n = len(nbr)
    alive = (1 << n) - 1
    cnt = vertex_counts(nbr, alive, k)
    total = sum(cnt) // k
    core, rnd = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    level, rounds, states = min(cnt, default=0), 0, []
    while True:
        rounds += 1
        states.append((bin(alive).count("1"), total))
        frontier = sum(1 << v for v in _members(alive) if cnt[v] < level + 1)
        if not frontier:
            if not alive:
                break
            level = min(cnt[v] for v in _members(alive))
            continue
        for v in _members(frontier):
            core[v], rnd[v] = level, rounds
        total -= _peel(nbr, k, cnt, alive, frontier)
        alive &= ~frontier
    assert total == 0, total
    return Decomposition(core, rnd, int(core.max()) if n else 0, rounds, states, dense_state(states))


def sequential_core(g, k: int) -> np.ndarray:
    nbr = _bitsets(g)
    n = len(nbr)
    alive = (1 << n) - 1
    core = np.zeros(n, dtype=np.uint64)
    level = 0
    while alive:
        cnt = vertex_counts(nbr, alive, k)
        v = min(_members(alive), key=lambda x: cnt[x])
        level = max(level, cnt[v])
        core[v] = level
        alive &= ~(1 << v)
    return core
