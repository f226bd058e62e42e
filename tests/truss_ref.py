"""Plain Python / numpy ground truth for the local counts and the k-truss on SMALL graphs (test helper; shares no code with the library).

  supports(g)           per entry (u, v) of the CSR: |N(u) ^ N(v)|
  vertex_triangles(g)   per vertex: the triangles it lies in
  ktruss(g, k)          (per entry: the support of its edge inside the k-truss or REMOVED, undirected edges of the truss, rounds)
  trussness(g)          (per entry: the largest k whose k-truss holds its edge, the largest of them, rounds)

Peeling is naive and sequential: one edge of the frontier after the other leaves the graph and takes one from the support of the two other
edges of every triangle it was in.  The frontier itself is taken as a whole -- every alive edge below the threshold when a round begins --
so that `rounds` counts what the library counts: the rounds run, the one that finds the frontier empty included.  trussness raises k from 3;
from a level whose frontier is empty it goes to the smallest alive support + 3, the first level that can remove an edge.  A self loop is
not an edge: support 0, REMOVED, trussness 0."""
from __future__ import annotations

import numpy as np

REMOVED = 0xFFFFFFFF


def _rows(g):
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp)), np.asarray(g.col_idx, dtype=np.int64)


def _edge_supports(g) -> dict:
    """{(u, v), u < v: |N(u) ^ N(v)|}"""
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col_idx)
    out = {}
    for u in range(rp.size - 1):
        nu = col[rp[u]:rp[u + 1]]
        for v in nu[nu > u]:
            out[(u, int(v))] = int(np.intersect1d(nu, col[rp[v]:rp[v + 1]], assume_unique=True).size)
    return out


def _per_entry(g, values: dict, loop_value: int) -> np.ndarray:
    src, dst = _rows(g)
    return np.array([loop_value if u == v else values[(min(u, v), max(u, v))] for u, v in zip(src.tolist(), dst.tolist())], dtype=np.uint32)


def supports(g) -> np.ndarray:
    return _per_entry(g, _edge_supports(g), 0)


def vertex_triangles(g) -> np.ndarray:
    src, _ = _rows(g)
    s = np.bincount(src, weights=supports(g).astype(np.float64), minlength=len(g.row_ptr) - 1).astype(np.uint64)
    assert not (s & 1).any()
    return s >> 1


class _Peeler:
    def __init__(self, g):
        self.sup = _edge_supports(g)
        self.adj = {}
        for (u, v) in self.sup:
            self.adj.setdefault(u, set()).add(v)
            self.adj.setdefault(v, set()).add(u)
        self.rounds = 0

    def level(self, k: int, removed_at=None):
        """the rounds of threshold k - 2, until one finds the frontier empty; returns whether any edge left"""
        any_left = False
        while True:
            frontier = [e for e, s in self.sup.items() if s < k - 2]
            self.rounds += 1
            if not frontier:
                return any_left
            any_left = True
            for (u, v) in frontier:
                for w in self.adj[u] & self.adj[v]:
                    for e in ((min(u, w), max(u, w)), (min(v, w), max(v, w))):
                        self.sup[e] -= 1
                        assert self.sup[e] >= 0
                self.adj[u].discard(v)
                self.adj[v].discard(u)
                del self.sup[(u, v)]
                if removed_at is not None:
                    removed_at[(u, v)] = k - 1


def ktruss(g, k: int):
    assert k >= 2
    p = _Peeler(g)
    all_edges = list(p.sup)
    p.level(k)
    vals = {e: p.sup.get(e, REMOVED) for e in all_edges}
    return _per_entry(g, vals, REMOVED), len(p.sup), p.rounds


def trussness(g):
    p = _Peeler(g)
    tau, k, k_max = {}, 3, 0
    while p.sup:
        if p.level(k, tau):
            k_max = k - 1
        if p.sup:
            k = min(p.sup.values()) + 3
    return _per_entry(g, tau, 0), k_max, p.rounds
