"""Plain numpy ground truth of the house count (test helper; imported by tests/test_house_ref_host.py, tests/map_probe_graphs.py and
tests/test_gpu_map_kernels.py).  The house -- a 4-cycle u - v - b - a with a roof c on the edge (u, v), edge-induced, as the reference's
loop nest (house.h:1-16) counts it -- as a dense closed form that knows nothing of centres, ranges, maps or numberings.  With F the 0/1
adjacency, A2 = F F, A3 = A2 F and d the degrees, per edge (u, v):

    t(u, v) = A2 o F                      triangles on the edge: the roofs
    q(u, v) = (A3 - d_u - d_v + 1) o F    paths u - a - b - v of three edges with a != v, b != u: the squares on the edge
    X(u, v) = (F (t - F)) o F             sum over the roofs c of (t(c, v) - 1): the squares whose a is the roof

    house = sum over u < v of t q - X(u, v) - X(v, u)

(t q pairs every roof with every square of the edge; a pair whose roof is a vertex of the square is no house: the roof is a when b is one
of the other t(c, v) - 1 common neighbours of c and v, and likewise b on the side of u.)  Everything is held in float64 and must stay
exact: the largest intermediate is asserted below 2^53, and the last product and sum are taken in Python integers.

A vertex of degree <= 1 lies in no house (every vertex of a house has degree >= 2 in it), and neither its row nor its column adds to t,
q - the path a, b must be inner vertices of degree >= 2 - or X.  So the form runs on the subgraph induced by the vertices of degree >= 2:
graphs padded with isolated vertices or private leaves stay cheap.  That subgraph must hold at most MAX_DENSE vertices."""
from __future__ import annotations

import numpy as np

MAX_DENSE = 2500
EXACT = float(2 ** 53)


def core_adjacency(g):
    """(dense 0/1 float64 adjacency of the subgraph induced by the vertices of degree >= 2, their ids)"""
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    col = np.asarray(g.col_idx, dtype=np.int64)
    nv = rp.size - 1
    deg = np.diff(rp)
    core = np.flatnonzero(deg >= 2)
    assert core.size <= MAX_DENSE, f"{core.size} vertices of degree >= 2: the dense form is meant for at most {MAX_DENSE}"
    cid = np.full(nv, -1, dtype=np.int64)
    cid[core] = np.arange(core.size)
    src = np.repeat(np.arange(nv, dtype=np.int64), deg)
    keep = (cid[src] >= 0) & (cid[col] >= 0)
    F = np.zeros((core.size, core.size), dtype=np.float64)
    F[cid[src[keep]], cid[col[keep]]] = 1.0
    assert np.array_equal(F, F.T) and not F.diagonal().any(), "a symmetric simple graph"
    return F, core


def house(g) -> int:
    """houses of a symmetric simple graph, exact"""
    F, _ = core_adjacency(g)
    if F.shape[0] < 5:
        return 0
    d = F.sum(axis=1)
    A2 = F @ F
    A3 = A2 @ F
    t = A2 * F
    q = (A3 - d[:, None] - d[None, :] + 1.0) * F
    X = (F @ (t - F)) * F
    for m in (A2, A3, t, q, X):
        assert float(np.abs(m).max()) < EXACT, "an intermediate left the exact range of float64"
    iu, iv = np.nonzero(np.triu(F, 1))
    ti, qi = t[iu, iv].astype(np.int64), q[iu, iv].astype(np.int64)
    xi = (X[iu, iv] + X[iv, iu]).astype(np.int64)
    assert float(t.max()) * float(max(q.max(), 1.0)) < EXACT
    total = sum(int(a) * int(b) - int(c) for a, b, c in zip(ti.tolist(), qi.tolist(), xi.tolist()))
    assert total >= 0
    return total


def house_loops(g) -> int:
    """the same count by the literal loop nest over (edge, roof, square) of a SMALL graph: the check of the closed form itself"""
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    col = np.asarray(g.col_idx, dtype=np.int64)
    nv = rp.size - 1
    adj = [set(col[rp[v]:rp[v + 1]].tolist()) for v in range(nv)]
    total = 0
    for u in range(nv):
        for v in adj[u]:
            if v < u:
                continue
            for c in adj[u] & adj[v]:
                for a in adj[u]:
                    if a == v or a == c:
                        continue
                    for b in adj[a] & adj[v]:
                        if b != u and b != c:
                            total += 1
    return total


def house_complete(n: int) -> int:
    """houses of K_n: five vertices chosen, and the 5! placings of the pattern on them fall into classes of |Aut(house)| = 2 (the mirror that
    swaps u with v and a with b): 60 C(n, 5)"""
    from math import comb

    return 60 * comb(n, 5)
