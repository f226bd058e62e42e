"""Plain numpy ground truth of the local 4-cycle counts (test helper; imported by tests/test_rect_local_host.py and the GPU tests of
gm_rect_local).  It uses the UNPRUNED identities, which know nothing of the kernel's centres, ranges or numbering:

    R_uv = sum over w in N(u) \\ {v} of (codeg(w, v) - 1)      the 4-cycles u - v - y - w: y a common neighbour of w and v other than u
    R_v  = sum over x != v of C(codeg(v, x), 2)               the 4-cycles v - a - x - b: x the vertex opposite v

codeg(a, b) = |N(a) ^ N(b)|.  The 4-cycles are edge-induced (chords do not matter), as the reference's `rectangle` counts them.
A vertex of degree 1 lies on no cycle: those are stripped first (their entries are 0), the identities run on the rest under compact ids,
so graphs padded with private leaves stay cheap.  Per vertex v one bincount over the rows of its neighbours gives codeg(v, .); the work is
the number of 2-paths of the stripped graph."""
from __future__ import annotations

import numpy as np


def _ranges(starts, lens):
    """the concatenation of arange(s, s + n) over (starts, lens), and the first index of every piece in it (every n > 0)"""
    first = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=first[1:])
    idx = np.arange(int(lens.sum()), dtype=np.int64) + np.repeat(starts - first, lens)
    return idx, first


def rect_local(g):
    """(R per entry as uint64[ne] in the graph's entry order, R_v as uint64[nv]) of a symmetric simple graph with ascending rows"""
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    col = np.asarray(g.col_idx, dtype=np.int64)
    nv, ne = rp.size - 1, col.size
    deg = np.diff(rp)
    src = np.repeat(np.arange(nv, dtype=np.int64), deg)
    keep = (deg[src] >= 2) & (deg[col] >= 2)         # the entries between two vertices of degree >= 2
    core = np.flatnonzero(deg >= 2)
    cid = np.full(nv, -1, dtype=np.int64)
    cid[core] = np.arange(core.size)
    kept = np.flatnonzero(keep)                        # their indices in the graph's entry order (rows stay ascending)
    csrc, ccol = cid[src[kept]], cid[col[kept]]
    n = core.size
    crp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(csrc, minlength=n), out=crp[1:])
    cdeg = np.diff(crp)
    ent = np.zeros(ne, dtype=np.uint64)
    rv = np.zeros(nv, dtype=np.uint64)
    for v in range(n):
        nb = ccol[crp[v]:crp[v + 1]]
        if nb.size == 0:
            continue
        idx, first = _ranges(crp[nb], cdeg[nb])       # the rows of v's neighbours: every row holds v, so none is empty
        w = ccol[idx]
        cd = np.bincount(w, minlength=n)              # codeg(v, .); cd[v] = deg(v)
        t = cd[w] - 1
        t[w == v] = 0                                 # w != v
        ent[kept[crp[v]:crp[v + 1]]] = np.add.reduceat(t, first).astype(np.uint64)   # the entries v -> u, u in id order
        cd[v] = 0
        rv[core[v]] = np.uint64(int((cd * (cd - 1) // 2).sum()))
    return ent, rv


def total(rv):
    """the 4-cycles of the graph from R_v: every cycle has four vertices"""
    s = sum(int(x) for x in rv)
    assert s % 4 == 0
    return s // 4


def total_by_pairs(g):
    """the 4-cycles of the graph alone, for graphs with too many vertices of degree >= 2 for rect_local's bincount per vertex: every
    2-path u - x - v, u < v, listed once (the rows of equal degree d together, C(d, 2) pairs each), codeg(u, v) = how often a pair occurs,
    and sum C(codeg, 2) counts every cycle by both of its diagonals.  The work is the number of 2-paths."""
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    col = np.asarray(g.col_idx, dtype=np.int64)
    deg = np.diff(rp)
    keys = []
    for d in np.unique(deg[deg >= 2]):
        rows = np.flatnonzero(deg == d)
        nb = col[rp[rows][:, None] + np.arange(d)[None, :]]   # ascending within a row
        i, j = np.triu_indices(int(d), 1)
        keys.append(((nb[:, i] << 32) | nb[:, j]).ravel())
    if not keys:
        return 0
    codeg = np.unique(np.concatenate(keys), return_counts=True)[1].astype(np.int64)
    s = int((codeg * (codeg - 1) // 2).sum())
    assert s % 2 == 0
    return s // 2


def brute_force(g):
    """the same two arrays by listing every 4-cycle of a SMALL graph (the check of the identities themselves)"""
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    col = np.asarray(g.col_idx, dtype=np.int64)
    nv = rp.size - 1
    adj = [set(col[rp[v]:rp[v + 1]].tolist()) for v in range(nv)]
    pos = {(v, int(u)): int(rp[v]) + i for v in range(nv) for i, u in enumerate(col[rp[v]:rp[v + 1]])}
    ent = np.zeros(col.size, dtype=np.uint64)
    rv = np.zeros(nv, dtype=np.uint64)
    for a in range(nv):  # a the smallest vertex of the cycle a - b - c - d, b < d
        for b in adj[a]:
            for d in adj[a]:
                if not (a < b < d):
                    continue
                for c in adj[b] & adj[d]:
                    if c > a:
                        for x, y in ((a, b), (b, c), (c, d), (d, a)):
                            ent[pos[(x, y)]] += np.uint64(1)
                            ent[pos[(y, x)]] += np.uint64(1)
                        for x in (a, b, c, d):
                            rv[x] += np.uint64(1)
    return ent, rv
