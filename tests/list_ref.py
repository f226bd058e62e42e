"""The triangle list in plain numpy (the reference of tests/test_list_host.py and tests/test_gpu_list.py): for every u, every neighbour
v > u and every w > v in N(u) ^ N(v) the row (u, v, w) -- int32[T, 3], sorted lexicographically (list_ref); the same rows by another walk,
over the oriented lists, in the order gm_tc_list documents, with every oriented entry's first slot (list_ref_ordered)."""
from __future__ import annotations

import numpy as np


def list_ref(g) -> np.ndarray:
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col_idx, dtype=np.int64)
    rows = []
    for u in range(len(rp) - 1):
        nu = col[rp[u]:rp[u + 1]]
        for v in nu[nu > u]:
            w = np.intersect1d(nu, col[rp[v]:rp[v + 1]], assume_unique=True)
            w = w[w > v]
            if w.size:
                rows.append(np.stack([np.full(w.size, u), np.full(w.size, v), w], axis=1))
    out = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 3), dtype=np.int32)
    return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))]


def list_ref_ordered(g):
    """the list in the order gm_tc_list documents, and where every oriented entry starts in it: (int32[T, 3], int64[entries + 1]).
    Orient by (degree, id): v is in N+(u) when its degree is the greater, ties by id.  For u ascending by id, for v ascending in N+(u), for
    w ascending in N+(u) & N+(v) the row (u, v, w) sorted ascending; the second array is the exclusive sum of the per-entry row counts over
    the entries (u, v) in that order (its last value is T).  Nothing of the library takes part."""
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col_idx, dtype=np.int64)
    nv = len(rp) - 1
    deg = np.diff(rp)
    out = []
    for u in range(nv):
        nu = col[rp[u]:rp[u + 1]]
        out.append(np.sort(nu[(deg[nu] > deg[u]) | ((deg[nu] == deg[u]) & (nu > u))]))
    has_out = np.array([o.size > 0 for o in out], dtype=bool)
    counts = [np.zeros(o.size, dtype=np.int64) for o in out]
    rows = []
    mark = np.zeros(nv, dtype=bool)
    for u in range(nv):
        ou = out[u]
        if ou.size < 2:
            continue  # (a row needs v and w in N+(u))
        mark[ou] = True
        for i in np.flatnonzero(has_out[ou]).tolist():
            v = int(ou[i])
            w = out[v][mark[out[v]]]  # ascending: N+(v) is
            if w.size:
                counts[u][i] = w.size
                rows.append(np.stack([np.full(w.size, u), np.full(w.size, v), w], axis=1))
        mark[ou] = False
    tri = np.sort(np.concatenate(rows), axis=1).astype(np.int32) if rows else np.zeros((0, 3), dtype=np.int32)
    off = np.zeros(sum(o.size for o in out) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(counts) if counts else np.zeros(0, dtype=np.int64), out=off[1:])
    return tri, off


def sort_rows(tri: np.ndarray) -> np.ndarray:
    """the rows of an int32[n, 3] array in lexicographic order"""
    tri = np.asarray(tri).reshape(-1, 3)
    return tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))]
