"""The triangle list in plain numpy (the reference of tests/test_list_host.py and tests/test_gpu_list.py): for every u, every neighbour
v > u and every w > v in N(u) ^ N(v) the row (u, v, w) -- int32[T, 3], sorted lexicographically."""
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


def sort_rows(tri: np.ndarray) -> np.ndarray:
    """the rows of an int32[n, 3] array in lexicographic order"""
    tri = np.asarray(tri).reshape(-1, 3)
    return tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))]
