"""The k-clique list in plain numpy / Python (the reference of tests/test_clique_list_host.py and tests/test_gpu_clique_list*.py), in the
order gm_clique_list documents (include/graphminer_amd.h):
  * the ROOT of a clique is its lowest vertex under the orientation of gm_graph_orient: lower degree first, ties by id;
  * rows come by ascending root id, and within a root lexicographically on the other k - 1 ids ascending (they are the ascending
    positions in the root's out-list, which is sorted by id);
  * a row is the k ids ascending, the root wherever its id sorts.
Nothing of the library takes part in a value.

  orientation(g)                 (a) degree and, per vertex, the bitset (a Python int over vertex ids) of its out-neighbours
  row_roots(g, rows)             (a) the root of every row
  clique_list_ref(g, k)          (b) the whole list, int32[n, k]
  check_list(g, k, rows, first)  (c) without enumerating: every row ascending and a clique, the rows strictly increasing in the order
  unrank / lex_window            (d) lexicographic unranking of k-subsets of range(n): the list of a complete graph
  planted_expected(p, k)         the SET of k-cliques of a tests/planted_cliques.py graph, from its blocks"""
from __future__ import annotations

from math import comb

import numpy as np


def _csr(g):
    return np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col_idx, dtype=np.int64)


def _bits(s: int):
    while s:
        low = s & -s
        yield low.bit_length() - 1
        s ^= low


def orientation(g):
    """(deg int64[nv], nbr: per vertex the bitset of N(v), out: per vertex the bitset of N+(v) -- the neighbours above it by (degree, id))"""
    rp, col = _csr(g)
    nv = len(rp) - 1
    deg = np.diff(rp)
    nbr, out = [0] * nv, [0] * nv
    for u in range(nv):
        a, o = 0, 0
        du = int(deg[u])
        for v in col[rp[u]:rp[u + 1]].tolist():
            a |= 1 << v
            dv = int(deg[v])
            if dv > du or (dv == du and v > u):
                o |= 1 << v
        nbr[u], out[u] = a, o
    return deg, nbr, out


def row_roots(g, rows: np.ndarray) -> np.ndarray:
    """the root of every row: its member that is lowest by (degree, id)"""
    rp, _ = _csr(g)
    rows = np.asarray(rows, dtype=np.int64)
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    deg = np.diff(rp)
    key = deg[rows] * (len(rp) + 1) + rows  # (degree, id) as one number
    return rows[np.arange(rows.shape[0]), np.argmin(key, axis=1)]


def _descend(nbr, cand: int, m: int, prefix: list, out: list):
    """the m-cliques inside cand, lexicographic on ascending ids, appended to out as prefix + members"""
    if m == 1:
        out.extend(prefix + [v] for v in _bits(cand))
        return
    for v in _bits(cand):
        nxt = cand & nbr[v] & ~((1 << (v + 1)) - 1)
        if nxt:
            _descend(nbr, nxt, m - 1, prefix + [v], out)


def clique_list_ref(g, k: int) -> np.ndarray:
    """every k-clique of the symmetric graph g once, int32[n, k], rows ascending, in the documented order"""
    assert k >= 2
    _, nbr, out = orientation(g)
    rows = []
    for u in range(len(nbr)):
        if out[u]:
            found = []
            _descend(nbr, out[u], k - 1, [], found)
            rows.extend(sorted(r + [u]) for r in found)
    return np.array(rows, dtype=np.int32).reshape(-1, k)


def order_keys(g, rows: np.ndarray) -> np.ndarray:
    """int64[n, k]: (root, the other k - 1 ids ascending) -- the documented order is the lexicographic order of these"""
    rows = np.asarray(rows, dtype=np.int64)
    n, k = rows.shape
    root = row_roots(g, rows)
    rest = np.sort(np.where(rows == root[:, None], np.iinfo(np.int64).max, rows), axis=1)[:, :k - 1]
    return np.concatenate([root[:, None], rest], axis=1)


def check_list(g, k: int, rows: np.ndarray, first: int = 0) -> None:
    """raises AssertionError unless every row holds k strictly ascending ids that are pairwise adjacent and the rows are strictly increasing
    in the documented order (hence distinct).  `first`: the index of rows[0] in the whole list, for the messages only."""
    rp, col = _csr(g)
    nv = len(rp) - 1
    rows = np.asarray(rows)
    assert rows.ndim == 2 and rows.shape[1] == k, f"shape {rows.shape} for k = {k}"
    r = rows.astype(np.int64)
    if r.shape[0] == 0:
        return
    assert r.min() >= 0 and r.max() < nv, f"ids outside 0 .. {nv - 1}"
    bad = np.flatnonzero((r[:, 1:] <= r[:, :-1]).any(axis=1))
    assert bad.size == 0, f"row {first + int(bad[0])} is not strictly ascending: {r[bad[0]].tolist()}"
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(rp))
    keys = np.sort((src << 32) | col)
    for a in range(k):
        for b in range(a + 1, k):
            want = (r[:, a] << 32) | r[:, b]
            at = np.minimum(np.searchsorted(keys, want), keys.size - 1)
            bad = np.flatnonzero(keys[at] != want)
            assert bad.size == 0, f"row {first + int(bad[0])} is no clique: {r[bad[0]].tolist()} lacks the edge ({r[bad[0], a]}, {r[bad[0], b]})"
    key = order_keys(g, r)
    diff = key[1:] - key[:-1]
    nz = diff != 0
    lead = np.argmax(nz, axis=1)
    step = diff[np.arange(diff.shape[0]), lead]  # the first differing column (0: equal rows)
    bad = np.flatnonzero(step <= 0)
    assert bad.size == 0, (f"rows {first + int(bad[0])} and {first + int(bad[0]) + 1} are out of order or equal: "
                           f"{r[bad[0]].tolist()} then {r[bad[0] + 1].tolist()}")


# ---- (d) complete graphs: every degree is equal, the root of a subset is its smallest id, the list is the lexicographic list of k-subsets ----
def unrank(n: int, k: int, r: int) -> list:
    """the k-subset of range(n) of rank r in lexicographic order"""
    assert 0 <= r < comb(n, k)
    out, x = [], 0
    for left in range(k, 0, -1):
        while True:
            c = comb(n - x - 1, left - 1)  # the subsets that take x next
            if r < c:
                break
            r -= c
            x += 1
        out.append(x)
        x += 1
    return out


def lex_window(n: int, k: int, first: int, count: int) -> np.ndarray:
    """rows first .. first + count - 1 of the lexicographic list of k-subsets of range(n): one unranking, then successors"""
    count = max(0, min(count, comb(n, k) - first))
    out = np.zeros((count, k), dtype=np.int32)
    if count == 0:
        return out
    cur = unrank(n, k, first)
    for t in range(count):
        out[t] = cur
        i = k - 1
        while i >= 0 and cur[i] == n - k + i:
            i -= 1
        if i < 0:
            break
        cur[i] += 1
        for j in range(i + 1, k):
            cur[j] = cur[j - 1] + 1
    return out


def sort_rows(rows: np.ndarray) -> np.ndarray:
    """the rows of an int[n, k] array in lexicographic order"""
    rows = np.asarray(rows)
    return rows[np.lexsort(rows.T[::-1])] if rows.shape[0] else rows


# ---- planted graphs (tests/planted_cliques.py): a k-clique lies inside one block plus at most one member of I -------------------------------
class _Csr:
    def __init__(self, row_ptr, col_idx):
        self.row_ptr, self.col_idx = row_ptr, col_idx


_BLOCK_CACHE: dict = {}


def _block_cliques(blk, m: int) -> np.ndarray:
    """the m-cliques of a block on its local ids, int64[n, m] (m = 1: its vertices; m = 2: its edges)"""
    import planted_cliques as P

    if (blk, m) not in _BLOCK_CACHE:
        a, b = P.block_pairs(blk)
        if m == 1:
            res = np.arange(blk.size, dtype=np.int64).reshape(-1, 1)
        elif m == 2:
            res = np.stack([a, b], axis=1).astype(np.int64).reshape(-1, 2)
        else:
            s, t = np.concatenate([a, b]), np.concatenate([b, a])
            order = np.lexsort((t, s))
            rp = np.zeros(blk.size + 1, dtype=np.int64)
            np.cumsum(np.bincount(s, minlength=blk.size), out=rp[1:])
            res = clique_list_ref(_Csr(rp, t[order]), m).astype(np.int64)
        _BLOCK_CACHE[(blk, m)] = res
    return _BLOCK_CACHE[(blk, m)]


def planted_expected(p, k: int) -> np.ndarray:
    """the SET of k-cliques of a Planted graph, int32[n, k], rows ascending, sorted lexicographically: the k-cliques of every block plus
    (member of I) x (the (k - 1)-cliques of each block it is joined to)"""
    parts = []
    for bi, blk in enumerate(p.blocks):
        ids = p.h_id[p.first[bi]:p.first[bi + 1]]
        c = _block_cliques(blk, k)
        if c.shape[0]:
            parts.append(ids[c])
    for x, m in enumerate(p.members):
        for bi in m.blocks:
            ids = p.h_id[p.first[bi]:p.first[bi + 1]]
            c = _block_cliques(p.blocks[bi], k - 1)
            if c.shape[0]:
                parts.append(np.concatenate([ids[c], np.full((c.shape[0], 1), p.i_id[x], dtype=np.int64)], axis=1))
    rows = np.concatenate(parts) if parts else np.zeros((0, k), dtype=np.int64)
    return sort_rows(np.sort(rows, axis=1).astype(np.int32))
