"""CPU references for the local motif counts (gm_motif_local): the 15 graphlet-degree orbits of every vertex, Przulj's numbering.

(a) enumerate_orbits(g): every connected vertex-induced 3- and 4-vertex subgraph once (ESU), each of its vertices classified by the subgraph's
    edge count and the vertex's degree inside it.  Knows nothing of the closed forms.  For graphs of up to a few million subgraphs.
(b) compose(g): numpy, for larger graphs -- t(e) from truss_ref, R_v from rect_local_ref, K_v from clique_local_ref, the diamond term
    N12(v) = sum over the triangles {v, a, b} of (t(ab) - 1) from the triangles themselves, the neighbour sums from their definitions and
    the substitution from non-induced to induced written out here, independently of csrc/gm_orbit.h.  compose_from(...) is the same with
    the four inputs handed in (the dense cells of the GPU tests take them from matrix products, dense_inputs).
All values are uint64 modulo 2^64, as the library's."""
from __future__ import annotations

from math import comb

import numpy as np

N_ORBITS = {3: 4, 4: 15}
M64 = (1 << 64) - 1


def _rows(g):
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    return rp, np.asarray(g.col_idx, dtype=np.int64), np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


# ---- (a) enumeration ---------------------------------------------------------------------------------------------------------------------
def _orbit(m, mx, d):
    """the orbit of a vertex of degree d inside a connected 4-vertex subgraph of m edges and largest degree mx"""
    if m == 3:
        return (6 if d == 1 else 7) if mx == 3 else (4 if d == 1 else 5)
    if m == 4:
        return 8 if mx == 2 else (9, 10, 11)[d - 1]
    if m == 5:
        return 12 if d == 2 else 13
    return 14


def enumerate_orbits(g) -> np.ndarray:
    rp, col, _ = _rows(g)
    nv = rp.size - 1
    adj = [set(col[rp[v]:rp[v + 1]].tolist()) - {v} for v in range(nv)]
    out = np.zeros((15, nv), dtype=np.uint64)
    cnt = [[0] * nv for _ in range(15)]
    for v in range(nv):
        cnt[0][v] = len(adj[v])

    def leaf(sub):
        deg = [sum(1 for b in sub if b in adj[a]) for a in sub]
        m, mx = sum(deg) // 2, max(deg)
        if len(sub) == 3:
            for a, d in zip(sub, deg):
                cnt[3 if m == 3 else (2 if d == 2 else 1)][a] += 1
        else:
            for a, d in zip(sub, deg):
                cnt[_orbit(m, mx, d)][a] += 1

    def extend(sub, ext, root, k):
        if len(sub) == k - 1:
            for w in ext:
                leaf(sub + [w])
            return
        ext = set(ext)
        while ext:
            w = ext.pop()
            seen = set(sub)
            for a in sub:
                seen |= adj[a]
            extend(sub + [w], ext | {u for u in adj[w] if u > root and u not in seen}, root, k)

    for k in (3, 4):
        for v in range(nv):
            extend([v], {u for u in adj[v] if u > v}, v, k)
    for o in range(15):
        out[o] = np.array(cnt[o], dtype=np.uint64)
    return out


# ---- (b) composition ---------------------------------------------------------------------------------------------------------------------
def _u64(values) -> np.ndarray:
    return np.array([int(x) & M64 for x in values], dtype=np.uint64)


def diamond_term(g, sup) -> np.ndarray:
    """N12(v) = sum over the triangles {v, a, b} of t(ab) - 1, from the triangles: per entry (v, a) the common neighbours b, half the sum"""
    rp, col, src = _rows(g)
    nv = rp.size - 1
    x = {}
    for e, (u, a) in enumerate(zip(src.tolist(), col.tolist())):
        x[(u, a)] = int(sup[e]) - 1
    out = [0] * nv
    for v in range(nv):
        nb = col[rp[v]:rp[v + 1]]
        for a in nb.tolist():
            if a == v:
                continue
            for b in np.intersect1d(nb, col[rp[a]:rp[a + 1]], assume_unique=True).tolist():
                out[v] += x[(a, b)]
    assert all(s % 2 == 0 for s in out)
    return _u64(s // 2 for s in out)


def _c2(n):
    """C(n, 2) of a uint64 array below 2^32, exact"""
    n = np.asarray(n, dtype=np.uint64)
    return np.where(n < 2, 0, n * (n - np.uint64(1)) // np.uint64(2)).astype(np.uint64)


def compose_from(g, sup, rv, kv, n12, k=4) -> np.ndarray:
    """the orbits from t per entry (uint32), R_v, K_v and N12(v).  uint64 arrays: sums, differences and products wrap modulo 2^64 as the
    library's do; the three divisions (T_v, C(n, 2), C(d, 3)) act on values far below 2^64"""
    rp, col, src = _rows(g)
    nv = rp.size - 1
    u = np.uint64
    d = np.diff(rp).astype(u)
    assert int(d.max(initial=0)) < (1 << 21), "C(d, 3) is formed without wrapping"
    t = np.asarray(sup).astype(u)
    da = d[col]

    def rowsum(values):  # (rows are contiguous: differences of the running sum, exact modulo 2^64)
        cs = np.concatenate([np.zeros(1, dtype=u), np.cumsum(values, dtype=u)])
        return cs[rp[1:]] - cs[rp[:-1]]

    T = rowsum(t) // u(2)
    e1 = rowsum(da - u(1))
    o = [None] * 15
    o[0], o[3] = d, T
    o[2] = _c2(d) - T
    o[1] = e1 - u(2) * T
    if k == 4:
        R, K, n12 = (np.asarray(a, dtype=u) for a in (rv, kv, n12))
        N4 = rowsum(e1[col]) - d * (d - u(1)) - u(2) * T
        N5 = (d - u(1)) * e1 - u(2) * T
        N6 = rowsum(_c2(da - u(1)))
        N7 = np.where(d < 3, 0, d * (d - u(1)) * (d - u(2)) // u(6)).astype(u)
        N9 = rowsum(T[col]) - u(2) * T
        N10 = rowsum(t * (da - u(2)))
        N11 = T * (d - u(2))
        N13 = rowsum(_c2(t))
        # non-induced -> induced: a copy of a graphlet lies in every induced subgraph with at least its edges
        o[14] = K
        o[13] = N13 - u(3) * o[14]
        o[12] = n12 - u(3) * o[14]
        o[11] = N11 - u(2) * o[13] - u(3) * o[14]
        o[10] = N10 - u(2) * o[12] - u(2) * o[13] - u(6) * o[14]
        o[9] = N9 - u(2) * o[12] - u(3) * o[14]
        o[8] = R - o[12] - o[13] - u(3) * o[14]
        o[7] = N7 - o[11] - o[13] - o[14]
        o[6] = N6 - o[9] - o[10] - u(2) * o[12] - o[13] - u(3) * o[14]
        o[5] = N5 - u(2) * o[8] - o[10] - u(2) * o[11] - u(2) * o[12] - u(4) * o[13] - u(6) * o[14]
        o[4] = N4 - u(2) * o[8] - u(2) * o[9] - o[10] - u(4) * o[12] - u(2) * o[13] - u(6) * o[14]
    return np.stack([np.asarray(o[i], dtype=u) for i in range(N_ORBITS[k])])


def compose(g, k=4) -> np.ndarray:
    import clique_local_ref as KR
    import rect_local_ref as RR
    import truss_ref as TR

    sup = TR.supports(g)
    if k == 3:
        return compose_from(g, sup, None, None, None, k=3)
    return compose_from(g, sup, RR.rect_local(g)[1], KR.vertex_cliques(g, 4), diamond_term(g, sup))


def counts(orbits) -> list:
    """what gm_motif(k) returns, from the column sums (exact integers, then modulo 2^64)"""
    s = [int(sum(int(x) for x in row)) & M64 for row in orbits]
    if len(s) == 4:
        return [s[2], s[3] // 3]
    return [s[7], s[4] // 2, s[9], s[8] // 4, s[13] // 2, s[14] // 4]


# ---- the inputs of a dense graph from matrix products (K_n with sparse structure attached: the GPU tests' dense cells) ----------------------
def dense_inputs(g, core: int):
    """(t per entry, R_v, K_v, N12) of a graph whose vertices 0 .. core - 1 form a clique K_core and whose other vertices are adjacent to
    clique vertices only.  t, R_v and N12 come from float64 products of the dense adjacency matrix (every value below 2^53: exact).  K_v:
    an outside vertex x with the attachment set S_x lies in C(|S_x|, 3) 4-cliques, a clique vertex in C(core - 1, 3) plus
    C(|S_x| - 1, 2) for every x it is attached to (tests/test_motif_local_host.py checks this against clique_local_ref on a small one)."""
    rp, col, src = _rows(g)
    nv = rp.size - 1
    A = np.zeros((nv, nv), dtype=np.float64)
    A[src, col] = 1.0
    assert bool((A[:core, :core] + np.eye(core) == 1.0).all()), "vertices 0 .. core - 1 form a clique"
    assert not A[core:, core:].any(), "the outside vertices are adjacent to clique vertices only"
    A2 = A @ A
    t = A2[src, col]
    C2 = A2 * (A2 - 1.0) / 2.0
    np.fill_diagonal(C2, 0.0)
    rv = C2.sum(axis=1)  # (a 4-cycle at v has one vertex opposite v: a pair of their common neighbours)
    X = np.zeros_like(A)
    X[src, col] = t - 1.0
    n12 = np.einsum("va,av->v", A, X @ A) / 2.0
    assert max(float(A2.max()) ** 2, float(rv.max()), float(n12.max())) < 2.0 ** 53
    d = np.diff(rp)
    kv = np.zeros(nv, dtype=object)
    kv[:core] = comb(core - 1, 3)
    for x in range(core, nv):
        kv[x] = comb(int(d[x]), 3)
        kv[col[rp[x]:rp[x + 1]]] += comb(int(d[x]) - 1, 2)
    return t.astype(np.uint32), _u64(np.rint(rv).astype(np.int64)), _u64(kv), _u64(np.rint(n12).astype(np.int64))


def clique_with_satellites(core: int, n_out: int, seed: int, lo=2, hi=12):
    """K_core (vertices 0 .. core - 1) and n_out further vertices, each attached to a seeded random lo .. hi clique vertices: the clique's
    vertices and edges stop looking alike (degrees, supports and diamonds differ), the DAG rows stay those of K_core"""
    from planted_squares import _graph

    rng = np.random.default_rng(seed)
    iu = np.triu_indices(core, 1)
    s, d = [iu[0].astype(np.int64)], [iu[1].astype(np.int64)]
    for x in range(core, core + n_out):
        att = rng.choice(core, size=int(rng.integers(lo, hi + 1)), replace=False)
        s.append(att.astype(np.int64))
        d.append(np.full(att.size, x, dtype=np.int64))
    return _graph(core + n_out, np.concatenate(s), np.concatenate(d))


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def book_orbits(n) -> np.ndarray:
    """B_n, spine vertices 0 and 1, pages 2 .. n + 1 (triangles {0, 1, p}): the connected induced 4-subgraphs are the diamonds {0, 1, p, q},
    chord = the spine, and the 3-stars {s, p, q, r} around one spine vertex s"""
    out = np.zeros((15, n + 2), dtype=object)
    out[0, :2], out[0, 2:] = n + 1, 2
    out[3, :2], out[3, 2:] = n, 1
    # 2-paths: p - s - q (pages p != q around a spine vertex s) are induced: pages are not adjacent
    out[2, :2] = comb(n, 2)
    out[1, 2:] = 2 * (n - 1)
    # 4-subsets {0, 1, p, q}: diamonds, chord = the spine; {s, p, q, r}: 3-stars centred at the spine vertex s
    out[13, :2], out[12, 2:] = comb(n, 2), n - 1
    out[7, :2], out[6, 2:] = comb(n, 3), 2 * comb(n - 1, 2)
    return np.stack([_u64(r) for r in out])


def star_orbits(m) -> np.ndarray:
    """K_{1,m}, centre 0"""
    out = np.zeros((15, m + 1), dtype=object)
    out[0, 0], out[0, 1:] = m, 1
    out[2, 0], out[1, 1:] = comb(m, 2), m - 1
    out[7, 0], out[6, 1:] = comb(m, 3), comb(m - 1, 2)
    return np.stack([_u64(r) for r in out])
