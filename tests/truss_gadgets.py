"""The hub-edge gadget of the k-clique truss tests (test helper; shares no code with the library): a graph in which ONE edge with a long
list of surviving common neighbours leaves while everything else stays, each survivor with its own decrements.

  A    ids 0 .. a - 1: a seeded sparse G(a, p)
  Z1   ids a .. a + m - 1: a clique of m boosters, each joined to all of A;  Z2: ids a + m .. a + 2 m - 1, the same
  h1   a + 2 m, joined to all of A and of Z1;  h2 = h1 + 1, joined to all of A and of Z2;  h1 - h2 is the hub edge e
  hubs = 3: h3 = h2 + 1 and Z3 behind it, joined to h1 like h2 -- two hub edges (h1, h2), (h1, h3) that share a vertex and their survivors
  triangle: hubs = 3 and the edge (h2, h3) too -- three hub edges of K_{k-2}(A) + K_{k-3}(A) each, one frontier; (h1, h2), the lowest entry,
            keeps h3 among its survivors, the other two find an edge to their third hub blocked

With K_j(X) = the j-cliques of G[A] inside X (K_0 = 1, K_j = 0 for j < 0), A_w = A & N(w), A_wx = A_w & A_x and hubs = 2:
  K_e = K_{k-2}(A), S_e = A
  spoke (h, w):     sum_j K_j(A_w) C(m, k-2-j)                                   + K_{k-3}(A_w)   while e is there
  A-edge (w, x):    sum_j K_j(A_wx) g(k-2-j)                                     + K_{k-4}(A_wx)  while e is there
                    g(0) = 1, g(t) = hubs C(m + 1, t): t of the m + 1 members of one side, its boosters and its hub
  (z, w), z in Z:   sum_j K_j(A_w) C(m, k-2-j)
  (h, z), (z, z'):  sum_j K_j(A) C(m-1, k-2-j)
So with c = K_e + 1 the (k, c)-truss is everything but e, in two rounds, exactly when every other count exceeds K_e once e is gone:
expected() asserts that from the closed forms, before any library call, and booster() finds the smallest m for which it holds.
Once the hub edges are gone the forms do not depend on how many hubs there were, but for g.
split_hub_edge_gadget(a, p, q, m, seed): the hub edge AND a set X of edges among its survivors in one frontier (its docstring).
book(t, k): t pages on one spine edge -- thousands of decrements that land on one counter."""
from __future__ import annotations

import functools
from math import comb

import numpy as np

from clique_local_ref import _count
from core_gadgets import _a_bitsets, _a_edges

REMOVED = 0xFFFFFFFFFFFFFFFF


def hub_edge_gadget(a: int, p: float, m: int, seed: int, hubs: int = 2, triangle: bool = False):
    from graphminer_amd.rmat import csr_from_pairs

    assert hubs in (2, 3) and (hubs == 3 or not triangle)
    src, dst = _a_edges(a, p, seed)
    ids_a = np.arange(a)
    zi, zj = np.triu_indices(m, 1)
    parts_s, parts_d = [src], [dst]
    for i in range(hubs):
        ids_z, h = np.arange(a + i * m, a + (i + 1) * m), a + hubs * m + i
        parts_s += [np.repeat(ids_z, a), ids_z[zi], np.full(a, h), np.full(m, h)]
        parts_d += [np.tile(ids_a, m), ids_z[zj], ids_a, ids_z]
    h1 = a + hubs * m
    parts_s.append(np.full(hubs - 1, h1))
    parts_d.append(np.arange(h1 + 1, h1 + hubs))
    if triangle:
        parts_s.append(np.array([h1 + 1]))
        parts_d.append(np.array([h1 + 2]))
    s, d = np.concatenate(parts_s).astype(np.uint64), np.concatenate(parts_d).astype(np.uint64)
    return csr_from_pairs(a + hubs * m + hubs, s, d)


def book(t: int, k: int):
    """the spine edge (0, 1) and t pages on it, a page = a (k - 2)-clique joined to both ends of the spine (k = 3: a vertex, k = 4: an edge)"""
    from graphminer_amd.rmat import csr_from_pairs

    q = k - 2
    first = 2 + q * np.arange(t, dtype=np.int64)
    src, dst = [np.zeros(1, np.int64)], [np.ones(1, np.int64)]
    for i in range(q):
        src += [np.zeros(t, np.int64), np.ones(t, np.int64)]
        dst += [first + i, first + i]
        for j in range(i + 1, q):
            src.append(first + i)
            dst.append(first + j)
    return csr_from_pairs(2 + q * t, np.concatenate(src).astype(np.uint64), np.concatenate(dst).astype(np.uint64))


class _Forms:
    """the closed forms of one (a, p, seed, k), for any m; nbr: the bitsets of G[A] given outright (a, p, seed unused)"""

    def __init__(self, a: int, p: float, seed: int, k: int, hubs: int = 2, triangle: bool = False, nbr: list = None):
        nbr = _a_bitsets(a, p, seed) if nbr is None else nbr
        self.a, self.k, self.hubs = len(nbr), k, hubs
        a = self.a

        def kj(s):
            return [_count(nbr, s, j) for j in range(k - 1)]  # K_0 .. K_{k-2}

        self.ka = kj((1 << a) - 1)
        self.kw = [kj(nbr[w]) for w in range(a)]
        self.kwx = {(w, x): kj(nbr[w] & nbr[x]) for w in range(a) for x in range(w + 1, a) if (nbr[w] >> x) & 1}
        # a hub edge: the (k-2)-cliques of A, and with the third hub of a triangle among the common neighbours those of A + that hub
        self.k_e = self.ka[k - 2] + (self.ka[k - 3] if triangle else 0)

    def values(self, m: int):
        k = self.k

        def c(n, t):
            return comb(n, t) if t >= 0 else 0

        def g(t):
            return 0 if t < 0 else 1 if t == 0 else self.hubs * comb(m + 1, t)

        side = [sum(kw[j] * c(m, k - 2 - j) for j in range(k - 1)) for kw in self.kw]  # spokes once e is gone, and (z, w)
        inner = {e: sum(kx[j] * g(k - 2 - j) for j in range(k - 1)) for e, kx in self.kwx.items()}
        booster = sum(self.ka[j] * c(m - 1, k - 2 - j) for j in range(k - 1))  # (h, z) and (z, z')
        return side, inner, booster

    def least(self, m: int) -> int:
        side, inner, booster = self.values(m)
        return min(side + list(inner.values()) + [booster])

    def valid(self, m: int) -> bool:
        return m >= 2 and self.least(m) > self.k_e


@functools.lru_cache(maxsize=8)
def _forms(a: int, p: float, seed: int, k: int, hubs: int = 2, triangle: bool = False) -> _Forms:
    return _Forms(a, p, seed, k, hubs, triangle)


def _smallest_valid(forms) -> int:
    hi = 2
    while not forms.valid(hi):
        hi *= 2
    lo = hi // 2  # (not valid, or 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if forms.valid(mid) else (mid, hi)
    return hi


def booster(a: int, p: float, seed: int, k: int, hubs: int = 2, triangle: bool = False) -> int:
    """the smallest m at which the hub edge is the strict minimum and everything else outlasts it (every count grows with m)"""
    return _smallest_valid(_forms(a, p, seed, k, hubs, triangle))


def a_edges_from(a: int, p: float, seed: int, pos: int) -> tuple:
    """(the edges of G[A] with the higher end at position pos of S_e = A or beyond, those with both ends there)"""
    src, dst = _a_edges(a, p, seed)  # (src < dst)
    return int((dst >= pos).sum()), int((src >= pos).sum())


def _ends(g):
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    src = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    dst = np.asarray(g.col_idx, dtype=np.int64)
    return src, dst, np.minimum(src, dst), np.maximum(src, dst)


def _result(k: int, c: int, cnt, src, dst, gone: int, **more) -> dict:
    total = sum(int(x) for x in cnt[(src < dst) & (cnt != REMOVED)])
    assert total % comb(k, 2) == 0
    return {"c": c, "cnt": cnt.astype(np.uint64), "edges": dst.size // 2 - gone, "cliques": total // comb(k, 2), "rounds": 2, **more}


def expected(g, a: int, p: float, m: int, seed: int, k: int, hubs: int = 2, triangle: bool = False) -> dict:
    """what gm_clique_ktruss gives on g = hub_edge_gadget(a, p, m, seed, hubs, triangle) at c = K_e + 1: {"c", "cnt" (np.uint64[ne], REMOVED
    at both entries of every hub edge), "edges", "cliques", "rounds", "spoke_decrements", "pair_decrements" (the distinct amounts the spokes
    and the edges of A lose to one hub edge)}; asserts the gadget's preconditions"""
    forms = _forms(a, p, seed, k, hubs, triangle)
    side, inner, boost = forms.values(m)
    k_e, c = forms.k_e, forms.k_e + 1
    lost_w = [kw[k - 3] if k >= 3 else 0 for kw in forms.kw]
    lost_wx = {e: (kx[k - 4] if k >= 4 else 0) for e, kx in forms.kwx.items()}
    least_after = min(side + list(inner.values()) + [boost])
    print(f"hub-edge gadget a={a} p={p} m={m} k={k} hubs={hubs}{' in a triangle' if triangle else ''}: K_e={k_e}, the smallest other count "
          f"once the hub edges are gone {least_after}, {len(set(lost_w))} distinct spoke decrements, {len(set(lost_wx.values()))} distinct "
          f"pair decrements", flush=True)
    assert least_after > k_e, "the hub edges must be the strict minimum and everything else must outlast them: raise m"
    src, dst, lo, hi = _ends(g)
    h1 = a + hubs * m
    assert g.V() == h1 + hubs
    cnt = np.full(dst.size, boost, dtype=object)  # (h, z), (z, z')
    touches_a = lo < a
    cnt[touches_a & (hi >= a)] = np.array(side, dtype=object)[lo[touches_a & (hi >= a)]]  # spokes and (z, w)
    inner_at = np.flatnonzero(hi < a)
    for i in inner_at.tolist():
        cnt[i] = inner[(int(lo[i]), int(hi[i]))]
    hub_edges = lo >= h1
    assert int(hub_edges.sum()) == 2 * (3 if triangle else hubs - 1)
    cnt[hub_edges] = REMOVED
    return _result(k, c, cnt, src, dst, int(hub_edges.sum()) // 2, spoke_decrements=sorted(set(lost_w)),
                   pair_decrements=sorted(set(lost_wx.values())))


# ---- the split gadget: the hub edge and a set of edges among its survivors in ONE frontier ---------------------------------------------------
def _split_parts(a: int, p: float, q: float, seed: int):
    """(src, dst of the edges inside the halves, src, dst of X): the seeded G(a, p) without its pairs of unequal parity; X = about q a of
    those pairs drawn by a second seeded stream, and the pair (0 or 1, a - 1) -- the first and the last word of the matrix of S_e = A"""
    src, dst = _a_edges(a, p, seed)
    same = (src & 1) == (dst & 1)
    iu, ju = np.triu_indices(a, 1)
    cross = np.flatnonzero((iu & 1) != (ju & 1))
    pick = np.sort(np.random.default_rng([seed, 1]).choice(cross, size=max(8, round(q * a)), replace=False))
    first = 1 - ((a - 1) & 1)
    xs, xd = np.append(iu[pick], first), np.append(ju[pick], a - 1)
    pairs = np.unique(np.stack([xs, xd], axis=1), axis=0)  # (the forced pair may have been drawn)
    return src[same], dst[same], pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)


def split_hub_edge_gadget(a: int, p: float, q: float, m: int, seed: int):
    """A = L + R, the even and the odd ids of 0 .. a - 1 (so that the pairs across fall in every word of the matrix), a seeded sparse G(., p)
    inside each half, and X: about q a seeded edges across, each from L to R.
      Z1L, Z2L, Z1R, Z2R   ids a + i m .. a + (i + 1) m - 1, i = 0 .. 3: four cliques of m boosters; Z.L joined to all of L, Z.R to all of R
      h1 = a + 4 m         joined to A, Z1L and Z1R;  h2 = h1 + 1: joined to A, Z2L and Z2R;  e = (h1, h2)
    An edge (w, x) of X has the common neighbours {h1, h2} + A_w & A_x and no booster: its count is tiny.  With c = K_e + 1 the first frontier
    is e and all of X; the edges of X lie at lower canonical entries than e and their four spokes are alive, so ONLY the pair filter of the
    matrix keeps e from accounting the cliques {w, x, h1, h2, ..} that the edges of X account.  G' = G - e - X is two one-sided hub-edge
    gadgets, on L and on R, that share the two hubs and no clique: the closed forms of _Forms per side."""
    from graphminer_amd.rmat import csr_from_pairs

    src, dst, xs, xd = _split_parts(a, p, q, seed)
    ids = (np.arange(0, a, 2), np.arange(1, a, 2))
    zi, zj = np.triu_indices(m, 1)
    h1 = a + 4 * m
    parts_s, parts_d = [src, xs, np.array([h1])], [dst, xd, np.array([h1 + 1])]
    for i in range(4):
        ids_z, half, h = np.arange(a + i * m, a + (i + 1) * m), ids[i // 2], h1 + (i & 1)
        parts_s += [np.repeat(ids_z, half.size), ids_z[zi], np.full(m, h)]
        parts_d += [np.tile(half, m), ids_z[zj], ids_z]
    for h in (h1, h1 + 1):
        parts_s.append(np.full(a, h))
        parts_d.append(np.arange(a))
    s, d = np.concatenate(parts_s).astype(np.uint64), np.concatenate(parts_d).astype(np.uint64)
    return csr_from_pairs(h1 + 2, s, d)


class _SplitForms:
    """the closed forms of one split gadget (a, p, q, seed, k), for any m: K_e and the counts of X in G, _Forms per half for G'"""

    def __init__(self, a: int, p: float, q: float, seed: int, k: int):
        src, dst, xs, xd = _split_parts(a, p, q, seed)
        self.a, self.k, self.x = a, k, list(zip(xs.tolist(), xd.tolist()))
        inside = [0] * a
        for u, v in zip(src.tolist(), dst.tolist()):
            inside[u] |= 1 << v
            inside[v] |= 1 << u
        full = list(inside)
        for u, v in self.x:
            full[u] |= 1 << v
            full[v] |= 1 << u

        def half(par):  # the bitsets of G[half], the member of id 2 i + par renumbered i
            return [sum(1 << (v >> 1) for v in range(par, a, 2) if (inside[w] >> v) & 1) for w in range(par, a, 2)]

        def kj(s, j):
            return _count(full, s, j) if j >= 0 else 0

        self.sides = [_Forms(0, 0.0, 0, k, nbr=half(par)) for par in (0, 1)]
        self.k_e = kj((1 << a) - 1, k - 2)
        # an edge of X: the (k-2)-cliques of its common neighbours, A_wx with none, one or both of the adjacent hubs
        self.x_counts = [kj(full[w] & full[x], k - 2) + 2 * kj(full[w] & full[x], k - 3) + kj(full[w] & full[x], k - 4) for w, x in self.x]

    def least(self, m: int) -> int:
        return min(f.least(m) for f in self.sides)

    def valid(self, m: int) -> bool:
        return m >= 2 and self.least(m) > self.k_e


@functools.lru_cache(maxsize=8)
def _split_forms(a: int, p: float, q: float, seed: int, k: int) -> _SplitForms:
    return _SplitForms(a, p, q, seed, k)


def split_booster(a: int, p: float, q: float, seed: int, k: int) -> int:
    """booster() for the split gadget: the smallest m at which everything but e and X outlasts K_e in G'"""
    return _smallest_valid(_split_forms(a, p, q, seed, k))


def split_expected(g, a: int, p: float, q: float, m: int, seed: int, k: int) -> dict:
    """expected() for g = split_hub_edge_gadget(a, p, q, m, seed): REMOVED at both entries of e and of every edge of X, everywhere else the
    count in G' by the closed forms of the entry's half; also "x" = |X|, "x_most" = the largest count of X in G, "x_words" = the matrix words
    of the two ends of the forced pair, "words" = the words of a row; "spoke_decrements": what the spokes lose to e, the distinct
    K_{k-3}(A_w) in G'.  Asserts the gadget's preconditions, all of them arithmetic"""
    forms = _split_forms(a, p, q, seed, k)
    k_e, c = forms.k_e, forms.k_e + 1
    vals = [f.values(m) for f in forms.sides]
    least_after, x_most = forms.least(m), max(forms.x_counts)
    lost_w = sorted({kw[k - 3] for f in forms.sides for kw in f.kw})
    forced = (1 - ((a - 1) & 1), a - 1)
    print(f"split gadget a={a} p={p} q={q} m={m} k={k}: K_e={k_e}, |X|={len(forms.x)} with counts up to {x_most}, the smallest other count in "
          f"G' {least_after}, {len(lost_w)} distinct spoke decrements, the pair {forced} in X: {forced in forms.x}", flush=True)
    assert x_most < c, "every edge of X must enter the first frontier"
    assert least_after >= c, "everything but e and X must outlast them: raise m"
    assert len(forms.x) >= 8 and all((w ^ x) & 1 and w < x < a for w, x in forms.x)
    assert forced in forms.x and forced[0] >> 5 == 0 and forced[1] >> 5 == (a - 1) >> 5, "a pair of X over the first and the last word of a row"
    assert k < 4 or len(lost_w) >= 3, "at least three distinct spoke decrements"
    src, dst, lo, hi = _ends(g)
    h1 = a + 4 * m
    assert g.V() == h1 + 2
    cnt = np.empty(dst.size, dtype=object)
    par = np.where(lo < a, lo & 1, np.minimum((lo - a) // m, 3) // 2)  # the half of the entry's lower end: an id of A, or a booster's clique
    for s in (0, 1):
        side, inner, boost = vals[s]
        cnt[(par == s) & (lo >= a)] = boost  # (h, z), (z, z')
        sel = (par == s) & (lo < a) & (hi >= a)
        cnt[sel] = np.array(side, dtype=object)[lo[sel] >> 1]  # spokes and (z, w)
        for i in np.flatnonzero((par == s) & (hi < a) & ((hi & 1) == s)).tolist():
            cnt[i] = inner[(int(lo[i]) >> 1, int(hi[i]) >> 1)]
    gone = ((hi < a) & (((lo ^ hi) & 1) == 1)) | (lo == h1)  # X and e
    assert int(gone.sum()) == 2 * (len(forms.x) + 1)
    cnt[gone] = REMOVED
    return _result(k, c, cnt, src, dst, len(forms.x) + 1, x=len(forms.x), x_most=x_most, x_words=(forced[0] >> 5, forced[1] >> 5),
                   words=(a + 31) >> 5, spoke_decrements=lost_w)




# ---- the cells of tests/test_gpu_clique_truss.py whose preconditions tests/test_clique_truss_host.py asserts without a GPU ------------------
def split_cells(rc: dict) -> list:
    """(a, p, q, k): |S_e| = a one past each boundary of the peel's paths (rc: common.kcl_row_constants()); the last is the wide kernel's"""
    return [(rc["regs2"] + 1, 0.2, 0.25, 4), (rc["regs2"] + 1, 0.3, 0.25, 5), (rc["regs8"] + 1, 0.1, 0.25, 4), (rc["regs12"] + 1, 0.07, 0.25, 4),
            (rc["lds"] + 1, 0.05, 0.25, 4)]


def triangle_cells(rc: dict) -> list:
    """(a, p, k): the three hubs in a triangle, on the workgroup path and in the wide kernel"""
    return [(rc["regs2"] + 1, 0.2, 3), (rc["regs2"] + 1, 0.2, 4), (rc["lds"] + 1, 0.05, 3), (rc["lds"] + 1, 0.05, 4)]


def second_group_cells(rc: dict) -> list:
    """(a, p, k): hub-edge gadgets whose matrix rows have more than 64 words -- position `lanes` is the first of the wide pair walk's second
    group of words; at a = lanes + 65 the positions from `lanes` on have pairs among themselves"""
    return [(rc["lanes"] + 1, 0.004, 4), (rc["lanes"] + 65, 0.004, 4)]


def long_row_cell(rc: dict) -> tuple:
    """(a, p, k, the least m): the workgroup path with 2 a boosters or more behind each hub -- every survivor's row, its 2 m boosters and the
    two hubs at least, is longer than 4 |S_e| = 4 a, so the pair walk streams S_e against the row"""
    return rc["regs2"] + 1, 0.2, 4, 2 * (rc["regs2"] + 1)
