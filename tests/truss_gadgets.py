"""The hub-edge gadget of the k-clique truss tests (test helper; shares no code with the library): a graph in which ONE edge with a long
list of surviving common neighbours leaves while everything else stays, each survivor with its own decrements.

  A    ids 0 .. a - 1: a seeded sparse G(a, p)
  Z1   ids a .. a + m - 1: a clique of m boosters, each joined to all of A;  Z2: ids a + m .. a + 2 m - 1, the same
  h1   a + 2 m, joined to all of A and of Z1;  h2 = h1 + 1, joined to all of A and of Z2;  h1 - h2 is the hub edge e
  hubs = 3: h3 = h2 + 1 and Z3 behind it, joined to h1 like h2 -- two hub edges (h1, h2), (h1, h3) that share a vertex and their survivors

With K_j(X) = the j-cliques of G[A] inside X (K_0 = 1, K_j = 0 for j < 0), A_w = A & N(w), A_wx = A_w & A_x and hubs = 2:
  K_e = K_{k-2}(A), S_e = A
  spoke (h, w):     sum_j K_j(A_w) C(m, k-2-j)                                   + K_{k-3}(A_w)   while e is there
  A-edge (w, x):    sum_j K_j(A_wx) (2 C(m, k-3-j) + f(k-2-j))                   + K_{k-4}(A_wx)  while e is there
                    f(0) = 1, f(t) = 2 C(m, t): t boosters, all of one side
  (z, w), z in Z:   sum_j K_j(A_w) C(m, k-2-j)
  (h, z), (z, z'):  sum_j K_j(A) C(m-1, k-2-j)
So with c = K_e + 1 the (k, c)-truss is everything but e, in two rounds, exactly when every other count exceeds K_e once e is gone:
expected() asserts that from the closed forms, before any library call, and booster() finds the smallest m for which it holds.
book(t, k): t pages on one spine edge -- thousands of decrements that land on one counter."""
from __future__ import annotations

from math import comb

import numpy as np

from clique_local_ref import _count
from core_gadgets import _a_bitsets, _a_edges

REMOVED = 0xFFFFFFFFFFFFFFFF


def hub_edge_gadget(a: int, p: float, m: int, seed: int, hubs: int = 2):
    from graphminer_amd.rmat import csr_from_pairs

    assert hubs in (2, 3)
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
    """the closed forms of one (a, p, seed, k), for any m"""

    def __init__(self, a: int, p: float, seed: int, k: int):
        self.a, self.k = a, k
        nbr = _a_bitsets(a, p, seed)

        def kj(s):
            return [_count(nbr, s, j) for j in range(k - 1)]  # K_0 .. K_{k-2}

        self.ka = kj((1 << a) - 1)
        self.kw = [kj(nbr[w]) for w in range(a)]
        self.kwx = {(w, x): kj(nbr[w] & nbr[x]) for w in range(a) for x in range(w + 1, a) if (nbr[w] >> x) & 1}
        self.k_e = self.ka[k - 2]

    def values(self, m: int):
        k = self.k

        def c(n, t):
            return comb(n, t) if t >= 0 else 0

        def f(t):
            return 0 if t < 0 else 1 if t == 0 else 2 * comb(m, t)

        side = [sum(kw[j] * c(m, k - 2 - j) for j in range(k - 1)) for kw in self.kw]  # spokes once e is gone, and (z, w)
        inner = {e: sum(kx[j] * (2 * c(m, k - 3 - j) + f(k - 2 - j)) for j in range(k - 1)) for e, kx in self.kwx.items()}
        booster = sum(self.ka[j] * c(m - 1, k - 2 - j) for j in range(k - 1))  # (h, z) and (z, z')
        return side, inner, booster

    def valid(self, m: int) -> bool:
        side, inner, booster = self.values(m)
        return m >= 2 and min(side + list(inner.values()) + [booster]) > self.k_e


def booster(a: int, p: float, seed: int, k: int) -> int:
    """the smallest m at which the hub edge is the strict minimum and everything else outlasts it (every count grows with m)"""
    forms = _Forms(a, p, seed, k)
    hi = 2
    while not forms.valid(hi):
        hi *= 2
    lo = hi // 2  # (not valid, or 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if forms.valid(mid) else (mid, hi)
    return hi


def expected(g, a: int, p: float, m: int, seed: int, k: int) -> dict:
    """what gm_clique_ktruss gives on g = hub_edge_gadget(a, p, m, seed) at c = K_e + 1: {"c", "cnt" (np.uint64[ne], REMOVED at both entries of
    e), "edges", "cliques", "rounds", "spoke_decrements", "pair_decrements" (the distinct amounts the spokes and the edges of A lose)};
    asserts the gadget's preconditions"""
    forms = _Forms(a, p, seed, k)
    side, inner, boost = forms.values(m)
    k_e, c = forms.k_e, forms.k_e + 1
    lost_w = [kw[k - 3] if k >= 3 else 0 for kw in forms.kw]
    lost_wx = {e: (kx[k - 4] if k >= 4 else 0) for e, kx in forms.kwx.items()}
    least_after = min(side + list(inner.values()) + [boost])
    print(f"hub-edge gadget a={a} p={p} m={m} k={k}: K_e={k_e}, the smallest other count once e is gone {least_after}, "
          f"{len(set(lost_w))} distinct spoke decrements, {len(set(lost_wx.values()))} distinct pair decrements", flush=True)
    assert least_after > k_e, "e must be the strict minimum and everything else must outlast it: raise m"
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    src = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    dst = np.asarray(g.col_idx, dtype=np.int64)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    h1 = a + 2 * m
    assert rp.size - 1 == h1 + 2
    cnt = np.full(dst.size, boost, dtype=object)  # (h, z), (z, z')
    touches_a = lo < a
    cnt[touches_a & (hi >= a)] = np.array(side, dtype=object)[lo[touches_a & (hi >= a)]]  # spokes and (z, w)
    inner_at = np.flatnonzero(hi < a)
    for i in inner_at.tolist():
        cnt[i] = inner[(int(lo[i]), int(hi[i]))]
    cnt[(lo == h1) & (hi == h1 + 1)] = REMOVED
    edges = dst.size // 2 - 1
    total = sum(int(x) for x in cnt[(src < dst) & (cnt != REMOVED)])
    assert total % comb(k, 2) == 0
    return {"c": c, "cnt": cnt.astype(np.uint64), "edges": edges, "cliques": total // comb(k, 2), "rounds": 2,
            "spoke_decrements": sorted(set(lost_w)), "pair_decrements": sorted(set(lost_wx.values()))}
