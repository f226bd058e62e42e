"""The hub gadget of the k-clique core tests (test helper; shares no code with the library): a graph in which ONE vertex with a long surviving
neighbourhood leaves while all its neighbours stay, each with a different decrement.

  A   ids 0 .. a - 1: a seeded sparse G(a, p)
  Z   ids a .. a + m - 1: a clique of m boosters, each joined to all of A
  h   the highest id(s): a hub joined to all of A and to none of Z; hubs = 2: h1 < h2, adjacent, both joined to all of A

With K_j(X) = the j-cliques inside the vertex set X (K_0 = 1) and A_w = A & N(w):
  K(h)  = K_{k-1}(A)                                (two hubs: + K_{k-2}(A), the cliques that hold both; the two counts are equal)
  after the hubs are gone:  K_w = sum_j K_j(A_w) C(m, k-1-j)  for w in A,   K_z = sum_j K_j(A) C(m-1, k-1-j)  for z in Z,  j = 0 .. k-1
  before:  K_w + K_{k-2}(A_w)                       (two hubs: + 2 K_{k-2}(A_w) + K_{k-3}(A_w))
So with c = K(h) + 1 the (k, c)-core is A + Z exactly when every count before exceeds K(h) -- the hubs leave alone, in one round -- and
every count after reaches c: expected() asserts both from the closed forms, before any library call.  The booster clique makes the plain
reference too slow; the closed forms only count inside A.
windmill(t) and star(n): thousands of decrements that land on one counter."""
from __future__ import annotations

from math import comb

import numpy as np

from clique_local_ref import _count

REMOVED = 0xFFFFFFFFFFFFFFFF


def _a_edges(a: int, p: float, seed: int):
    """the edges u < v of the seeded G(a, p)"""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(a, 1)
    keep = rng.random(iu.size) < p
    return iu[keep].astype(np.int64), ju[keep].astype(np.int64)


def _a_bitsets(a: int, p: float, seed: int) -> list:
    nbr = [0] * a
    for u, v in zip(*(x.tolist() for x in _a_edges(a, p, seed))):
        nbr[u] |= 1 << v
        nbr[v] |= 1 << u
    return nbr


def hub_gadget(a: int, p: float, m: int, seed: int, hubs: int = 1):
    """the graph: A, then Z, then the hub(s)"""
    from graphminer_amd.rmat import csr_from_pairs

    assert hubs in (1, 2)
    src, dst = _a_edges(a, p, seed)
    ids_a, ids_z, ids_h = np.arange(a), np.arange(a, a + m), np.arange(a + m, a + m + hubs)
    zi, zj = np.triu_indices(m, 1)
    parts_s = [src, np.repeat(ids_z, a), ids_z[zi], np.repeat(ids_h, a)]
    parts_d = [dst, np.tile(ids_a, m), ids_z[zj], np.tile(ids_a, hubs)]
    if hubs == 2:
        parts_s.append(ids_h[:1])
        parts_d.append(ids_h[1:])
    s, d = np.concatenate(parts_s).astype(np.uint64), np.concatenate(parts_d).astype(np.uint64)
    return csr_from_pairs(a + m + hubs, s, d)


def windmill(t: int):
    """t triangles on one centre: the centre is vertex 0, triangle i holds 2 i + 1 and 2 i + 2"""
    from graphminer_amd.rmat import csr_from_pairs

    x = 2 * np.arange(t, dtype=np.int64) + 1
    zero = np.zeros(t, dtype=np.int64)
    return csr_from_pairs(2 * t + 1, np.concatenate([zero, zero, x]).astype(np.uint64), np.concatenate([x, x + 1, x + 1]).astype(np.uint64))


def star(leaves: int):
    """vertex 0 joined to `leaves` others"""
    from graphminer_amd.rmat import csr_from_pairs

    return csr_from_pairs(leaves + 1, np.zeros(leaves, dtype=np.uint64), np.arange(1, leaves + 1, dtype=np.uint64))


def expected(a: int, p: float, m: int, seed: int, k: int, hubs: int = 1) -> dict:
    """what gm_clique_kcore gives at c = K(h) + 1: {"c", "cnt" (np.uint64[nv], REMOVED at the hubs), "vertices", "cliques", "rounds",
    "decrements" (the distinct amounts the members of A lose)}; asserts the gadget's preconditions"""
    nbr = _a_bitsets(a, p, seed)
    all_a = (1 << a) - 1

    def kj(s, j):
        return 0 if j < 0 else _count(nbr, s, j)

    ka = [kj(all_a, j) for j in range(k)]
    k_hub = ka[k - 1] + (ka[k - 2] if hubs == 2 else 0)
    c = k_hub + 1
    after, before = [], []
    for w in range(a):
        kw = [kj(nbr[w], j) for j in range(k)]
        aft = sum(kw[j] * comb(m, k - 1 - j) for j in range(k))
        lost = kw[k - 2] if hubs == 1 else 2 * kw[k - 2] + (kw[k - 3] if k >= 3 else 0)
        after.append(aft)
        before.append(aft + lost)
    k_z = sum(ka[j] * comb(m - 1, k - 1 - j) for j in range(k))
    decrements = sorted({b - x for b, x in zip(before, after)})
    print(f"gadget a={a} p={p} m={m} k={k} hubs={hubs}: K(h)={k_hub} min before {min(before + [k_z])} min after {min(after + [k_z])} "
          f"{len(decrements)} distinct decrements", flush=True)
    assert min(before + [k_z]) > k_hub, "the hubs must leave alone: raise m"
    assert min(after + [k_z]) >= c, "all of A and Z must survive: raise m"
    cnt = np.array(after + [k_z] * m + [REMOVED] * hubs, dtype=np.uint64)
    total = sum(after) + k_z * m
    assert total % k == 0
    return {"c": c, "cnt": cnt, "vertices": a + m, "cliques": total // k, "rounds": 2, "decrements": decrements}
