"""Graphs made of twin classes, whose match counts are known exactly at any size (test helper, imported by the twin-graph tests).

A twin class is a set of vertices with the same neighbours outside the set: independent (false twins) or a clique (true twins). Any
permutation inside a class is an automorphism, so the number of copies of a pattern P is sum_j C(n, j) N_j over the class size n, with
N_j independent of n: a polynomial in n of degree at most |V(P)|. Its value at n = 65 K follows exactly from oracle counts at |V(P)| + 1
small sizes (Lagrange interpolation in rationals, asserted integral). Numbering does not change a count.

Families (params; the LAST one is the size that interpolation varies):
  kab          (a, b)  complete bipartite K_{a,b}: ids 0 .. a-1 the a side, a .. a+b-1 the b side
  book         (n,)    book B_n: spine edge 0-1, pages 2 .. n+1 joined to both spine ends
  split        (a, b)  S_{a,b}: a K_a (ids 0 .. a-1), b false twins joined to all of it, a pendant 3-path a+b - a+b+1 - a+b+2 on vertex 0
  complete     (n,)    K_n, one class of true twins
  multipartite (r, s)  complete multipartite K_{s x r}: r independent parts of s ids each (part of id i: i // s)

`what`: tc, diamond, rectangle, house, pentagon, tailedtriangle, 4path, 3star, clique<k> (k >= 3), motif3 (a list of 2) and motif4 (a
list of 6), as the CPU oracle orders them. The oracle is the source of truth; the closed forms of CLOSED are shortcuts it confirms
(tests/test_twin_reference.py)."""
from __future__ import annotations

import functools
from fractions import Fraction
from math import comb

import numpy as np

import oracle as O

FAMILIES = ("kab", "book", "split", "complete", "multipartite")
SGL = ("tc", "diamond", "rectangle", "house", "pentagon", "tailedtriangle", "4path", "3star", "motif3", "motif4")


def pattern_size(what: str) -> int:
    """|V(P)|: the degree bound of a count as a polynomial in a class size"""
    if what.startswith("clique"):
        return int(what[6:])
    return {"tc": 3, "motif3": 3, "house": 5, "pentagon": 5}.get(what, 4)


def pairs(family: str, params) -> tuple[int, np.ndarray, np.ndarray]:
    """(number of vertices, edge sources, edge destinations) on the family's natural ids"""
    s, d = [], []
    if family == "kab":
        a, b = params
        n = a + b
        s.append(np.repeat(np.arange(a), b))
        d.append(np.tile(np.arange(a, n), a))
    elif family == "book":
        (m,) = params
        n = m + 2
        pages = np.arange(2, n)
        s += [np.array([0]), np.zeros(m, np.int64), np.ones(m, np.int64)]
        d += [np.array([1]), pages, pages]
    elif family == "split":
        a, b = params
        n = a + b + 3
        iu, ju = np.triu_indices(a, 1)
        s += [iu, np.repeat(np.arange(a), b), np.array([0, a + b, a + b + 1])]
        d += [ju, np.tile(np.arange(a, a + b), a), np.array([a + b, a + b + 1, a + b + 2])]
    elif family == "complete":
        (n,) = params
        iu, ju = np.triu_indices(n, 1)
        s.append(iu)
        d.append(ju)
    elif family == "multipartite":
        r, sz = params
        n = r * sz
        iu, ju = np.triu_indices(n, 1)
        keep = iu // sz != ju // sz
        s.append(iu[keep])
        d.append(ju[keep])
    else:
        raise ValueError(family)
    return n, np.concatenate(s).astype(np.int64), np.concatenate(d).astype(np.int64)


def numbering(n: int, src: np.ndarray, dst: np.ndarray, order: str = "natural", seed: int = 0) -> np.ndarray:
    """new id of every natural id: "natural"; "degree" (ascending degree, the hubs get the top ids); "hubs_first" (descending);
    "random" (a seeded permutation)"""
    if order == "natural":
        return np.arange(n, dtype=np.int64)
    if order == "random":
        return np.random.default_rng(seed).permutation(n).astype(np.int64)
    deg = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    rank = np.argsort(deg if order == "degree" else -deg, kind="stable")
    if order not in ("degree", "hubs_first"):
        raise ValueError(order)
    new = np.empty(n, dtype=np.int64)
    new[rank] = np.arange(n)
    return new


def graph(family: str, params, order: str = "natural", seed: int = 0, nv: int | None = None, offset: int = 0):
    """the graph as a graphminer_amd Graph: ids placed by `order`, then shifted by `offset` inside an id space of `nv` vertices (default:
    just the graph's own); the ids outside the block are isolated"""
    from graphminer_amd.rmat import csr_from_pairs

    n, s, d = pairs(family, params)
    nv = n if nv is None else nv
    assert 0 <= offset and offset + n <= nv
    new = numbering(n, s, d, order, seed) + offset
    return csr_from_pairs(nv, new[s].astype(np.uint64), new[d].astype(np.uint64))


def top_offset(family: str, params, nv: int) -> int:
    """the offset that puts the family's last id at nv - 1"""
    return nv - pairs(family, params)[0]


def oracle_count(g, what: str):
    """the CPU oracle's count of `what` on a graphminer_amd Graph"""
    sym = O.OGraph(g.row_ptr, g.col_idx)
    if what == "tc" or what.startswith("clique"):
        dag = O.orient(sym)
        return O.tc(dag) if what in ("tc", "clique3") else O.clique(dag, int(what[6:]))
    fn = {"diamond": O.diamond, "rectangle": O.rectangle, "house": O.house, "pentagon": O.pentagon, "tailedtriangle": O.tailedtriangle,
          "4path": O.path4, "3star": O.star3, "motif3": O.motif3, "motif4": O.motif4}[what]
    return fn(sym)


# closed forms, each confirmed against the oracle (tests/test_twin_reference.py)
CLOSED = {
    "kab": {
        "tc": lambda a, b: 0, "diamond": lambda a, b: 0, "house": lambda a, b: 0, "pentagon": lambda a, b: 0,
        "tailedtriangle": lambda a, b: 0,
        "rectangle": lambda a, b: comb(a, 2) * comb(b, 2),
        "3star": lambda a, b: a * comb(b, 3) + b * comb(a, 3),
        "4path": lambda a, b: a * (a - 1) * b * (b - 1),
        "motif3": lambda a, b: [a * comb(b, 2) + b * comb(a, 2), 0],
        "motif4": lambda a, b: [a * comb(b, 3) + b * comb(a, 3), 0, 0, comb(a, 2) * comb(b, 2), 0, 0],
        **{f"clique{k}": (lambda a, b: 0) for k in range(3, 9)},
    },
    "book": {
        "tc": lambda n: n, "diamond": lambda n: comb(n, 2), "rectangle": lambda n: comb(n, 2), "house": lambda n: 0,
        "pentagon": lambda n: 0,
        "3star": lambda n: 2 * comb(n + 1, 3),
        "4path": lambda n: 3 * n * (n - 1),
        "tailedtriangle": lambda n: 2 * n * (n - 1),
        "motif3": lambda n: [2 * comb(n, 2), n],
        "motif4": lambda n: [2 * comb(n, 3), 0, 0, 0, comb(n, 2), 0],
        "clique3": lambda n: n,
        **{f"clique{k}": (lambda n: 0) for k in range(4, 9)},
    },
    "complete": {"tc": lambda n: comb(n, 3), **{f"clique{k}": (lambda n, k=k: comb(n, k)) for k in range(3, 9)}},
    "multipartite": {"tc": lambda r, s: comb(r, 3) * s ** 3, **{f"clique{k}": (lambda r, s, k=k: comb(r, k) * s ** k) for k in range(3, 9)}},
}


def lagrange(xs, ys, x) -> int:
    """the value at x of the polynomial through (xs, ys), in rationals; asserted to be an integer"""
    tot = Fraction(0)
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        t = Fraction(yi)
        for j, xj in enumerate(xs):
            if j != i:
                t *= Fraction(x - xj, xi - xj)
        tot += t
    assert tot.denominator == 1, (xs, ys, x, tot)
    return int(tot)


def fit_sizes(what: str) -> list[int]:
    """the D + 1 class sizes (D = |V(P)|) that an interpolation is fitted on"""
    return list(range(1, pattern_size(what) + 2))


@functools.lru_cache(maxsize=None)
def _oracle_at(family: str, params: tuple, what: str):
    c = oracle_count(graph(family, params), what)
    return tuple(c) if isinstance(c, list) else c


def interpolate(family: str, params, what: str, sizes=None):
    """the count at `params` from oracle counts at `sizes` of the last parameter (default: fit_sizes(what)), the others held"""
    params = tuple(params)
    xs = list(sizes or fit_sizes(what))
    ys = [_oracle_at(family, params[:-1] + (x,), what) for x in xs]
    if isinstance(ys[0], tuple):
        return [lagrange(xs, [y[i] for y in ys], params[-1]) for i in range(len(ys[0]))]
    return lagrange(xs, ys, params[-1])


def has_closed_form(family: str, what: str) -> bool:
    return what in CLOSED.get(family, {})


def expected(family: str, params, what: str):
    """the exact count of `what` on family(params): its closed form where there is one, else exact interpolation from the oracle"""
    if has_closed_form(family, what):
        return CLOSED[family][what](*params)
    return interpolate(family, params, what)
