"""tests/truss_ref.py -- the plain Python ground truth of the local counts and the k-truss -- against what is already pinned: the triangle
and diamond counts of tests/golden/golden.json (the reference's binaries) and closed forms on the twin families of tests/twin_graphs.py.
And the host-only refusals of gm_tc_local / gm_ktruss / gm_truss_decompose (no device needed).  Every value is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

import truss_ref as TR
import twin_graphs as T
from common import GOLDEN, load_graph
from graphminer_amd import _lib

SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


@functools.lru_cache(maxsize=None)
def sup_of(name):
    return TR.supports(load_graph(name))


@pytest.mark.parametrize("name", SMALL)
def test_supports_against_the_goldens(name):
    g = load_graph(name)
    sup = sup_of(name).astype(np.int64)
    tri = GOLDEN[name]["motif3"][1]
    check(f"{name} sum of supports / 6", int(sup.sum()) // 6, tri)
    assert int(sup.sum()) % 6 == 0
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    up = src < g.col_idx
    check(f"{name} sum C(sup, 2) over u < v", int((sup[up] * (sup[up] - 1) // 2).sum()), GOLDEN[name]["diamond"])
    check(f"{name} sum T_v", int(TR.vertex_triangles(g).sum()), 3 * tri)
    # the two directions of every edge agree
    key = np.minimum(src, g.col_idx) * g.V() + np.maximum(src, g.col_idx)
    o = np.argsort(key, kind="stable")
    assert (sup[o][0::2] == sup[o][1::2]).all()


def uniq(a):
    return sorted(set(int(x) for x in a))


@pytest.mark.parametrize("n", [3, 4, 7])
def test_complete(n):
    g = T.graph("complete", (n,))
    check(f"K_{n} supports", uniq(TR.supports(g)), [n - 2])
    tau, k_max, rounds = TR.trussness(g)
    check(f"K_{n} trussness", (uniq(tau), k_max), ([n], n))
    sup, m, r = TR.ktruss(g, n)
    check(f"K_{n} {n}-truss", (uniq(sup), m, r), ([n - 2], n * (n - 1) // 2, 1))
    sup, m, r = TR.ktruss(g, n + 1)
    check(f"K_{n} {n + 1}-truss", (uniq(sup), m, r), ([TR.REMOVED], 0, 2))


@pytest.mark.parametrize("n", [1, 5, 40])
def test_book(n):
    g = T.graph("book", (n,))
    sup = TR.supports(g)
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    spine = (src < 2) & (g.col_idx < 2)
    check(f"B_{n} spine", uniq(sup[spine]), [n])
    check(f"B_{n} pages", uniq(sup[~spine]), [1])
    check(f"B_{n} T_v", TR.vertex_triangles(g).tolist(), [n, n] + [1] * n)
    tau, k_max, _ = TR.trussness(g)
    check(f"B_{n} trussness", (uniq(tau), k_max), ([3], 3))
    check(f"B_{n} 4-truss", TR.ktruss(g, 4)[1], 0)


@pytest.mark.parametrize("a,b", [(3, 2), (5, 4)])
def test_split(a, b):
    g = T.graph("split", (a, b))
    tau, k_max, _ = TR.trussness(g)
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    pendant = (src >= a + b) | (g.col_idx >= a + b)
    check(f"S_{a},{b} pendant path", uniq(tau[pendant]), [2])
    check(f"S_{a},{b} the rest", (uniq(tau[~pendant]), k_max), ([a + 1], a + 1))


@pytest.mark.parametrize("r,s", [(3, 2), (4, 3), (2, 5)])
def test_multipartite(r, s):
    tau, k_max, _ = TR.trussness(T.graph("multipartite", (r, s)))
    check(f"K_{s}x{r} trussness", (uniq(tau), k_max), ([(r - 2) * s + 2], (r - 2) * s + 2))


def test_kab():
    g = T.graph("kab", (3, 5))
    check("K_3,5 supports", uniq(TR.supports(g)), [0])
    tau, k_max, rounds = TR.trussness(g)
    check("K_3,5 trussness", (uniq(tau), k_max, rounds), ([2], 2, 2))
    check("K_3,5 3-truss", TR.ktruss(g, 3)[1], 0)
    check("K_3,5 2-truss", TR.ktruss(g, 2)[1:], (15, 1))


def test_double_decrement_shape():
    """K_5 plus a vertex joined to two of its vertices, k = 5: the extra edges leave, edge 0-1 goes from 4 to 3, K_5 stays"""
    from graphminer_amd.rmat import csr_from_pairs

    iu, ju = np.triu_indices(5, 1)
    g = csr_from_pairs(6, np.concatenate([iu, [0, 1]]).astype(np.uint64), np.concatenate([ju, [5, 5]]).astype(np.uint64))
    check("support of 0-1", int(TR.supports(g)[0]), 4)
    sup, m, rounds = TR.ktruss(g, 5)
    check("5-truss", (uniq(sup), m, rounds), ([3, TR.REMOVED], 10, 2))


def test_host_only_refusals():
    lib = _lib.load()
    n, rounds, kmax, total = C.c_uint64(7), C.c_int32(7), C.c_int32(7), C.c_uint64(7)
    check("gm_tc_local(NULL)", lib.gm_tc_local(None, None, None, None, C.byref(total), None), _lib.GM_ERR_INVALID)
    check("gm_ktruss(NULL, 3)", lib.gm_ktruss(None, 3, None, None, C.byref(n), C.byref(rounds), None), _lib.GM_ERR_INVALID)
    check("gm_ktruss(NULL, 1)", lib.gm_ktruss(None, 1, None, None, C.byref(n), C.byref(rounds), None), _lib.GM_ERR_INVALID)
    check("gm_truss_decompose(NULL)", lib.gm_truss_decompose(None, None, None, C.byref(kmax), C.byref(rounds), None), _lib.GM_ERR_INVALID)
    check("gm_version", lib.gm_version() >= 101, True)
