"""k-truss and truss decomposition on the GPU (gm_ktruss / gm_truss_decompose, csrc/gm_local.hip) against the naive sequential peeling of
tests/truss_ref.py: per entry, the supports inside the truss included, the number of edges and the number of whole-frontier rounds -- on
the five small graphs, and on the shapes where a CONCURRENT round goes wrong: all three edges of a triangle in one frontier, two of them,
a survivor that two frontier edges would both decrement, 70,000 decrements on one counter, several truss levels in one graph.  The peel
kernel bisects the rows in global memory (no LDS stage: no row length at which it changes path).  Every value is printed before it is
asserted."""
import functools
import os
import subprocess

import numpy as np
import pytest

import truss_ref as TR
import twin_graphs as T
from common import ROOT, load_graph
from graphminer_amd import ktruss, truss_decompose
from graphminer_amd.rmat import csr_from_pairs

pytestmark = pytest.mark.gpu
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
REMOVED = TR.REMOVED


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_arrays(label, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    print(f"{label}: {len(want)} values, {bad.size} differ, first at {bad[:5].tolist()}: got {np.asarray(got)[bad[:5]].tolist()} "
          f"want {np.asarray(want)[bad[:5]].tolist()}", flush=True)
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, label


def from_pairs(nv, pairs):
    s, d = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    return csr_from_pairs(nv, s, d)


def clique_pairs(ids):
    return [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]]


def check_ktruss(label, sym, g, k, want=None):
    """gm_ktruss at k against the helper (or `want` = its (per entry, edges, rounds)); returns the number of edges"""
    want_sup, want_m, want_rounds = want if want is not None else TR.ktruss(g, k)
    m, sup, rounds, st = ktruss(sym, k, return_stats=True)
    check_arrays(f"{label} {k}-truss per entry", sup, want_sup)
    check(f"{label} {k}-truss edges", m, want_m)
    check(f"{label} {k}-truss edges against the entries", m, int((sup != REMOVED).sum()) // 2)
    check(f"{label} {k}-truss rounds", rounds, want_rounds)
    assert rounds >= 1 and st.tasks == g.E() and st.kernel_ms > 0
    return m


def check_decompose(label, sym, g, want=None):
    want_tau, want_kmax, want_rounds = want if want is not None else TR.trussness(g)
    tau, k_max, rounds = truss_decompose(sym)
    check_arrays(f"{label} trussness per entry", tau, want_tau)
    check(f"{label} k_max", k_max, want_kmax)
    check(f"{label} k_max against the entries", k_max, int(tau.max()))
    check(f"{label} decomposition rounds", rounds, want_rounds)
    assert rounds >= 1
    return k_max


@functools.lru_cache(maxsize=None)
def ref_trussness(name):
    return TR.trussness(load_graph(name))


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs(dev, name):
    g = load_graph(name)
    with g.to_device(dev) as sym:
        k_max = check_decompose(name, sym, g, ref_trussness(name))
        for k in (2, 3, 4, k_max, k_max + 1):
            m = check_ktruss(name, sym, g, k)
            # k_max is the largest k with a non-empty k-truss, and the k-truss is the edges of trussness >= k
            check(f"{name} {k}-truss empty", m == 0, k > k_max)
            check(f"{name} {k}-truss edges against the trussness", m, int((ref_trussness(name)[0] >= k).sum()) // 2)
        check_decompose(name + " again", sym, g, ref_trussness(name))


def test_all_three_edges_in_one_frontier(dev):
    for n in (3, 4):
        g = T.graph("complete", (n,))
        with g.to_device(dev) as sym:
            m, sup, rounds = ktruss(sym, n + 1)
            check(f"K_{n} {n + 1}-truss", (m, np.unique(sup).tolist(), rounds), (0, [REMOVED], 2))
            check_ktruss(f"K_{n}", sym, g, n)
            check_decompose(f"K_{n}", sym, g)


def test_two_frontier_edges_of_a_triangle(dev):
    """K_4 minus the edge 2-3 at k = 4: the four outer edges (support 1) leave in one round, the chord 0-1 loses one per triangle -- each
    time from a triangle with two frontier edges -- and leaves in the next"""
    g = from_pairs(4, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)])
    with g.to_device(dev) as sym:
        m, sup, rounds = ktruss(sym, 4)
        check("K_4 - e 4-truss", (m, np.unique(sup).tolist(), rounds), (0, [REMOVED], 3))
        check_ktruss("K_4 - e", sym, g, 3)
        check_decompose("K_4 - e", sym, g)


def test_no_double_decrement(dev):
    """K_5 plus a vertex joined to two of its vertices, k = 5: edge 0-1 must go 4 -> 3 and K_5 survive with supports 3"""
    g = from_pairs(6, clique_pairs(list(range(5))) + [(0, 5), (1, 5)])
    with g.to_device(dev) as sym:
        m, sup, rounds = ktruss(sym, 5)
        check("K_5 + v 5-truss", (m, np.unique(sup).tolist(), rounds), (10, [3, REMOVED], 2))
        check_ktruss("K_5 + v", sym, g, 5)
        check_ktruss("K_5 + v", sym, g, 6)
        check_decompose("K_5 + v", sym, g)


def test_many_decrements_on_one_counter(dev):
    """B_70000 at k = 4: the 140,000 page edges leave in round 1 and take 70,000 from the spine's counter, the spine leaves in round 2"""
    n = 70000
    g = T.graph("book", (n,))
    with g.to_device(dev) as sym:
        m, sup, rounds = ktruss(sym, 4)
        check(f"B_{n} 4-truss", (m, np.unique(sup).tolist(), rounds), (0, [REMOVED], 3))
        m, sup, rounds = ktruss(sym, 3)
        src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
        spine = (src < 2) & (g.col_idx < 2)
        check(f"B_{n} 3-truss", (m, sup[spine].tolist(), np.unique(sup[~spine]).tolist(), rounds), (2 * n + 1, [n, n], [1], 1))
        tau, k_max, rounds = truss_decompose(sym)
        check(f"B_{n} trussness", (np.unique(tau).tolist(), k_max), ([3], 3))


def test_k300(dev):
    n = 300
    g = T.graph("complete", (n,))
    with g.to_device(dev) as sym:
        m, sup, rounds = ktruss(sym, n)
        check(f"K_{n} {n}-truss", (m, np.unique(sup).tolist(), rounds), (n * (n - 1) // 2, [n - 2], 1))
        m, sup, rounds = ktruss(sym, n + 1)
        check(f"K_{n} {n + 1}-truss", (m, np.unique(sup).tolist(), rounds), (0, [REMOVED], 2))
        tau, k_max, rounds = truss_decompose(sym)
        check(f"K_{n} trussness", (np.unique(tau).tolist(), k_max, rounds), ([n], n, 3))


def test_several_levels(dev):
    """K_5 and K_9 sharing vertex 0, and a pendant path on vertex 1: trussness 5, 9 and 2"""
    k5, k9 = [0, 1, 2, 3, 4], [0] + list(range(5, 13))
    g = from_pairs(16, clique_pairs(k5) + clique_pairs(k9) + [(1, 13), (13, 14), (14, 15)])
    with g.to_device(dev) as sym:
        k_max = check_decompose("K_5 + K_9 + path", sym, g)
        check("K_5 + K_9 + path k_max", k_max, 9)
        for k in (2, 3, 5, 6, 9, 10):
            check_ktruss("K_5 + K_9 + path", sym, g, k)
    g = T.graph("split", (6, 5), order="random", seed=2)  # a shuffled numbering
    with g.to_device(dev) as sym:
        check_decompose("S_6,5 shuffled", sym, g)
        check_ktruss("S_6,5 shuffled", sym, g, 7)


def test_refusals_and_the_empty_graph(dev):
    import ctypes as C

    import torch

    from graphminer_amd import Graph, _lib

    lib = _lib.load()
    n, rounds, kmax = C.c_uint64(5), C.c_int32(5), C.c_int32(5)
    with load_graph("citeseer").to_device(dev) as sym:
        buf = torch.zeros(sym.ne, dtype=torch.int32, device=f"cuda:{dev}")
        check("k = 1", lib.gm_ktruss(sym.handle, 1, None, None, C.byref(n), C.byref(rounds), None), _lib.GM_ERR_INVALID)
        check("no trussness array", lib.gm_truss_decompose(sym.handle, None, None, C.byref(kmax), C.byref(rounds), None), _lib.GM_ERR_INVALID)
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("ktruss world = 2", lib.gm_ktruss(sym.handle, 3, C.byref(la), None, C.byref(n), C.byref(rounds), None), _lib.GM_ERR_UNSUPPORTED)
        check("decompose world = 2", lib.gm_truss_decompose(sym.handle, C.byref(la), buf.data_ptr(), C.byref(kmax), C.byref(rounds), None),
              _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        cnt = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = cnt.data_ptr()
        check("ktruss d_counts", lib.gm_ktruss(sym.handle, 3, C.byref(la), None, C.byref(n), C.byref(rounds), None), _lib.GM_ERR_UNSUPPORTED)
        # the entries may be left out: the count alone
        check("count only", lib.gm_ktruss(sym.handle, 3, None, None, C.byref(n), C.byref(rounds), None), _lib.GM_OK)
        check("count only, edges", int(n.value), TR.ktruss(load_graph("citeseer"), 3)[1])
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        check("no edges, 3-truss", ktruss(sym, 3)[0::2], (0, 0))
        check("no edges, trussness", truss_decompose(sym)[1:], (0, 0))


def test_cli_citeseer(dev):
    exe = os.path.join(ROOT, "graphminer_amd", "bin", "truss_gpu_base")
    prefix = os.path.join(ROOT, "tests", "fixtures", "citeseer", "graph")
    g = load_graph("citeseer")
    r = subprocess.run([exe, prefix, "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    check("truss_gpu_base 4", r.stdout.strip().splitlines()[-1], f"ktruss_edges = {TR.ktruss(g, 4)[1]}")
    r = subprocess.run([exe, prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    check("truss_gpu_base", r.stdout.strip().splitlines()[-1], f"max_truss = {ref_trussness('citeseer')[1]}")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    check("truss_gpu_base without arguments", r.returncode, 1)
