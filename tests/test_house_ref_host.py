"""The dense closed form of the house count (tests/house_ref.py), the reference of tests/test_gpu_map_kernels.py, checked on the CPU: against
the CPU oracle's loop nest (oracle.house) on the small golden graphs and on three seeded random graphs, against a literal Python loop nest,
against the closed-form value of K_n worked out by hand (60 C(n, 5): house_ref.house_complete), and on graphs padded with leaves and
isolated vertices, which the form strips.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import house_ref as H
import oracle as O
from common import GOLDEN, load_graph, random_graph

SMALL = ["rmat6_ef4_s1", "rmat8_ef8_s42", "citeseer", "cora"]


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


@pytest.mark.parametrize("name", SMALL)
def test_golden_graphs(name):
    g = load_graph(name)
    want = O.house(O.OGraph(g.row_ptr, g.col_idx))
    check(f"{name} oracle against the golden", want, GOLDEN[name]["house"])
    check(f"{name} dense form against the oracle", H.house(g), want)


@pytest.mark.parametrize("nv,ne,seed", [(30, 130, 1), (40, 320, 2), (25, 240, 3)])
def test_random_graphs(nv, ne, seed):
    g = random_graph(nv, ne, seed)
    want = O.house(O.OGraph(g.row_ptr, g.col_idx))
    assert want > 0
    check(f"G({nv}, {ne} draws) loop nest against the oracle", H.house_loops(g), want)
    check(f"G({nv}, {ne} draws) dense form against the oracle", H.house(g), want)


@pytest.mark.parametrize("n", [4, 5, 6, 9, 33])
def test_complete_graph(n):
    from graphminer_amd.rmat import csr_from_pairs

    i, j = np.triu_indices(n, 1)
    g = csr_from_pairs(n, i.astype(np.uint64), j.astype(np.uint64))
    check(f"K_{n} dense form against 60 C(n, 5)", H.house(g), H.house_complete(n))
    if n <= 9:
        check(f"K_{n} loop nest against 60 C(n, 5)", H.house_loops(g), H.house_complete(n))


def test_leaves_and_isolated_vertices_are_stripped():
    """a random graph, then the same with a leaf on every third vertex, a path of two leaves' worth hanging off one, and isolated ids between"""
    from graphminer_amd.rmat import csr_from_pairs

    g = random_graph(40, 320, 2)
    want = H.house(g)
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr)).astype(np.uint64)
    col = g.col_idx.astype(np.uint64)
    half = src < col
    owners = np.arange(0, 40, 3, dtype=np.uint64)
    leaves = np.uint64(50) + np.arange(owners.size, dtype=np.uint64) * np.uint64(2)  # (the ids between them stay isolated)
    h = csr_from_pairs(100, np.concatenate([src[half], owners]), np.concatenate([col[half], leaves]))
    assert int((np.diff(h.row_ptr) == 1).sum()) == owners.size and int((np.diff(h.row_ptr) == 0).sum()) > 0
    F, core = H.core_adjacency(h)
    assert core.size <= 40 and int(core.max()) < 40
    check("padded graph", H.house(h), want)
    check("padded graph, oracle", O.house(O.OGraph(h.row_ptr, h.col_idx)), want)
