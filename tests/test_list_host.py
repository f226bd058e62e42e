"""Triangle listing, the part that needs no GPU: the plain numpy reference of tests/list_ref.py against the golden triangle counts, its
ordered form (the documented order of gm_tc_list, by a walk of its own) against it, by hand and on complete graphs, and the ABI surface
of gm_tc_list (declared, bound, refusing a null handle, mirrored as tc_list)."""
import numpy as np
import pytest

import graphminer_amd
from common import GOLDEN, load_graph, random_graph
from graphminer_amd import _lib
from list_ref import list_ref, list_ref_ordered, sort_rows

SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]


@pytest.mark.parametrize("name", SMALL)
def test_list_ref_matches_the_golden_counts(name):
    tri = list_ref(load_graph(name))
    print(f"{name}: {len(tri)} rows, golden {GOLDEN[name]['motif3'][1]}", flush=True)
    assert tri.dtype == np.int32 and tri.shape == (GOLDEN[name]["motif3"][1], 3)
    assert bool((tri[:, 0] < tri[:, 1]).all() and (tri[:, 1] < tri[:, 2]).all()), "every row ascending"
    assert len(np.unique(tri, axis=0)) == len(tri), "every row once"


def _check_ordered(label, g, want_sorted):
    tri, off = list_ref_ordered(g)
    print(f"{label}: ordered {tri.shape} {tri.dtype}, entries {len(off) - 1}, off[-1] {int(off[-1])}, list_ref {want_sorted.shape}", flush=True)
    assert tri.dtype == np.int32 and off.dtype == np.int64
    assert np.array_equal(sort_rows(tri), want_sorted), label
    assert int(off[0]) == 0 and int(off[-1]) == len(tri) and bool((np.diff(off) >= 0).all())
    deg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
    assert len(off) - 1 == int(deg.sum()) // 2, "one oriented entry per edge"
    return tri, off


@pytest.mark.parametrize("name", SMALL)
def test_ordered_ref_is_list_ref_on_the_small_graphs(name):
    g = load_graph(name)
    _check_ordered(name, g, list_ref(g))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ordered_ref_is_list_ref_with_many_degree_ties(seed):
    """G(48, ~0.25): degrees of 48 vertices fall on a dozen values, so most orientations are decided by id"""
    g = random_graph(48, 300 + 40 * seed, seed)
    deg = np.diff(np.asarray(g.row_ptr))
    src = np.repeat(np.arange(g.V()), deg)
    ties = int((deg[src] == deg[np.asarray(g.col_idx)]).sum()) // 2
    print(f"seed {seed}: {g.E()} entries, {ties} edges between equal degrees, {len(set(deg.tolist()))} distinct degrees", flush=True)
    assert ties >= 20
    tri, _ = _check_ordered(f"random seed {seed}", g, list_ref(g))
    assert len(tri) >= 50


def test_ordered_ref_by_hand():
    """the hub 0 has the lowest id and the highest degree: every edge points AT it, so it is never u or v and its triangles come out in
    the order of their other corners' rows.  Degrees 6 4 3 3 2 2 2; N+(1) = 0; N+(2) = 0 1 3; N+(3) = 0 1; N+(4) = 0 5; N+(5) = 0;
    N+(6) = 0 1; N+(0) is empty."""
    from graphminer_amd.rmat import csr_from_pairs

    edges = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2), (1, 3), (2, 3), (1, 6), (4, 5)]
    g = csr_from_pairs(7, np.array([a for a, _ in edges], dtype=np.uint64), np.array([b for _, b in edges], dtype=np.uint64))
    tri, off = list_ref_ordered(g)
    # u = 2: v = 1 gives w = 0; v = 3 gives w = 0, 1.  u = 3: v = 1 gives w = 0.  u = 4: v = 5 gives w = 0.  u = 6: v = 1 gives w = 0.
    want = [[0, 1, 2], [0, 2, 3], [1, 2, 3], [0, 1, 3], [0, 4, 5], [0, 1, 6]]
    # entries: (1,0) (2,0) (2,1) (2,3) (3,0) (3,1) (4,0) (4,5) (5,0) (6,0) (6,1)
    want_off = [0, 0, 0, 1, 3, 3, 4, 4, 5, 5, 5, 6]
    print(f"by hand: rows {tri.tolist()} off {off.tolist()}", flush=True)
    assert tri.tolist() == want and off.tolist() == want_off
    assert want != sorted(want), "the documented order is not the lexicographic one here"
    assert np.array_equal(sort_rows(tri), list_ref(g))


@pytest.mark.parametrize("n", [3, 9, 66])
def test_ordered_ref_of_a_complete_graph_is_lexicographic(n):
    import itertools

    import twin_graphs as T

    tri, off = list_ref_ordered(T.graph("complete", (n,)))
    want = np.array(list(itertools.combinations(range(n), 3)), dtype=np.int32)
    print(f"K_{n}: {tri.shape} rows, want {want.shape}", flush=True)
    assert np.array_equal(tri, want)
    # entry (u, v) holds the n - 1 - v triangles (u, v, w > v)
    per = [n - 1 - v for u in range(n) for v in range(u + 1, n)]
    assert np.diff(off).tolist() == per


def test_entry_point_is_bound():
    assert "gm_tc_list" in {s[0] for s in _lib.SYMBOLS}


def test_null_handle_is_refused():
    rc = _lib.load().gm_tc_list(None, None, 0, 0, None, None, None, None)
    print(f"gm_tc_list on a null handle: {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID


def test_python_mirror_is_exported():
    assert "tc_list" in graphminer_amd.__all__ and callable(graphminer_amd.tc_list)
