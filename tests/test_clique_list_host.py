"""tests/clique_list_ref.py against the golden k-clique counts, its checker against broken lists, its unranking and the planted expectation
against the reference itself; the ABI surface of gm_clique_list (declared, bound, refusing a null handle, mirrored as clique_list, its
thresholds exported).  No GPU.  Every value is printed before it is asserted."""
import ctypes as C
import functools
import itertools
from math import comb

import numpy as np
import pytest

import planted_cliques as P
from clique_list_ref import check_list, clique_list_ref, lex_window, order_keys, planted_expected, row_roots, sort_rows, unrank
from common import GOLDEN, load_graph
from list_ref import list_ref

SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42"]


@functools.lru_cache(maxsize=None)
def ref(name, k):
    r = clique_list_ref(load_graph(name), k)
    r.setflags(write=False)
    return r


def golden(name, k):
    return GOLDEN[name]["tc"] if k == 3 else GOLDEN[name][f"clique{k}"]


@pytest.mark.parametrize("name", SMALL)
def test_ref_counts_and_checker_accepts(name):
    g = load_graph(name)
    for k in range(3, 9):
        rows = ref(name, k)
        print(f"{name} k={k}: {len(rows)} rows, golden {golden(name, k)}", flush=True)
        assert len(rows) == golden(name, k)
        check_list(g, k, rows, 0)
    tri = ref(name, 3)
    print(f"{name} k=3 against list_ref: {tri.shape} {list_ref(g).shape}", flush=True)
    assert np.array_equal(sort_rows(tri), list_ref(g))


def test_roots_and_order_keys():
    g = load_graph("citeseer")
    rows = ref("citeseer", 4)
    deg = np.diff(np.asarray(g.row_ptr))
    roots = row_roots(g, rows)
    for r, root in list(zip(rows.tolist(), roots.tolist()))[:50]:
        want = min(r, key=lambda v: (deg[v], v))
        assert root == want, (r, root, want)
    keys = order_keys(g, rows)
    print(f"roots ascending: {bool((np.diff(keys[:, 0]) >= 0).all())}", flush=True)
    assert (np.diff(keys[:, 0]) >= 0).all()


def test_checker_rejects_broken_lists():
    g = load_graph("citeseer")
    rows = np.array(ref("citeseer", 4))
    check_list(g, 4, rows, 0)
    swapped = rows.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    with pytest.raises(AssertionError, match="out of order"):
        check_list(g, 4, swapped, 0)
    dup = np.concatenate([rows[:20], rows[19:]])
    with pytest.raises(AssertionError, match="out of order or equal"):
        check_list(g, 4, dup, 0)
    bad = rows.copy()
    nv = g.V()
    row = bad[5].astype(np.int64)
    nbrs = set(np.asarray(g.col_idx)[int(g.row_ptr[row[0]]):int(g.row_ptr[row[0] + 1])].tolist())
    other = next(v for v in range(int(row[3]) + 1, nv) if v not in nbrs)
    bad[5, 3] = other
    with pytest.raises(AssertionError, match="no clique"):
        check_list(g, 4, bad, 0)
    desc = rows.copy()
    desc[7] = desc[7][::-1]
    with pytest.raises(AssertionError, match="ascending"):
        check_list(g, 4, desc, 0)


def test_unranking_is_the_ref_on_k9():
    import twin_graphs as T

    g = T.graph("complete", (9,))
    for k in range(3, 9):
        want = np.array(list(itertools.combinations(range(9), k)), dtype=np.int32)
        got = clique_list_ref(g, k)
        print(f"K_9 k={k}: ref {got.shape}, combinations {want.shape}", flush=True)
        assert np.array_equal(got, want)
        assert np.array_equal(lex_window(9, k, 0, comb(9, k)), want)
        for r in (0, 1, comb(9, k) // 2, comb(9, k) - 1):
            assert unrank(9, k, r) == want[r].tolist()
        assert np.array_equal(lex_window(9, k, 5, 7), want[5:12])
    assert unrank(256, 5, 2**32) == lex_window(256, 5, 2**32 - 1, 2)[1].tolist()


@pytest.mark.parametrize("members", ["standard", "staircase"])
def test_planted_expectation_is_the_ref(members):
    blocks = P.random_blocks(44, *P.LOW)
    mk = P._standard_members if members == "standard" else P._staircase_members
    for scattered in (False, True):
        p = P.Planted(blocks, mk(blocks, 44), scattered)
        for k in (3, 4, 5):
            want = sort_rows(clique_list_ref(p.graph, k))
            got = planted_expected(p, k)
            print(f"planted {members} scattered={scattered} k={k}: expected {got.shape}, ref {want.shape}, total {p.expected(k)[2]}", flush=True)
            assert np.array_equal(got, want)
            assert len(got) == p.expected(k)[2]


def _list_cell(base, off, ks, recipe):
    """the graph of a cell of tests/test_gpu_clique_list.py (the same Cell, the constants read from the library: a host call)"""
    from common import gm_constant

    consts = {"l2": gm_constant("kcl_list_regs2_row"), "l8": gm_constant("kcl_list_regs8_row"), "lds": gm_constant("kcl_local_lds_row"), "big": 2048}
    cell = P.Cell(f"{base}{off:+d}", "L", base, off, ks, True, recipe)
    return P.cell_graph(cell, tuple(sorted(consts.items()))), consts[base] + off


@pytest.mark.parametrize("base,off,ks,recipe,asked", [("l8", 0, (6, 7, 8), P.HIGH, (6, 7, 8)), ("lds", 0, (6, 7, 8), P.HIGH, (6, 7, 8)),
                                                      ("big", 1, (3, 4, 5), P.LOW, (5,))], ids=["l8+0-high", "lds+0-high", "big+1 k=5"])
def test_planted_listing_cells_are_feasible(base, off, ks, recipe, asked):
    """what test_planted_rows_on_both_sides_of_every_constant asks of its inputs before it runs the GPU, for the cells whose row is AT a
    constant at k = 6, 7, 8 and for the row of 2049 entries at k = 5"""
    p, d = _list_cell(base, off, ks, recipe)
    print(f"{base}{off:+d}: the longest row {p.max_row}, the roots' rows {p.root_rows()}, {p.nv} vertices", flush=True)
    assert (p.max_row, max(p.root_rows())) == (d, d)
    for k in asked:
        cond, want = p.conditions(k), planted_expected(p, k)
        print(f"{base}{off:+d} k={k}: {cond}, expected rows {len(want)}, total {p.expected(k)[2]}", flush=True)
        assert cond["blocks_with_clique"] >= 0.9 and len(want) >= 1000 and len(want) == p.expected(k)[2]
        assert len(np.unique(want, axis=0)) == len(want) and bool((want[:, 1:] > want[:, :-1]).all())


def test_root_boundaries_on_a_reference_list():
    """tests/list_windows.py root_boundaries on the reference's own list of a planted graph: the slots it names are where the root, the
    entry and the pair change, and the windows it calls exact hold one root / entry / pair"""
    from list_windows import out_list, root_boundaries

    blocks = P.random_blocks(150, *P.LOW)
    p = P.Planted(blocks, P._standard_members(blocks, 150), True)
    rows = clique_list_ref(p.graph, 4)
    keys = order_keys(p.graph, rows)
    root = int(p.i_id[0])
    L = out_list(p.graph, root)
    bounds, exact, info = root_boundaries(p.graph, keys, root)
    print(f"root {root}: {info}\n  {bounds}\n  {exact}", flush=True)
    assert len(L) == 150 == info["row"] and info["cross pairs behind a carried base"] >= 1
    i, l, before = info["cross pair"]
    assert l // 64 > i // 64 and before >= 1
    named = dict(bounds)
    r0, r1 = named["the root's first slot"], named["the slot behind the root"]
    assert bool((keys[r0:r1, 0] == root).all()) and (r0 == 0 or keys[r0 - 1, 0] != root) and (r1 == len(keys) or keys[r1, 0] != root)
    for label, b in bounds:
        if "entry" in label and "pair" not in label:
            assert keys[b, 0] == root and (b == r0 or keys[b - 1, 1] != keys[b, 1]), label
        elif "pair" in label and "rows into" not in label:
            assert keys[b, 0] == root and (b == r0 or tuple(keys[b - 1, 1:3]) != tuple(keys[b, 1:3])), label
    b = named["a pair in a later chunk than its entry"]
    assert (int(np.searchsorted(L, keys[b, 1])), int(np.searchsorted(L, keys[b, 2]))) == (i, l) and keys[b - 1, 1] == keys[b, 1]
    for (label, first, cap), cols in zip(exact, (1, 2, 3)):
        inside = keys[first:first + cap, :cols]
        assert cap >= 1 and bool((inside == inside[0]).all()), label
        assert first == 0 or tuple(keys[first - 1, :cols]) != tuple(inside[0]), label
        assert first + cap == len(keys) or tuple(keys[first + cap, :cols]) != tuple(inside[0]), label


def test_abi_surface():
    import graphminer_amd
    from graphminer_amd import _lib

    assert "gm_clique_list" in {s[0] for s in _lib.SYMBOLS}
    lib = _lib.load()
    rc = lib.gm_clique_list(None, 4, None, 0, 0, None, None, None, None)
    print(f"gm_clique_list on a null handle: {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID
    assert "clique_list" in graphminer_amd.__all__ and callable(graphminer_amd.clique_list)
    vals = {}
    for name in ("kcl_list_regs2_row", "kcl_list_regs8_row", "kcl_local_lds_row"):
        v = C.c_int64(0)
        _lib.check(lib.gm_constant(name.encode(), C.byref(v)), "gm_constant")
        vals[name] = int(v.value)
    print(f"constants: {vals}", flush=True)
    assert 0 < vals["kcl_list_regs2_row"] < vals["kcl_list_regs8_row"] < vals["kcl_local_lds_row"]
