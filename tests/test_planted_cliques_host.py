"""The planted-clique graphs (tests/planted_cliques.py) on the CPU: the rule that gives their expected values against clique_local_ref on
the WHOLE graph, entry by entry and vertex by vertex, on small instances (both block kinds, both layouts, roots and tops, k = 3 .. 8); the
DAG row lengths the helper claims against an orientation worked out here from the degrees; and, for every cell of
tests/test_gpu_clique_local_planted.py, the conditions its inputs have to meet for the GPU comparison to mean something."""
import numpy as np
import pytest

import clique_local_ref as R
import planted_cliques as P
from common import kcl_row_constants


def dag_rows(g):
    """the DAG row of every vertex under the orientation lower degree -> higher degree, ties by id, from the CSR alone"""
    rp, col = g.row_ptr, g.col_idx.astype(np.int64)
    deg = np.diff(rp)
    src = np.repeat(np.arange(deg.size, dtype=np.int64), deg)
    out = (deg[col] > deg[src]) | ((deg[col] == deg[src]) & (col > src))
    return src[out], col[out]


def small_members(nb, d):
    """two roots (every block; the first two) and three tops (even blocks, the last block, the middle blocks), ids below, inside and above H"""
    return (P.Member(tuple(range(nb)), d // 2), P.Member((0, 1), 0), P.Member(tuple(range(0, nb, 2)), 0, True),
            P.Member((nb - 1,), d, True), P.Member(tuple(range(1, nb - 1)), d // 3, True))


SMALL = {
    "random-low": (P.random_blocks(42, 8, 12, 0.7, seed=5), (3, 4, 5)),
    "random-high": (P.random_blocks(56, 12, 16, 0.9, seed=5), (6, 7, 8)),
    "complete": (tuple(P.Block("complete", b) for b in (9, 10, 11, 12, 13)), (3, 4, 5, 6, 7, 8)),
    "mixed-kinds": ((P.Block("complete", 11), P.Block("random", 14, 0.9, 3), P.Block("complete", 12), P.Block("random", 13, 0.9, 4)), (5, 6, 8)),
}


@pytest.mark.parametrize("scattered", [False, True], ids=["contig", "scat"])
@pytest.mark.parametrize("name", list(SMALL))
def test_rule_against_the_reference_on_the_whole_graph(name, scattered):
    blocks, ks = SMALL[name]
    d = sum(b.size for b in blocks)
    assert d <= 64
    g = P.Planted(blocks, small_members(len(blocks), d), scattered, seed=3)
    graph = g.graph
    for k in ks:
        want_ent = R.entry_cliques(graph, k)
        want_kv = R.vertex_cliques(graph, k, want_ent)
        ent, kv, total, inner = g.expected(k)
        bad = np.flatnonzero(ent != want_ent)
        print(f"{name} scattered={scattered} k={k}: {ent.size} entries, {bad.size} differ, first {bad[:5].tolist()}; total {total}", flush=True)
        assert bad.size == 0 and ent.dtype == np.uint64 and ent.shape == want_ent.shape
        assert np.array_equal(kv, want_kv) and kv.dtype == np.uint64
        assert total * k == sum(int(x) for x in want_kv) and total > 0
        assert len(inner) == sum(P.block_pairs(b)[0].size for b in blocks)
    if name == "complete":  # the closed forms, written out once more: block of b vertices with n members of I on it
        k = 5
        ent, kv, _, _ = g.expected(k)
        from math import comb

        for bi, b in enumerate(blocks):
            h = g.h_id[g.first[bi]:g.first[bi + 1]]
            e = g.row_ptr[h[0]] + np.flatnonzero(graph.N(int(h[0])) == h[1])[0]
            assert int(ent[e]) == comb(b.size - 2, k - 2) + int(g.n_i[bi]) * comb(b.size - 2, k - 3)
            assert int(kv[h[0]]) == comb(b.size - 1, k - 1) + int(g.n_i[bi]) * comb(b.size - 1, k - 2)


@pytest.mark.parametrize("scattered", [False, True], ids=["contig", "scat"])
def test_row_lengths_of_a_small_instance(scattered):
    blocks, _ = SMALL["random-low"]
    d = sum(b.size for b in blocks)
    g = P.Planted(blocks, small_members(len(blocks), d), scattered, seed=3)
    src, dst = dag_rows(g.graph)
    rows = np.bincount(src, minlength=g.nv)
    assert np.array_equal(rows[:g.n_core], g.row_len) and int(rows.max()) == g.max_row
    assert (rows[g.n_core:] == 1).all()  # a leaf points at its owner
    sizes = [b.size for b in blocks]
    assert g.root_rows() == [d, sizes[0] + sizes[1]]
    for x, m in enumerate(g.members):
        u = int(g.i_id[x])
        joined = np.sort(np.concatenate([g.h_id[g.first[bi]:g.first[bi + 1]] for bi in m.blocks]))
        if m.top:
            assert rows[u] == 0 and np.diff(g.row_ptr)[u] == g.D + 1
            assert all(g.dag_position(int(h), u) >= 0 for h in joined)  # it sits in the rows of its H vertices
        else:
            assert np.array_equal(dst[src == u], joined)  # exactly its H vertices, in id order
    assert (np.diff(g.row_ptr)[g.h_id] == g.D).all()
    # the ids: members below, inside and above the H ids
    assert g.i_id.min() == 0 and g.i_id.max() == g.n_core - 1 and ((g.i_id > g.h_id.min()) & (g.i_id < g.h_id.max())).any()
    if scattered:
        assert any(np.ptp(g.h_id[g.first[bi]:g.first[bi + 1]]) > 2 * blocks[bi].size for bi in range(len(blocks)))
    else:
        assert all(np.ptp(g.h_id[g.first[bi]:g.first[bi + 1]]) <= blocks[bi].size + len(g.members) for bi in range(len(blocks)))


def test_block_sizes():
    for total, lo, hi in ((63, 8, 14), (65, 13, 18), (442, 13, 18), (2060, 8, 14), (213, 8, 14), (96, 8, 8)):
        s = P.block_sizes(total, lo, hi, 0)
        assert sum(s) == total and min(s) >= lo and max(s) <= hi, (total, s)
    assert len({b.seed for b in P.random_blocks(2060, 8, 14, 0.8)}) == P.VARIANTS


def check_claim(cell, g, consts):
    for name in cell.above:
        assert g.max_row > consts[name], (cell.name, g.max_row, name)
    for name in cell.upto:
        assert g.max_row <= consts[name], (cell.name, g.max_row, name)


@pytest.mark.parametrize("cell", P.CELLS, ids=[c.name for c in P.CELLS])
def test_conditions_of_every_gpu_cell(cell):
    consts = kcl_row_constants()
    g = P.cell_graph(cell, tuple(sorted(consts.items())))
    d = max(P.mixed_rows(consts)) if cell.special == "mixed" else consts.get(cell.base, 0) + cell.off
    print(f"{cell.name}: d {d}, {g.nv} vertices, {g.col_idx.size} entries, D {g.D}, max row {g.max_row}, roots {g.root_rows()[:6]}", flush=True)
    # the rows: the longest root has d entries and is the DAG's longest row (E-branch: its H rows are longer, on purpose)
    assert max(g.root_rows()) == d
    if cell.special != "branch":
        assert g.max_row == d and int(g.row_len[g.is_h].max()) < d
    check_claim(cell, g, consts)
    src, _ = dag_rows(g.graph)
    rows = np.bincount(src, minlength=g.nv)
    assert np.array_equal(rows[:g.n_core], g.row_len) and int(rows.max()) == g.max_row
    for k in cell.ks:
        c = g.conditions(k)
        print(f"{cell.name} k={k}: {c}", flush=True)
        assert c["min_block"] >= k + 3
        assert c["blocks_with_clique"] >= 0.9
        assert c["inner_nonzero"] >= 0.5
        assert c["inner_distinct"] >= 32  # (k = 3: a value is (common neighbours inside the block) + n_I -- the staircase of tops gives them)
        if k >= 7:
            assert c["max_block"] <= 24
        if cell.special == "k70":
            assert c["max_block"] == P.WAVE + 6 and max(b.size for b in g.blocks if b.kind == "random") <= 24
    if cell.family == "C":
        assert cell.scattered
    if cell.special == "k70":  # the set of a pair of the complete block: its other members, more than one deal round
        assert g.blocks[0].kind == "complete" and g.blocks[0].size - 2 > P.WAVE and cell.scattered and max(cell.ks) <= 6
    if cell.special == "mixed":
        want = P.mixed_rows(consts)
        assert sorted(g.root_rows()) == sorted(want)
        assert want[0] <= consts["split"] < want[1] <= consts["lds"] < want[2] < want[3]
        wide = [int(g.i_id[x]) for x, m in enumerate(g.members) if not m.top and len(m.blocks) and g.row_len[g.i_id[x]] > consts["lds"]]
        assert g.row_len[min(wide)] == want[3]  # as numbered the longer wide root comes first
    if cell.special == "find":
        for bi, want in ((0, P.FIND_ROWS[:2]), (1, P.FIND_ROWS[2:])):
            have = set(g.h_rows(bi).tolist())
            assert set(want) <= have, (bi, sorted(have))
        # as numbered the entry searched for -- a block neighbour above -- is not at the front of its row: tops with smaller ids precede it
        h = g.h_id[g.first[0]:g.first[1]]
        longest = int(h[np.argmax(g.row_len[h])])
        nb = [int(v) for v in h if v > longest and g.dag_position(longest, int(v)) >= 0]
        assert nb and min(g.dag_position(longest, v) for v in nb) > 0
        tops = g.i_id[[x for x, m in enumerate(g.members) if m.top and m.blocks == (0,)]]
        assert (tops < h.min()).any() and ((tops > h.min()) & (tops < h.max())).any() and (tops > g.h_id.max()).any()
    if cell.special == "branch":
        assert (g.row_len[g.is_h] > 4 * d).all() and set(g.root_rows()) == {d}
        assert min(int(g.n_i[bi]) for bi in range(len(g.blocks))) == 5 * d + 1  # 40 tops and the root
