"""The cells of tests/test_gpu_clique_count_planted.py on the CPU (tests/planted_count_cells.py): the class rule restated from the
library's constants gives the steps the kernels were written for; every cell sits on the row it claims and meets the conditions that keep
it from hiding a failure; and every family's construction, at shrunken sizes, has the total the oracle counts on the oriented graph -- so
the expected totals rest on the oracle and on binomials, never on the library.  Needs the built library for gm_constant only."""
import numpy as np
import pytest

import oracle as O
import planted_cliques as P
import planted_count_cells as PC
from common import clique_count_constants

CONSTS = clique_count_constants()
CELLS = PC.cells(CONSTS)


def test_restated_class_rule_gives_the_steps_of_today():
    c = CONSTS
    steps = PC.class_steps(c)
    for s in steps:
        print(s, flush=True)
    assert (c["bit_words"], c["mma_words_small"], c["mma_words_big"], c["wide_max_deg"], c["cb_max_deg"], c["stage_cap"]) == (2048, 9216, 36864, 2048, 2048, 1024)
    assert steps == PC.STEPS_TODAY
    # more than four column blocks never occur (entries 4 .. 7 of a vertex's eight queue entries are skipped)
    assert max(PC.row_class(d, c)[2] for d in range(1025, c["cb_max_deg"] + 1)) == 4
    # every step has a cell on each side, at k = 4, in family M
    rows = {cell.row for cell in CELLS if cell.family == "M"}
    assert all(d in rows and d + 1 in rows for d, _, _ in steps)
    assert len({cell.name for cell in CELLS}) == len(CELLS)


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_conditions_of_every_gpu_cell(cell):
    c = CONSTS
    g = PC.cell_graph(cell)
    census = PC.class_census(g.row_len, c)
    print(f"{cell.name}: {g.nv} vertices, {g.col_idx.size} entries, D {g.D}, roots {g.root_rows()[:6]}, max row {g.max_row}, by class {census}", flush=True)
    assert max(g.root_rows()) == cell.row == g.max_row
    assert np.array_equal(PC.stated_rows(cell, g), np.sort(g.row_len))
    assert g.nv < 2 ** 31 and g.col_idx.size < 2 ** 31
    for k in cell.ks:
        total, share = PC.planted_total(g, k), PC.blocks_with_clique(g, k)
        print(f"{cell.name} k={k}: total {total}, blocks with a k-clique {share:.3f}", flush=True)
        assert 0 < total < 2 ** 64
        assert share >= 0.9
        assert min(b.size for b in g.blocks) >= k
        if cell.family in ("M", "Mc") and len(g.blocks) > 1:
            # no two blocks with more than a tenth of the total have the same size: one swapped for the other changes the total
            heavy = [size for size, s in PC.block_shares(g, k) if s > 0.1]
            print(f"  heavy blocks {heavy}", flush=True)
            assert len(heavy) == len(set(heavy)) >= 1
    if cell.recipe == "mix":
        assert g.blocks[0].kind == "complete" and 2 * g.blocks[0].size > cell.row and g.blocks[1].kind == "complete" and g.blocks[1].size != g.blocks[0].size
        span = np.ptp(g.h_id[g.first[0]:g.first[1]])
        assert (span > 0.9 * cell.row) if cell.scattered else (span < g.blocks[0].size + len(g.members))
    if cell.family in ("M", "Mc", "B", "R"):
        assert PC.row_class(cell.row, c) == cell.between[0]
    if cell.family == "B":
        a, b = PC.root_hosting(g, 0, c)
        assert (a, b) == (cell.row - cell.row // 2, cell.row // 2) and min(a, b) >= 1
        assert PC.root_hosting(g, 0, c, topo=False) == (cell.row, 0)  # as numbered the tail is the whole row: the root hosts everything
    if cell.family == "R":
        assert sorted(g.root_rows()) == sorted(cell.arg)
        assert {PC.row_class(r, c) if isinstance(PC.row_class(r, c), str) else PC.row_class(r, c)[1] for r in g.root_rows()} == {"narrow", 0, 1, 2}
        assert PC.matrix_words(g, c) * 4 > 2 * (1 << 20)  # an arena of 1 MiB: three rounds or more
        roots = [int(g.i_id[x]) for x, m in enumerate(g.members) if not m.top]
        assert g.row_len[min(roots)] == max(g.root_rows())  # as numbered the longest root comes first
    if cell.family == "D" and cell.between[0] == "m":
        m = cell.between[1]
        assert g.blocks[0].kind in ("complete", "hub") and g.blocks[0].size == m + 1 and cell.row >= m + 1
        first = int(g.h_id[g.first[0]:g.first[1]].min())  # the matrix row of m set bits: the first member's edges into its block
        assert g.row_len[first] - sum(1 for mm in g.members if mm.top and 0 in mm.blocks) == m
        if g.blocks[0].kind == "hub":
            assert first == g.h_id[0] and not cell.scattered
    if any(f.startswith("core_cut") for f in cell.forms):
        x = max((x for x, m in enumerate(g.members) if not m.top), key=lambda x: int(g.row_len[g.i_id[x]]))
        for plus in (0, 3):
            h, base = PC.core_cut(g, x, plus)
            below = PC.plan_tasks(g, c, base) - PC.plan_tasks(g, c, 0)
            print(f"  core cut +{plus}: GM_CORE_H {h}, base {base}, streamed entries of wide rows {below}", flush=True)
            assert base % 32 == plus and h >= 64 and 0 < below < PC.plan_tasks(g, c, -1) - PC.plan_tasks(g, c, 0)


def shrunk(cell):
    return PC.build(cell, shrink=-(-cell.row // 80))


SMALL_CELLS = [cell for cell in CELLS if cell.name in ("M-1025", "M-2048-one-block", "Mc-1409", "B-800", "R-roots", "D-m256", "D-row4097", "D-m2048", "D-k8")]


@pytest.mark.parametrize("cell", SMALL_CELLS, ids=[c.name for c in SMALL_CELLS])
def test_family_recipe_against_the_oracle_at_shrunken_size(cell):
    g = shrunk(cell)
    assert max(g.root_rows()) <= 80
    assert np.array_equal(PC.stated_rows(cell, g), np.sort(g.row_len))
    odag = O.orient(O.OGraph(g.row_ptr, g.col_idx))
    assert np.array_equal(np.sort(np.diff(odag.row_ptr)[:g.n_core]), np.sort(g.row_len))
    for k in (4, 5, 6):
        want = O.clique(odag, k)
        got = PC.planted_total(g, k)
        print(f"{cell.name} shrunk to rows {g.root_rows()[:6]} ({len(g.blocks)} blocks) k={k}: planted total {got}, oracle {want}", flush=True)
        assert got == want > 0
        assert got == g.expected(k)[2]  # (the entry-by-entry rule of planted_cliques.py sums to the same)
