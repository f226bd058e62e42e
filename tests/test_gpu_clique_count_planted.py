"""The global k-clique count on the GPU (gm_clique: csrc/gm_cbuild.hip, gm_cgather.hip, gm_cmma.hip, clique_small_kernel, the mining
kernel's arena path, the k >= 5 recursion of csrc/gm_chunk.h) on planted-clique graphs (tests/planted_count_cells.py): one graph on each
side of every row length at which the count changes path, dense blocks of different sizes spread over the root's row, the expected
total from binomials and the per-block reference alone.  On a complete graph every matrix word is all ones and a read of the wrong row
or column block still gives the right total; here one block read for another changes it.

A case is (cell, form), on a fresh handle (plans are cached per handle; developer options are read when a plan is built):
  default       the plan as the library builds it (the blocked or the row-major gather: gm_clique4_gather_info says which)
  as_numbered   tune[6] & 0x200: the planted ids are not topological -- whole-list streams, square task grids, no core
  core_h0       GM_CORE_H=0: no core bitmap, every wide row built by cbuild_kernel (by default the whole of H lies in the core)
  row_gather, mining                 tune[6] & 0x8000000 / 0x40000
  core_cut32, core_cut3              GM_CORE_H so that the core's base cuts the longest root's row: a multiple of 32, and 3 above one
  world3, world2p1                   rank shares summed (policy 0 / 1)
  small_arena                        GM_WIDE_ARENA_MB=1: three rounds or more
  any_width, filter_stage2           k >= 5: tune[6] & 0x200000 / 0x20
At k = 4 the case asserts what the plan holds (clique_plan_info) against the plan restated on the CPU BEFORE it compares the count.  Every
figure is printed before it is asserted.  tests/test_planted_count_cells_host.py checks the cells and their expected totals on the CPU."""
from math import comb

import numpy as np
import pytest

import planted_count_cells as PC
from common import clique_count_constants
from graphminer_amd import CliqueSolver, Graph, _lib, clique_plan_info
from graphminer_amd._lib import dev_option

pytestmark = pytest.mark.gpu
CONSTS = clique_count_constants()
CELLS = PC.cells(CONSTS)
CASES = [(cell, form) for cell in CELLS for form in cell.forms]
MB = 1 << 20


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


TUNE = {"as_numbered": PC.AS_NUMBERED, "row_gather": PC.ROW_GATHER, "mining": PC.CLIQUE4_MINING, "any_width": PC.ANY_WIDTH,
        "filter_stage2": PC.FILTER_STAGE2}


def gather_info(dag):
    import ctypes as C

    info = (C.c_int64 * 4)()
    _lib.check(_lib.load().gm_clique4_gather_info(dag.handle, info), "gm_clique4_gather_info")
    return [int(x) for x in info]


def longest_root(g):
    return max((x for x, m in enumerate(g.members) if not m.top), key=lambda x: int(g.row_len[g.i_id[x]]))


def options_of(form, g):
    """the developer options of a form and the core's base they imply (None: the default core)"""
    if form == "core_h0":
        return {"GM_CORE_H": "0"}, -1
    if form in ("core_cut32", "core_cut3"):
        h, base = PC.core_cut(g, longest_root(g), 0 if form == "core_cut32" else 3)
        return {"GM_CORE_H": str(h)}, base
    if form == "small_arena":
        return {"GM_WIDE_ARENA_MB": "1"}, None
    return {}, None


def count_on_fresh_handle(dev, graph, k, form, opts):
    """(count, plan info or None, gather info or None) of one form on a fresh handle"""
    tune = t6(TUNE[form]) if form in TUNE else None
    for name, value in opts.items():
        dev_option(name, value)
    try:
        with graph.to_device(dev) as sym:
            dag = sym.orient()
            try:
                if form == "world3":
                    return sum(CliqueSolver(dag, k, rank=r, world=3) for r in range(3)), None, None
                if form == "world2p1":
                    return sum(CliqueSolver(dag, k, rank=r, world=2, policy=1) for r in range(2)), None, None
                got = CliqueSolver(dag, k, tune=tune)
                if k != 4:
                    return got, None, None
                if form == "mining":  # (everything in the mining kernel: this call builds no plan)
                    with pytest.raises(_lib.GraphMinerError):
                        clique_plan_info(dag)
                    return got, None, None
                return got, clique_plan_info(dag, as_numbered=form == "as_numbered"), (gather_info(dag) if form != "as_numbered" else None)
            finally:
                dag.free()
    finally:
        for name in opts:
            dev_option(name, None)


def plan_claims(g, c, form, info, ginfo, base_of_form):
    """what the plan of this form has to hold, from the graph's rows alone; returns the list of claims that fail"""
    census = PC.class_census(g.row_len, c)
    topo = form != "as_numbered"
    if base_of_form is None:
        core_base = g.nv - min(g.nv, c["core_h_default"]) if topo else -1
    else:
        core_base = base_of_form
    want = {"topo": topo, "stage": c["stage_cap"] if g.max_row <= c["stage_cap"] else c["cb_max_deg"], "core_base": core_base,
            "wide": census[0] + census[1] + census[2], "wide_by_class": [census[0], census[1], census[2]],
            "tasks": PC.plan_tasks(g, c, core_base), "arena_entries": int(g.row_len[g.row_len > c["cb_max_deg"]].sum())}
    print(f"  plan: got {info}", flush=True)
    print(f"  plan: want {want}; gather info {ginfo}; matrix words {PC.matrix_words(g, c)}", flush=True)
    bad = [key for key, v in want.items() if info[key] != v]
    if form == "small_arena":
        if not (PC.matrix_words(g, c) > 2 * MB // 4 and info["rounds"] >= 3):
            bad.append("rounds >= 3")
    elif info["rounds"] != 1:
        bad.append("rounds == 1")
    if core_base < 0 and (info["gather_units"] or info["gather_items"]):
        bad.append("no gather without a core")
    if ginfo is not None and (ginfo[0], ginfo[2]) != (info["gather_units"], info["gather_items"]):
        bad.append("gm_clique4_gather_info agrees")
    if core_base >= 0 and want["wide"] and form != "row_gather" and not info["gather_units"]:
        bad.append("blocked gather units")  # (a core and wide rows: the plan lists units for the blocked gather)
    return bad


@pytest.mark.parametrize("cell,form", CASES, ids=[f"{c.name}-{f}" for c, f in CASES])
def test_cell(dev, cell, form):
    c = CONSTS
    g = PC.cell_graph(cell)
    census = PC.class_census(g.row_len, c)
    print(f"{cell.name} {form}: {g.nv} vertices, {g.col_idx.size} entries, roots {g.root_rows()[:6]}, DAG max row {g.max_row}, "
          f"row {cell.row} = {PC.row_class(cell.row, c)} (sides {cell.between}), rows by class {census}", flush=True)
    # the cell sits where it claims: the root's row, the DAG's longest row, every row with a matrix as the recipe states it
    assert max(g.root_rows()) == cell.row == g.max_row
    assert np.array_equal(PC.stated_rows(cell, g), np.sort(g.row_len))
    if cell.family in ("M", "Mc", "B", "R"):
        assert cell.between[0] == PC.row_class(cell.row, c)
    if cell.family == "B":
        a, b = PC.root_hosting(g, 0, c)
        print(f"  root edges hosted by the root (type A) {a}, by the far end (type B) {b}; as numbered {PC.root_hosting(g, 0, c, topo=False)}", flush=True)
        assert (a, b) == (cell.row - cell.row // 2, cell.row // 2) and a >= 1 and b >= 1
    opts, base = options_of(form, g)
    failed = []
    for k in cell.ks:
        want = PC.planted_total(g, k)
        got, info, ginfo = count_on_fresh_handle(dev, g.graph, k, form, opts)
        print(f"{cell.name} {form} k={k}: got {got} want {want}", flush=True)
        if info is not None:
            bad = plan_claims(g, c, form, info, ginfo, base)
            assert not bad, (cell.name, form, "plan", bad)  # (before the count)
        if got != want:
            failed.append((k, got, want))
    assert not failed, failed


@pytest.mark.parametrize("form", PC.BASE_FORMS)
def test_complete_graph_one_past_the_longest_matrix(dev, form):
    """K_(cb_max_deg + 1) as a plain complete graph: the first vertex's row has cb_max_deg entries -- accumulators at cb_max_deg - 2, the
    per-block float sums near their largest value, the last word of the last column block -- and every shorter row follows"""
    n = CONSTS["cb_max_deg"] + 1
    col = np.tile(np.arange(n, dtype=np.int32), n).reshape(n, n)
    col = col[~np.eye(n, dtype=bool)]
    graph = Graph(row_ptr=np.arange(n + 1, dtype=np.int64) * (n - 1), col_idx=col, name=f"K{n}")
    opts, _ = options_of(form, None)
    got, info, _ = count_on_fresh_handle(dev, graph, 4, form, opts)
    print(f"K_{n} {form}: got {got} want {comb(n, 4)}; plan {info}", flush=True)
    assert info["wide_by_class"][2] >= 1 and info["arena_entries"] <= 0
    assert got == comb(n, 4)
