"""The map kernels of the rectangle and the house (csrc/gm_mine.hip: rect_lds_kernel + rect_acc_kernel, house_lds_kernel + house_acc_kernel;
pent_acc_kernel shares the global maps) on the planted graphs of tests/map_probe_graphs.py: packed counters on the last value of their width,
centres, rows and ends on both sides of every size at which the kernels change path.  For every cell, on a fresh handle per form (plans and
options are cached per handle):

  path first  the plan the library built (map_plan_info: ranges, widths, tasks by kind) equals the plan restated on the CPU from the sizes the
              library exports, and every claim of the cell holds -- BEFORE a count is compared: a cell that lands on another path fails
  counts      every form against tests/rect_local_ref.py / tests/house_ref.py, which know nothing of centres, ranges or widths

Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import map_probe_graphs as M
import oracle as O
import rect_local_ref as R
from graphminer_amd import MotifSolver, SglSolver, map_plan_info

pytestmark = pytest.mark.gpu
AS_NUMBERED, GLOBAL_MAPS, FLAT = 0x200, 0x20000, 0x800
M64 = 2 ** 64


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def consts():
    return M.constants()


@functools.lru_cache(maxsize=None)
def case(name):
    """(cell, reference count), computed once and left unchanged"""
    cell = M.build(name, consts())
    return cell, M.reference(cell)


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def assert_claims(name, cell):
    for claim, holds in cell.claims.items():
        print(f"{name}: {claim}: {holds}", flush=True)
        assert holds, claim


def ranks(fn, world=3):
    return sum(fn(rank=r, world=world) for r in range(world)) % M64


def run_form(label, g, dev, pattern, tune, want, plan=None):
    """one form on a fresh handle: the count, then -- where the form builds the LDS plan -- the plan; the plan is asserted first"""
    with g.to_device(dev) as sym:
        got, st = SglSolver(sym, pattern, tune=tune, return_stats=True)
        print(f"{label}: kernel_ms {st.kernel_ms:.3f} tasks {st.chunks} count {got} (reference {want})", flush=True)
        if plan is not None:
            check(f"{label} plan", map_plan_info(sym, pattern), M.plan_public(plan))
        check(label, got, want)


@pytest.mark.parametrize("name", M.RECT_CELLS)
def test_rectangle_cell(dev, devopt, name):
    cell, want = case(name)
    g = cell.graph
    assert_claims(name, cell)
    for k, v in cell.options.items():
        devopt(k, v)
    run_form(f"{name} default", g, dev, "rectangle", None, want, cell.plans["default"])
    run_form(f"{name} as numbered", g, dev, "rectangle", t6(AS_NUMBERED), want, cell.plans["as numbered"])
    run_form(f"{name} global maps", g, dev, "rectangle", t6(GLOBAL_MAPS), want)
    if cell.slow_forms:  # (left out of the two 2^16 cells ONLY: the flattened form intersects two lists for each of the 2^31 wedges of a hub)
        run_form(f"{name} flat", g, dev, "rectangle", t6(FLAT), want)
    with g.to_device(dev) as sym:
        check(f"{name} three ranks", ranks(lambda **kw: SglSolver(sym, "rectangle", **kw)), want)
    with g.to_device(dev) as sym:  # (the cells hold no triangle: the vertex-induced 4-cycles of the 4-motif are the edge-induced ones)
        m4 = MotifSolver(sym, 4)
        print(f"{name} 4-motif: {m4}", flush=True)
        check(f"{name} 4-motif, no diamond and no 4-clique", m4[4:], [0, 0])
        check(f"{name} 4-motif, 4-cycles", m4[3], want)
    if cell.options:  # the cell needs an option to reach its path: the same graph at the default threshold, against its own restated plan
        devopt(None)
        from planted_squares import degree_copy

        run_form(f"{name} default threshold", g, dev, "rectangle", None, want, M.rect_plan(degree_copy(g)[0], consts()))


@pytest.mark.parametrize("name", M.HOUSE_CELLS)
def test_house_cell(dev, devopt, name):
    cell, want = case(name)
    g = cell.graph
    assert_claims(name, cell)
    for k, v in cell.options.items():
        devopt(k, v)
    run_form(f"{name} default", g, dev, "house", None, want, cell.plans["default"])
    run_form(f"{name} global maps", g, dev, "house", t6(GLOBAL_MAPS), want)
    if cell.slow_forms:  # (left out of the cliques of a thousand vertices, the queue cells and the cut cell: the flattened form takes one task per
        # (v0, v1, v3), 10^9 of them in K_1024 and 10^8 under 66 .. 200 rows of a thousand keys)
        run_form(f"{name} flat", g, dev, "house", t6(FLAT), want)
    with g.to_device(dev) as sym:
        check(f"{name} three ranks", ranks(lambda **kw: SglSolver(sym, "house", **kw)), want)
    if cell.options:
        devopt(None)
        run_form(f"{name} default threshold", g, dev, "house", None, want, M.house_plan(g, consts()))


def test_plan_info_before_a_plan_and_for_other_patterns(dev, devopt):
    """gm_map_plan_info builds nothing: no plan before a first call with the maps in LDS (a call with every end in the global maps makes
    none), none for a pattern without one; afterwards the rectangle's plan of either copy and the house's are reported side by side"""
    from graphminer_amd import GraphMinerError

    cell, want = case("rect-width-2^8-1")
    devopt("GM_RECT_LDS_MIN", "1")
    with cell.graph.to_device(dev) as sym:
        for pattern in ("rectangle", "house", "pentagon", "diamond"):
            with pytest.raises(GraphMinerError):
                map_plan_info(sym, pattern)
        check("global maps", SglSolver(sym, "rectangle", tune=t6(GLOBAL_MAPS)), want)
        with pytest.raises(GraphMinerError):
            map_plan_info(sym, "rectangle")
        check("default", SglSolver(sym, "rectangle"), want)
        check("plan", map_plan_info(sym, "rectangle"), M.plan_public(cell.plans["default"]))
        with pytest.raises(GraphMinerError):
            map_plan_info(sym, "house")
        check("house of a bipartite graph", SglSolver(sym, "house"), 0)
        check("house plan", map_plan_info(sym, "house"), M.plan_public(M.house_plan(cell.graph, consts(), lds_min=1)))
        check("rectangle plan, still", map_plan_info(sym, "rectangle"), M.plan_public(cell.plans["default"]))


REUSE = ["house-fields-fw16", "house-fields-fw16+1"]


@functools.lru_cache(maxsize=None)
def reuse_case(name):
    import house_ref as H

    g = case(name)[0].graph
    return g, {"rectangle": R.total(R.rect_local(g)[1]), "house": H.house(g), "pentagon": O.pentagon(O.OGraph(g.row_ptr, g.col_idx))}


@pytest.mark.parametrize("name", REUSE)
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_maps_are_left_zeroed_between_kernels(dev, devopt, name, order):
    """rectangle, pentagon, rectangle (global maps), house, pentagon, rectangle on ONE handle, and the same reversed: the acc kernels of the three
    patterns share the global maps of the handle, and every launch must leave them zeroed for the next"""
    g, want = reuse_case(name)
    print(f"{name}: {want}", flush=True)
    assert all(v > 0 for v in want.values())
    devopt("GM_RECT_LDS_MIN", "1")
    seq = [("rectangle", None), ("pentagon", None), ("rectangle", t6(GLOBAL_MAPS)), ("house", None), ("pentagon", None), ("rectangle", None)]
    if order == "reversed":
        seq = seq[::-1]
    with g.to_device(dev) as sym:
        for i, (pattern, tune) in enumerate(seq):
            check(f"{name} {order} step {i}: {pattern}{' global maps' if tune else ''}", SglSolver(sym, pattern, tune=tune), want[pattern])
        for pattern in ("house", "rectangle"):
            check(f"{name} {order} {pattern} global maps, last", SglSolver(sym, pattern, tune=t6(GLOBAL_MAPS)), want[pattern])
