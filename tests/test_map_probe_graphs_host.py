"""The planted graphs of the map kernels (tests/map_probe_graphs.py), checked on the CPU: every cell's claims about its path hold against the
sizes the library exports, its reference count is not zero, a closed form agrees with the plain reference wherever both are affordable, the
two sides of a boundary land on different plans, and the restated plans agree with csrc/gm_centre_plan.h on what the header's own host check
pins (the literal range cases of tests/centre_plan_host_check.cc, restated through rect_ranges).  Needs the built library for gm_constant,
no GPU.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import map_probe_graphs as M
import rect_local_ref as R


@functools.lru_cache(maxsize=None)
def consts():
    return M.constants()


@functools.lru_cache(maxsize=None)
def cell(name):
    return M.build(name, consts())


def test_constants_are_exported():
    c = consts()
    print(c, flush=True)
    assert all(v > 0 for v in c.values())
    assert c["one_task_rows"] % 64 == 0 and c["tile_group"] % 64 == 0 and c["mark_window"] % c["tile_group"] == 0
    assert c["house_fw16_rows"] < c["one_task_rows"] and c["long_row"] < c["house_wg_row"]
    # the widths the fields of a one-task centre of the house are given: n rows and S <= n (n - 1) fit 6 + 10 and 11 + 21 bits
    f, t = c["house_fw16_rows"], c["one_task_rows"]
    assert f < 2 ** 6 and f * (f - 1) < 2 ** 10 and t < 2 ** 11 and t * (t - 1) < 2 ** 21


@pytest.mark.parametrize("name", M.CELLS)
def test_cell_claims(name):
    x = cell(name)
    for claim, holds in x.claims.items():
        print(f"{name}: {claim}: {holds}", flush=True)
    assert x.claims and all(x.claims.values()), [k for k, v in x.claims.items() if not v]
    want = M.reference(x)
    print(f"{name}: {x.graph.V()} vertices {x.graph.E()} entries, options {x.options}, reference {want}", flush=True)
    assert want > 0
    assert x.graph.E() <= 1_200_000
    if name.startswith("rect-cut"):
        print(f"{name}: centres that carry a 4-cycle: {x.centres}", flush=True)
        assert "first ids of the zone" in x.centres and "+1" in x.centres and (("+0" in x.centres) == (name == "rect-cut-1-range"))
    if x.closed_form is not None and x.graph.E() < M.BIG_REFERENCE:
        assert R.total(R.rect_local(x.graph)[1]) == x.closed_form
    if x.pattern == "house":
        assert int((np.diff(x.graph.row_ptr) >= 2).sum()) <= 2500


def test_total_by_pairs_against_the_other_references():
    """rect_local_ref.total_by_pairs, the reference of the cut cells, against rect_local and the listing of every 4-cycle"""
    from common import random_graph

    g = random_graph(60, 400, 5)
    want = R.total(R.brute_force(g)[1])
    print(f"G(60, 400 draws): brute force {want}, rect_local {R.total(R.rect_local(g)[1])}, pairs {R.total_by_pairs(g)}", flush=True)
    assert want > 0 and R.total(R.rect_local(g)[1]) == want and R.total_by_pairs(g) == want
    for name in ("rect-rows", "rect-one-task-rows+1", "rect-range-edges"):
        x = cell(name)
        assert R.total_by_pairs(x.graph) == R.total(R.rect_local(x.graph)[1]), name


def public(name, copy="default"):
    return M.plan_public(cell(name).plans[copy])


PAIRS = [("rect-cut-1-range", "rect-cut-2-ranges"), ("rect-width-2^8-1", "rect-width-2^8"), ("rect-width-2^16-1", "rect-width-2^16"), ("rect-one-task-rows", "rect-one-task-rows+1"),
         ("house-fields-one-task", "house-fields-one-task+1"), ("house-ranges-1-fw16", "house-ranges-2-fw16"), ("house-ranges-4-fw32", "house-ranges-5-fw32")]


@pytest.mark.parametrize("a,b", PAIRS)
def test_two_sides_of_a_boundary_differ_in_plan(a, b):
    pa, pb = public(a), public(b)
    print(a, pa, b, pb, sep="\n", flush=True)
    differ = [k for k in ("n", "lb", "lds_range_tasks", "lds_whole_tasks") if pa.get(k) != pb.get(k)]
    assert differ, "the two cells would run the same path"


def test_fields_and_rows_differ_where_the_plan_cannot():
    """fw16 / fw32 fields and queued / strided rows are chosen inside the kernel from a centre's rows: the cells differ in those"""
    c = consts()
    a, b = cell("house-fields-fw16"), cell("house-fields-fw16+1")
    assert int(a.plans["default"]["deg"][a.twins[0]]) == c["house_fw16_rows"] and int(b.plans["default"]["deg"][b.twins[0]]) == c["house_fw16_rows"] + 1
    rows = {}
    for name in ("house-row-wg-1", "house-row-wg", "house-queue-1", "house-queue", "house-queue+8"):
        x = cell(name)
        deg = np.diff(x.graph.row_ptr)
        nb = x.graph.col_idx[x.graph.row_ptr[x.v0]:x.graph.row_ptr[x.v0 + 1]]
        rows[name] = int((deg[nb] >= c["house_wg_row"]).sum())
    print(rows, flush=True)
    assert rows == {"house-row-wg-1": 0, "house-row-wg": 2, "house-queue-1": c["house_wg_queue"] - 1, "house-queue": c["house_wg_queue"], "house-queue+8": c["house_wg_queue"] + 8}


def test_rect_ranges_restates_the_header():
    """the literal cases of tests/centre_plan_host_check.cc (blocks of 16 ids, 200 ids) through the Python restatement"""
    c = {"rect_block": 16}

    def ranges(bmax, max_ranges=7, nv=200):
        deg = np.zeros(nv, dtype=np.int64)
        for b, m in enumerate(bmax):
            deg[max(nv - (b + 1) * 16, 0)] = m
        return M.rect_ranges(nv, deg, c, max_ranges)

    small = [10] * 13
    assert ranges(small) == ([0, 8, 72, 136, 200], [3, 3, 3, 3])
    assert ranges(small, 2) == ([72, 136, 200], [3, 3])
    assert ranges([70000, 300] + small[2:]) == ([0, 24, 88, 152, 184, 200], [3, 3, 3, 4, 5])
    assert ranges(small[:3] + [256] + small[4:]) == ([0, 8, 72, 136, 168, 200], [3, 3, 3, 4, 4])
    assert ranges(small[:4] + [256] + small[5:]) == ([0, 40, 104, 136, 200], [3, 3, 4, 3])
    assert ranges([10, 65536] + small[2:]) == ([0, 40, 104, 168, 184, 200], [3, 3, 3, 5, 5])
