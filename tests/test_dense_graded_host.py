"""The dense reference of the support family and its two graded cells without a GPU (tests/dense_graded.py): the dense forms against the
sparse references on graphs both can run, the cells' DAG rows against the row lengths their names claim, and the two mutants -- a support
read one entry off, a degree read one vertex off -- which every sum the GPU tests compare must notice on the cells and cannot notice on
K_n.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import dense_graded as DG
import sgl5_ref as R5
import sgl6_ref as R6
import truss_ref as TR
import twin_graphs as T
from common import load_graph

SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
GRADED60 = [("graded60", s) for s in (1, 2, 3)]
KEYS5 = ("T", "D", "W", "A", "B", "H", "S", "P")
KEYS6 = ("X", "Y", "M", "Z", "R")
TCT_STAGE_MAX = 2048  # (the GPU tests read it from gm_constant "tct_stage_max")
MUTANT_SUMS = {"supports": (("A", "B", "W"), ("M", "X")), "degrees": (("A", "W", "S"), ("Y", "Z"))}


@functools.lru_cache(maxsize=None)
def graph(name):
    return DG.graded(60, 0.5, name[1]) if isinstance(name, tuple) else load_graph(name)


@pytest.mark.parametrize("name", SMALL + GRADED60)
def test_dense_sums_equal_the_sparse_references(name):
    g = graph(name)
    want5, want6 = R5.raw_sums(g, need=KEYS5), R6.raw_sums(g, need=KEYS6)
    got5, got6 = DG.dense_raw5(g, KEYS5), DG.dense_raw6(g, KEYS6)
    for k in KEYS5:
        print(f"{name} sgl5 {k}: dense {got5[k]} sparse {want5[k]}", flush=True)
    for k in KEYS6:
        print(f"{name} sgl6 {k}: dense {got6[k]} sparse {want6[k]}", flush=True)
    assert got5 == want5 and got6 == want6
    assert all(got5[k] > 0 for k in KEYS5) and all(got6[k] > 0 for k in KEYS6)
    with pytest.raises(ValueError):
        DG.dense_raw5(g, ("K4",))


@pytest.mark.parametrize("name", SMALL + GRADED60)
def test_dense_supports_equal_the_plain_ones(name):
    g = graph(name)
    sup, tv = DG.dense_supports(g)
    want_sup, want_tv = TR.supports(g), TR.vertex_triangles(g)
    print(f"{name}: {sup.size} entries, {int((sup != want_sup).sum())} supports differ; {tv.size} vertices, {int((tv != want_tv).sum())} T_v differ", flush=True)
    assert sup.dtype == want_sup.dtype == np.uint32 and tv.dtype == want_tv.dtype == np.uint64
    assert np.array_equal(sup, want_sup) and np.array_equal(tv, want_tv)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_finished_patterns_equal_the_loop_nests(seed):
    g = DG.graded(24, 0.5, seed)
    raw = DG.dense_raw5(g, KEYS5)
    raw["R"] = DG.dense_raw6(g, ("R",))["R"]
    raw["K4"] = R5.raw_sums(g, need=("K4",))["K4"]
    for pat in ("hourglass", "taileddiamond", "taileddiamond2", "semihouse", "5path"):
        want = R5.loops(g, pat)
        print(f"graded(24, 0.5, {seed}) {pat}: loops {want} dense closed form {R5.finish(pat, raw)}", flush=True)
        assert R5.finish(pat, raw) == want and want > 0


def test_the_sparse_reference_refuses_a_dense_graph():
    """K_700: 700 * 699 / 2 * 699 = 1.7 * 10^8 rows -- the refusal comes before any of them is made"""
    with pytest.raises(ValueError, match="dense_raw5"):
        R5.raw_sums(T.graph("complete", (700,)), need=("A",))
    assert R5.raw_sums(T.graph("complete", (40,)), need=("A",))["A"] == R5.complete_raw(40)["A"]


@functools.lru_cache(maxsize=None)
def facts(name):
    return DG.row_facts(DG.cell(name), TCT_STAGE_MAX)


@pytest.mark.parametrize("name", list(DG.CELLS))
def test_the_cells_are_where_they_claim(name):
    g, f = DG.cell(name), facts(name)
    print(f"{name} graded{DG.CELLS[name]}: {g.V()} vertices, {g.E() // 2} undirected edges, {DG.reference(name)['raw5']['T']} triangles, "
          f"longest DAG row {f['longest']}, rows in (1024, {TCT_STAGE_MAX}] {f['stage']}, rows beyond {f['beyond']}; distinct supports "
          f"{f['supports']} (on the entries of the stage rows {f['stage_supports']}, of the rows beyond {f['beyond_supports']}), distinct "
          f"degrees {f['degrees']} (of the keys of the stage rows {f['stage_degrees']}, of the rows beyond {f['beyond_degrees']})", flush=True)
    if name in ("stage", "corner"):
        assert f["stage"] >= 64 and f["beyond"] == 0
        assert f["stage_supports"] >= 64 and f["stage_degrees"] >= 64
        if name == "corner":  # (what lets the library take a corner of 1024 vertices: tests/dense_graded.py CELLS)
            assert (g.V() - 1024) % 32 == 0 and f["longest"] <= TCT_STAGE_MAX
    else:
        assert f["beyond"] >= 64
        assert f["beyond_supports"] >= 64 and f["beyond_degrees"] >= 64


def test_the_beyond_cell_is_the_smallest_of_its_kind():
    """one step of 50 vertices down no weight range tried keeps 64 rows beyond the stage AND 64 distinct supports and degrees on them"""
    n, lo, _ = DG.CELLS["beyond"]
    assert n % 50 == 0
    for lo_ in (lo, 0.98, 0.985, 0.99):
        f = DG.row_facts(DG.graded(n - 50, lo_, n - 50), TCT_STAGE_MAX)
        print(f"graded({n - 50}, {lo_}, {n - 50}): rows beyond {f['beyond']}, supports {f['beyond_supports']}, degrees {f['beyond_degrees']}", flush=True)
        assert not (f["beyond"] >= 64 and f["beyond_supports"] >= 64 and f["beyond_degrees"] >= 64)


@pytest.mark.parametrize("mutant", list(MUTANT_SUMS))
@pytest.mark.parametrize("name", list(DG.CELLS))
def test_the_cells_can_tell_a_misplaced_read(name, mutant):
    g, ref = DG.cell(name), DG.reference(name)
    k5, k6 = MUTANT_SUMS[mutant]
    got5, got6 = DG.dense_raw5(g, k5, mutant=mutant), DG.dense_raw6(g, k6, mutant=mutant)
    for k in k5:
        print(f"{name} mutant {mutant} sgl5 {k}: {got5[k]} true {ref['raw5'][k]}", flush=True)
        assert got5[k] != ref["raw5"][k], k
    for k in k6:
        print(f"{name} mutant {mutant} sgl6 {k}: {got6[k]} true {ref['raw6'][k]}", flush=True)
        assert got6[k] != ref["raw6"][k], k
    if mutant == "supports":  # per entry too: what the tc_local comparisons rest on
        rot = DG._supports_of(g, DG._Dense(g, mutant))[0]
        print(f"{name} mutant {mutant}: {int((rot != ref['sup']).sum())} of {rot.size} entries differ", flush=True)
        assert int((rot != ref["sup"]).sum()) > rot.size // 2


def test_the_mutants_change_nothing_on_a_complete_graph():
    # every support of K_n is n - 2 and every degree n - 1: a read at a wrong entry or vertex returns the right value.  This is why the
    # K_1300 / K_2060 / K_1100 cells of the GPU tests stay only as closed-form checks beside the graded cells.
    g = T.graph("complete", (40,))
    true5, true6 = DG.dense_raw5(g, KEYS5), DG.dense_raw6(g, KEYS6)
    want = R5.complete_raw(40)
    assert all(true5[k] == want[k] for k in ("T", "D", "W", "A", "B", "H", "S"))
    for mutant in MUTANT_SUMS:
        got5, got6 = DG.dense_raw5(g, KEYS5, mutant=mutant), DG.dense_raw6(g, KEYS6, mutant=mutant)
        print(f"K_40 mutant {mutant}: sgl5 {got5 == true5} sgl6 {got6 == true6}", flush=True)
        assert got5 == true5 and got6 == true6
