"""Local 4-cycle counts on the GPU (gm_rect_local, csrc/gm_rect_local.hip): the 4-cycles at every vertex and on every entry, in the caller's
numbering and entry order, against the plain numpy reference of tests/rect_local_ref.py -- entry by entry, vertex by vertex -- and the
total against the goldens and SglSolver("rectangle").  Every cell runs on the default copy (numbered ascending in degree), under
GM_T6_AS_NUMBERED and with its ids shuffled, and asserts what places it on its path of the kernel against the constants the library
exports (gm_constant; tests/planted_squares.py cell_path): one task against a task per range, flattened against wave-strided rows and the
tail of the unroll, 16 ids per range, more than two default ranges; K_{2, 92700}, whose hubs lie on more than 2^32 cycles; a graph without a
4-cycle; outputs left out; the other solvers of the handle; the device blocks; the refusals.  Every figure is printed before it is asserted."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

import planted_squares as P
import rect_local_ref as R
import truss_ref as TR
from common import GOLDEN, load_graph
from graphminer_amd import SglSolver, _lib, clique_local, rect_local, sgl6_raw, tc_local

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
SMALL = ["rmat6_ef4_s1", "rmat8_ef8_s42", "citeseer", "cora", "rmat10_ef16_s42"]


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def consts():
    return P.constants()


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, R per entry, R_v) of a golden graph or a planted cell, computed once and left unchanged"""
    g = P.cell_graph(name, consts()) if name in P.CELLS else load_graph(name)
    ent, rv = R.rect_local(g)
    ent.setflags(write=False)
    rv.setflags(write=False)
    return g, ent, rv


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_arrays(label, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    print(f"{label}: {len(want)} values, {bad.size} differ, first at {bad[:5].tolist()}: got {np.asarray(got)[bad[:5]].tolist()} "
          f"want {np.asarray(want)[bad[:5]].tolist()}", flush=True)
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, label


def compare(label, g, dev, want_ent, want_rv, tunes=(None, t6(AS_NUMBERED))):
    want_total = R.total(want_rv)
    with g.to_device(dev) as sym:
        for tune in tunes:
            total, rv, ent, st = rect_local(sym, tune=tune, return_stats=True)
            where = f"{label} {'as numbered' if tune else 'default copy'}"
            print(f"{where}: kernel_ms {st.kernel_ms} tasks {st.chunks} grid {st.grid}", flush=True)
            check_arrays(f"{where} entries", ent, want_ent)
            check_arrays(f"{where} R_v", rv, want_rv)
            check(f"{where} total", total, want_total)
            check(f"{where} stats.tasks", st.tasks, g.E())
            assert st.kernel_ms > 0


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs(dev, name):
    g, want_ent, want_rv = case(name)
    check(f"{name} reference total against the golden", R.total(want_rv), GOLDEN[name]["rectangle"])
    compare(name, g, dev, want_ent, want_rv)
    with g.to_device(dev) as sym:
        check(f"{name} total against SglSolver", rect_local(sym)[0], SglSolver(sym, "rectangle"))


def assert_on_path(name, g):
    for claim, holds in P.cell_path(name, g, consts()).items():
        print(f"{name}: {claim}: {holds}", flush=True)
        assert holds, claim


@pytest.mark.parametrize("name", P.CELLS)
def test_planted_cell(dev, devopt, name):
    g, want_ent, want_rv = case(name)
    assert_on_path(name, g)
    if name == "small-range":
        devopt("GM_RECT_LOCAL_RANGE", str(P.SMALL_RANGE))  # (read when the plan of a handle is built: every handle below is new)
    compare(name, g, dev, want_ent, want_rv)


@pytest.mark.parametrize("name", P.CELLS)
def test_planted_cell_shuffled(dev, devopt, name):
    g, want_ent, want_rv = case(name)
    h, newid = P.shuffled(g, seed=11)
    want_rv_h = np.empty_like(want_rv)
    want_rv_h[newid] = want_rv
    if name == "small-range":
        devopt("GM_RECT_LOCAL_RANGE", str(P.SMALL_RANGE))
    compare(f"{name} shuffled", h, dev, P.entries_to(g, newid, want_ent), want_rv_h)


def test_small_range_on_rmat10(dev, devopt):
    """64 ranges of 16 ids on the R-MAT golden of 1,024 vertices, both copies"""
    g, want_ent, want_rv = case("rmat10_ef16_s42")
    for label, h in (("degree copy", P.degree_copy(g)[0]), ("as numbered", g)):
        f = P.walk_facts(h, consts(), P.SMALL_RANGE)
        print(f"rmat10 {label}: largest centre {int(f.idx0.max())} rows, first/last id {f.key_on_first}/{f.key_on_last}, cut {f.cut_at_centre}, "
              f"gap {f.gap}, ranges credited per centre {f.max_ranges_used}", flush=True)
        assert f.key_on_first and f.key_on_last and f.cut_at_centre and f.gap and f.max_ranges_used >= 3
    devopt("GM_RECT_LOCAL_RANGE", str(P.SMALL_RANGE))
    compare("rmat10 16 ids per range", g, dev, want_ent, want_rv)


def test_hubs_beyond_32_bits(dev):
    """K_{2, 92700}: the two hubs lie on C(92700, 2) = 4,296,598,650 > 2^32 cycles, one LDS counter reaches 92,700, every entry carries 92,699"""
    n = 92700
    g = P.k2n(n)
    assert comb(n, 2) > 2 ** 32 and n > consts()["one_task"]
    want_ent = np.full(g.E(), n - 1, dtype=np.uint64)
    want_rv = np.r_[np.full(n, n - 1), [comb(n, 2)] * 2].astype(np.uint64)
    compare(f"K_2,{n}", g, dev, want_ent, want_rv, tunes=(None,))
    h, newid = P.shuffled(g, seed=5)
    want_rv_h = np.empty_like(want_rv)
    want_rv_h[newid] = want_rv
    compare(f"K_2,{n} shuffled", h, dev, want_ent, want_rv_h, tunes=(None,))


def test_no_cycle_and_nothing_out_of_place(dev):
    """a windmill of 300 triangles with 5,000 further leaves on its hub: rows of 5,600 keys, no 4-cycle; the arrays lie inside larger
    buffers whose other words keep their sentinel"""
    import torch

    g = P.windmill(300, 5000)
    ent0, rv0 = R.rect_local(g)
    assert not ent0.any() and not rv0.any() and int(np.diff(g.row_ptr).max()) == 5600
    lib, pad, sentinel = _lib.load(), 1024, -7
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            rv = torch.full((g.V() + 2 * pad,), sentinel, dtype=torch.int64, device=f"cuda:{dev}")
            ent = torch.full((g.E() + 2 * pad,), sentinel, dtype=torch.int64, device=f"cuda:{dev}")
            la, total = _lib.gm_launch(), C.c_uint64(9)
            if tune:
                la.tune[6] = tune[6]
            rc = lib.gm_rect_local(sym.handle, C.byref(la), rv.data_ptr() + 8 * pad, ent.data_ptr() + 8 * pad, C.byref(total), None)
            rv, ent = rv.cpu().numpy(), ent.cpu().numpy()
            check(f"windmill tune={tune} rc, total", (rc, int(total.value)), (_lib.GM_OK, 0))
            check(f"windmill tune={tune} non-zero entries, vertices", (int(np.count_nonzero(ent[pad:-pad])), int(np.count_nonzero(rv[pad:-pad]))), (0, 0))
            assert (rv[:pad] == sentinel).all() and (rv[-pad:] == sentinel).all() and (ent[:pad] == sentinel).all() and (ent[-pad:] == sentinel).all()


def test_outputs_left_out_and_repeated_calls(dev):
    g, want_ent, want_rv = case("centre+1")
    want_total = R.total(want_rv)
    with g.to_device(dev) as sym:
        total, rv, ent = rect_local(sym, vertex=False)
        check("entries only", (total, rv), (want_total, None))
        check_arrays("entries only", ent, want_ent)
        total, rv, ent = rect_local(sym, entries=False)
        check("vertices only", (total, ent), (want_total, None))
        check_arrays("vertices only", rv, want_rv)
        check("neither", rect_local(sym, vertex=False, entries=False), (want_total, None, None))
        first, second = rect_local(sym), rect_local(sym)
        check_arrays("entries, two calls in a row", second[2], first[2])
        check_arrays("R_v, two calls in a row", second[1], first[1])
        check_arrays("entries again", first[2], want_ent)
        check("totals", (first[0], second[0]), (want_total, want_total))


def test_other_solvers_keep_their_results_and_blocks_come_back(dev):
    from graphminer_amd._lib import dev_live_blocks

    name = "rmat10_ef16_s42"
    g, want_ent, want_rv = case(name)
    want_sup = TR.supports(g)
    before = dev_live_blocks()

    def others(sym, when):
        check(f"rectangle {when}", SglSolver(sym, "rectangle"), GOLDEN[name]["rectangle"])
        check(f"sgl6 R {when}", sgl6_raw(sym, ["R"])[3], GOLDEN[name]["rectangle"])
        check(f"sgl6 Z, R {when}", sgl6_raw(sym, ["Z", "R"])[3], GOLDEN[name]["rectangle"])
        check_arrays(f"supports {when}", tc_local(sym)[2], want_sup)
        check(f"4-clique total {when}", clique_local(sym, 4)[0], GOLDEN[name]["clique4"])
        return clique_local(sym, 4)[2], sgl6_raw(sym, ["Z"])[2]

    with g.to_device(dev) as sym:
        k4_before, z_before = others(sym, "before")
        for tune in (None, t6(AS_NUMBERED), None):
            total, rv, ent = rect_local(sym, tune=tune)
            check_arrays(f"entries between, tune={tune}", ent, want_ent)
            check_arrays(f"R_v between, tune={tune}", rv, want_rv)
        k4_after, z_after = others(sym, "after")
        check_arrays("4-clique entries before and after", k4_after, k4_before)
        check("sgl6 Z before and after", z_after, z_before)
        during = dev_live_blocks()
    with g.to_device(dev) as sym:  # the local 4-cycle counts first on a fresh handle
        check_arrays("entries first", rect_local(sym)[2], want_ent)
        check("rectangle after a first rect_local", SglSolver(sym, "rectangle"), GOLDEN[name]["rectangle"])
        check("sgl6 Z after a first rect_local", sgl6_raw(sym, ["Z"])[2], z_before)
    after = dev_live_blocks()
    print(f"live blocks: before {before} during {during} after {after}", flush=True)
    assert during > before and after == before


def test_refusals_and_the_empty_graph(dev):
    import torch

    from graphminer_amd import Graph

    lib = _lib.load()
    total = C.c_uint64(5)
    with load_graph("citeseer").to_device(dev) as sym:
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("world = 2", lib.gm_rect_local(sym.handle, C.byref(la), None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        buf = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = buf.data_ptr()
        check("d_counts", lib.gm_rect_local(sym.handle, C.byref(la), None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
        check("null handle", lib.gm_rect_local(None, None, None, None, C.byref(total), None), _lib.GM_ERR_INVALID)
        check("the total of a refused call", int(total.value), 0)
    with Graph(row_ptr=[0, 2, 3, 4], col_idx=[2, 1, 0, 0]).to_device(dev) as sym:  # row 0 descends
        check("unsorted rows", lib.gm_rect_local(sym.handle, None, None, None, C.byref(total), None), _lib.GM_ERR_INVALID)
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        total, rv, ent = rect_local(sym)
        check("no edges", (total, rv.tolist(), ent.tolist()), (0, [0, 0, 0], []))
