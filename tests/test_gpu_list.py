"""Triangle listing on the GPU (gm_tc_list, csrc/gm_list.hip): every triangle once, as a < b < c of the caller's numbering, against the plain
numpy list of tests/list_ref.py; the windows of one handle tile its fixed order; the 64-lane tile, the flattened / whole-wave threshold,
rows of more than 2048 entries, slots past 2^32, shuffled and offset numberings, the other solvers of the handle, the refusals; the
one-call list row for row against the ordered reference (list_ref_ordered: the documented order by a walk of its own); windows that start
and end on batch and ring-flush boundaries, every one with guard words in front of it and behind it (tests/list_windows.py).
Every value is printed before it is asserted."""
import ctypes as C
import functools
import itertools
from math import comb

import numpy as np
import pytest

import twin_graphs as T
from common import GOLDEN, check_rows, list_windows, load_graph
from graphminer_amd import Graph, SglSolver, TCSolver, _lib, ktruss, tc_list, tc_local
from graphminer_amd.rmat import csr_from_pairs
from list_ref import list_ref, list_ref_ordered, sort_rows
from list_windows import U64_MAX, guarded_window, tc_call

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
# csrc/gm_mine.h kListWholeWave: a streamed list of this many keys or more is strided by the whole wave, a shorter one is flattened.  The
# longest streamed list of K_n is N+(1), n - 2 keys: K_65 is the last complete graph that is all flattened, K_66 the first with a whole-wave list
WHOLE_WAVE = 64
SENTINEL = -7


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def ref(name):
    r = list_ref(load_graph(name))
    r.setflags(write=False)
    return r


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def ascending(tri):
    return bool((tri[:, 0] < tri[:, 1]).all() and (tri[:, 1] < tri[:, 2]).all())


def raw_call(sym, first, cap, buf, la=None):
    """gm_tc_list itself: (status, total, n_written); buf a torch int32 tensor or None"""
    total, written = C.c_uint64(99), C.c_uint64(99)
    rc = _lib.load().gm_tc_list(sym.handle, C.byref(la) if la is not None else None, first, cap, buf.data_ptr() if buf is not None else None,
                                C.byref(total), C.byref(written), None)
    return rc, int(total.value), int(written.value)


def windows(sym, size, upto):
    return list_windows(sym, size, upto, SENTINEL)


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs(dev, name):
    g = load_graph(name)
    want = ref(name)
    with g.to_device(dev) as sym:
        total, tri, st = tc_list(sym, return_stats=True)
        check_rows(f"{name} sorted list", sort_rows(tri), want)
        check(f"{name} every row a < b < c", ascending(tri), True)
        check(f"{name} total", total, GOLDEN[name]["motif3"][1])
        check(f"{name} n_written", len(tri), total)
        check(f"{name} stats.tasks", st.tasks, g.E())
        print(f"{name} kernel_ms {st.kernel_ms}", flush=True)
        assert st.kernel_ms > 0
        with sym.orient() as dag:
            check(f"{name} total against TCSolver", total, TCSolver(dag))
        total2, tri2 = tc_list(sym)
        check(f"{name} second call total", total2, total)
        check_rows(f"{name} second call, the same sequence", tri2, tri)


def test_count_only_and_guard_words(dev):
    import torch

    name = "rmat10_ef16_s42"
    T_ = GOLDEN[name]["motif3"][1]
    with load_graph(name).to_device(dev) as sym:
        check("count only", raw_call(sym, 0, 12345, None), (_lib.GM_OK, T_, 0))
        full = tc_list(sym)[1]
        call = tc_call(sym)
        # (guarded_window asserts: both pads all sentinel, exactly 3 n_written ints changed, nothing behind row n_written)
        rc, total, n, rows = guarded_window(call, 3, 0, T_ - 5, rows=T_ + 20, sentinel=SENTINEL)
        check("cap = T - 5", (rc, total, n), (_lib.GM_OK, T_, T_ - 5))
        check_rows("the first T - 5 rows", rows, full[:T_ - 5])
        rc, total, n, rows = guarded_window(call, 3, 1000, 77, sentinel=SENTINEL)
        check("a window in the middle", (rc, total, n), (_lib.GM_OK, T_, 77))
        check_rows("rows 1000 .. 1076", rows, full[1000:1077])
        for first in (T_, T_ + 1, 2**40):
            rc, total, n, rows = guarded_window(call, 3, first, 10, sentinel=SENTINEL)
            check(f"first = {first}", (rc, total, n, rows.shape), (_lib.GM_OK, T_, 0, (0, 3)))
        rc, total, n, rows = guarded_window(call, 3, T_ - 5, U64_MAX, rows=10, sentinel=SENTINEL)
        check("first = T - 5, cap = 2^64 - 1", (rc, total, n), (_lib.GM_OK, T_, 5))
        check_rows("the last five rows", rows, full[T_ - 5:])
        rc, total, n, rows = guarded_window(call, 3, 0, U64_MAX, rows=T_, sentinel=SENTINEL)
        check("first = 0, cap = 2^64 - 1", (rc, total, n), (_lib.GM_OK, T_, T_))
        check_rows("the whole list", rows, full)
        buf = torch.full((64,), SENTINEL, dtype=torch.int32, device=f"cuda:{dev}")
        check("first = 2^64 - 1, cap = 2^64 - 1", raw_call(sym, U64_MAX, U64_MAX, buf), (_lib.GM_OK, T_, 0))
        check("nothing written", bool((buf.cpu().numpy() == SENTINEL).all()), True)


@pytest.mark.parametrize("name", ["cora", "rmat10_ef16_s42"])
def test_windows_tile_the_list(dev, name):
    with load_graph(name).to_device(dev) as sym:
        total, full = tc_list(sym)
        check(f"{name} total", total, GOLDEN[name]["motif3"][1])
        for size, upto in ((1, min(200, total)), (7, total), (64, total), (1000, total)):
            check_rows(f"{name} windows of {size}", windows(sym, size, upto), full[:upto])
        parts = [tc_list(sym, first=f, cap=1000)[1] for f in range(0, total, 1000)]
        check_rows(f"{name} windows of 1000 through the mirror", np.concatenate(parts), full)


@pytest.mark.parametrize("n", sorted({3, 4, 63, 64, 65, 66, 130, 200, WHOLE_WAVE + 1, WHOLE_WAVE + 2}))
def test_complete_graphs_cross_the_tile_and_the_threshold(dev, n):
    """K_n: DAG rows of every length 0 .. n - 1, streamed lists of every length 0 .. n - 2"""
    want = np.array(list(itertools.combinations(range(n), 3)), dtype=np.int32).reshape(-1, 3)
    with T.graph("complete", (n,)).to_device(dev) as sym:
        total, tri = tc_list(sym)
        check(f"K_{n} total", total, comb(n, 3))
        check_rows(f"K_{n} rows", sort_rows(tri), want)
        upto = min(total, 2000)
        check_rows(f"K_{n} windows of 50", windows(sym, 50, upto), tri[:upto])


KAB = (2100, 2101)
KAB_INNER = [(0, 1), (1, 2), (0, 2)]


def kab_plus_triangle():
    n, s, d = T.pairs("kab", KAB)
    return csr_from_pairs(n, np.concatenate([s, [x for x, _ in KAB_INNER]]).astype(np.uint64),
                          np.concatenate([d, [y for _, y in KAB_INNER]]).astype(np.uint64))


def test_rows_beyond_2048_entries(dev):
    """K_{2100,2101} + one triangle inside the 2100 side: the DAG rows of the 2101 side have 2100 entries, more than the 2048-entry LDS stage
    of the other triangle kernels; the listing stages no row (the longer list is bisected in global memory), so no size is special to it"""
    a, b = KAB
    g = kab_plus_triangle()
    n, inner = g.V(), KAB_INNER
    want = np.array([(0, 1, 2)] + [(x, y, w) for x, y in inner for w in range(a, n)], dtype=np.int32)
    want = sort_rows(want)
    check("expected triangles", len(want), 6304)
    with g.to_device(dev) as sym:
        total, tri = tc_list(sym)
        check("total", total, 6304)
        check_rows("rows", sort_rows(tri), want)


def test_offsets_past_2_32(dev):
    n = 3000
    T_ = comb(n, 3)
    check("T of K_3000", T_, 4495501000)
    with T.graph("complete", (n,)).to_device(dev) as sym:
        check("count only", raw_call(sym, 0, 0, None), (_lib.GM_OK, T_, 0))
        total, both = tc_list(sym, first=2**32 - 100, cap=200)
        check("window across 2^32", (total, both.shape), (T_, (200, 3)))
        check("valid rows", bool(ascending(both) and both.min() >= 0 and both.max() < n), True)
        check("distinct rows", len(np.unique(both, axis=0)), 200)
        lo, hi = tc_list(sym, first=2**32 - 100, cap=100)[1], tc_list(sym, first=2**32, cap=100)[1]
        check_rows("two windows of 100", np.concatenate([lo, hi]), both)
        total, tail = tc_list(sym, first=T_ - 3, cap=10)
        check("the last three", (total, tail.shape), (T_, (3, 3)))
        check("valid last rows", bool(ascending(tail) and tail.max() < n and len(np.unique(tail, axis=0)) == 3), True)


def permuted_rmat10():
    g = load_graph("rmat10_ef16_s42")
    perm = np.random.default_rng(5).permutation(g.V()).astype(np.uint64)
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    return csr_from_pairs(g.V(), perm[src], perm[g.col_idx])


@pytest.mark.parametrize("which", ["rmat10 permuted", "multipartite (3, 40) at 517 of 1000"])
def test_the_callers_numbering(dev, which):
    g = permuted_rmat10() if which.startswith("rmat10") else T.graph("multipartite", (3, 40), nv=1000, offset=517)
    want = list_ref(g)
    assert len(want) == (GOLDEN["rmat10_ef16_s42"]["motif3"][1] if which.startswith("rmat10") else 40**3)
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            total, tri = tc_list(sym, tune=tune)
            check(f"{which} tune={tune} total", total, len(want))
            check_rows(f"{which} tune={tune} rows", sort_rows(tri), want)


# ---- the documented order, against a reference that walks it itself -------------------------------------------------------------------------
NUMBERED = ["rmat10 permuted", "multipartite (3, 40) at 517 of 1000"]
ORDERED = SMALL + ["K_66", "K_200"] + NUMBERED + ["K_{2100,2101} + triangle"]


def named_graph(name):
    if name in SMALL:
        return load_graph(name)
    if name.startswith("K_{"):
        return kab_plus_triangle()
    if name.startswith("K_"):
        return T.graph("complete", (int(name[2:]),))
    return permuted_rmat10() if name.startswith("rmat10") else T.graph("multipartite", (3, 40), nv=1000, offset=517)


@functools.lru_cache(maxsize=None)
def ordered(name):
    """(the list in the documented order, the first slot of every oriented entry): tests/list_ref.py, computed once, read-only"""
    tri, off = list_ref_ordered(named_graph(name))
    tri.setflags(write=False)
    off.setflags(write=False)
    return tri, off


@pytest.mark.parametrize("name", ORDERED)
def test_the_documented_order(dev, name):
    """the one-call list row for row: ascending entry (u, v) of the oriented copy as numbered, then ascending w"""
    want, off = ordered(name)
    print(f"{name}: {len(want)} rows over {len(off) - 1} oriented entries", flush=True)
    with named_graph(name).to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)) if name in NUMBERED else (None,):
            total, tri = tc_list(sym, tune=tune)
            check(f"{name} tune={tune} total", total, len(want))
            check_rows(f"{name} tune={tune} rows in the documented order", tri, want)


# ---- windows at batch and flush boundaries ---------------------------------------------------------------------------------------------------
WINDOW_CAPS = (1, 2, 63, 64, 65, 127, 128, 129)


def batch_slots(off):
    """the first slot of every batch of 64 consecutive oriented entries (and T behind the last one)"""
    ne = len(off) - 1
    return off[np.minimum(np.arange((ne + 63) // 64 + 1) * 64, ne)]


@pytest.mark.parametrize("name", ["rmat10_ef16_s42", "K_200", "K_{2100,2101} + triangle"])
def test_windows_at_batch_and_flush_boundaries(dev, name):
    """list_kernel<true> walks a batch from its first slot whatever the window: a window that starts or ends on a batch's first slot, one
    slot to either side, or on a slot at which the ring flushes 64 rows, with guard words in front of it and behind it"""
    want, off = ordered(name)
    T_ = len(want)
    boff = batch_slots(off)
    rows_of = np.diff(boff)
    full = np.flatnonzero(rows_of > 0)
    fat = int(np.argmax(rows_of))
    empty_next_to_full = [int(b) for b in np.flatnonzero(rows_of == 0) if 0 < b < len(rows_of) - 1 and rows_of[b - 1] > 0 and rows_of[b + 1] > 0]
    print(f"{name}: T {T_}, {len(rows_of)} batches, {len(full)} non-empty, the fattest {fat} holds {int(rows_of[fat])} rows, "
          f"empty between two non-empty: {empty_next_to_full[:5]}", flush=True)
    assert boff[-1] == T_
    if name.startswith("rmat10"):  # irregular: no batch is empty (its 165 batches hold 61 .. 1034 rows), the ring flushes a different number of times in each
        assert rows_of[fat] >= 256 and rows_of[full].min() * 8 <= rows_of[fat]
    elif name.startswith("K_{"):  # a row of 2100 entries is 33 batches and only its first two entries hold rows: runs of empty batches
        assert len(empty_next_to_full) == 0 and len(full) * 16 <= len(rows_of)
        empty_next_to_full = [int(b) + 1 for b in full[:-1] if rows_of[b + 1] == 0][1:4]  # (the empty batch behind a non-empty one)
        assert len(empty_next_to_full) == 3 and all(0 < boff[b] < T_ for b in empty_next_to_full)
    else:
        assert rows_of[fat] >= 2000 and len(full) == len(rows_of), "K_200: batches of thousands of rows, none empty"
    seeded = np.random.default_rng(11).choice(len(rows_of), 3, replace=False)
    s = int(boff[fat])
    bounds = [int(boff[full[0]]), s, int(boff[full[-1]])] + [int(boff[b]) for b in seeded]
    if rows_of[fat] >= 256:  # the ring's flushes inside the fattest batch
        bounds += [s + 64, s + 128, s + 64 * (int(rows_of[fat]) // 128)]
    starts = sorted({min(max(b + o, 0), T_ - 1) for b in bounds for o in (-1, 0, 1)})
    print(f"{name}: boundaries {bounds}, {len(starts)} starts x {len(WINDOW_CAPS)} caps", flush=True)
    with named_graph(name).to_device(dev) as sym:
        call = tc_call(sym)

        def window(label, first, cap):
            rc, total, n, rows = guarded_window(call, 3, first, cap, sentinel=SENTINEL)
            assert (rc, total, n) == (_lib.GM_OK, T_, min(cap, T_ - first)), (label, first, cap, rc, total, n)
            if not np.array_equal(rows, want[first:first + cap]):
                check_rows(f"{name} {label} first={first} cap={cap}", rows, want[first:first + cap])

        for first in starts:
            for cap in WINDOW_CAPS:
                window("boundary window", first, cap)
        window("exactly the fattest batch", s, int(rows_of[fat]))
        window("the fattest batch and a row on either side", max(s - 1, 0), int(rows_of[fat]) + 2)
        for b in empty_next_to_full[:3]:  # the last row before an empty batch and the first one behind it, and nothing else
            assert boff[b] == boff[b + 1] and 0 < boff[b] < T_
            window(f"around the empty batch {b}", int(boff[b]) - 1, 2)
            window(f"behind the empty batch {b}", int(boff[b]), 1)
            window(f"before the empty batch {b}", int(boff[b]) - 1, 1)
    print(f"{name}: every window is the reference's slice", flush=True)


def test_neighbours_on_the_handle(dev):
    name = "rmat10_ef16_s42"
    g = load_graph(name)
    with g.to_device(dev) as fresh:
        want_total, want_tri = tc_list(fresh)
    with g.to_device(dev) as fresh:
        want_local = tc_local(fresh)
    with g.to_device(dev) as fresh:
        want_truss = ktruss(fresh, 4)
    check("fresh total", want_total, GOLDEN[name]["motif3"][1])

    def same_list(label, sym):
        total, tri = tc_list(sym)
        check(label + " total", total, want_total)
        check_rows(label + " sequence", tri, want_tri)

    def same_local(label, sym):
        total, tv, sup = tc_local(sym)
        check(label, (total, bool(np.array_equal(tv, want_local[1])), bool(np.array_equal(sup, want_local[2]))), (want_local[0], True, True))

    def same_truss(label, sym):
        n, sup, _ = ktruss(sym, 4)
        check(label, (n, bool(np.array_equal(sup, want_truss[1]))), (want_truss[0], True))

    with g.to_device(dev) as sym:  # the list first, then each neighbour, the list after each
        same_list("list first", sym)
        same_local("tc_local after the list", sym)
        same_list("list after tc_local", sym)
        check("diamond after the list", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
        same_list("list after diamond", sym)
        same_truss("ktruss after the list", sym)
        same_list("list after ktruss", sym)
    for label, other in (("tc_local", same_local), ("ktruss", same_truss)):
        with g.to_device(dev) as sym:  # the neighbour first on a fresh handle
            other(f"{label} first", sym)
            same_list(f"list after a first {label}", sym)
            other(f"{label} again", sym)
    with g.to_device(dev) as sym:
        check("diamond first", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
        same_list("list after a first diamond", sym)
        check("diamond again", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])


def test_refusals_and_the_empty_graph(dev):
    import torch

    g = load_graph("citeseer")
    buf = torch.zeros(64, dtype=torch.int32, device=f"cuda:{dev}")
    with g.to_device(dev) as sym:
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("world = 2", raw_call(sym, 0, 4, buf, la), (_lib.GM_ERR_UNSUPPORTED, 0, 0))
        la = _lib.gm_launch()
        counts = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = counts.data_ptr()
        check("d_counts", raw_call(sym, 0, 4, buf, la), (_lib.GM_ERR_UNSUPPORTED, 0, 0))
        check("the handle still lists", tc_list(sym)[0], 1166)
    rev = g.col_idx.copy()
    for v in range(g.V()):
        a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
        rev[a:b] = rev[a:b][::-1]
    with Graph(row_ptr=g.row_ptr.copy(), col_idx=rev, name="citeseer_descending").to_device(dev) as sym:
        check("unsorted rows", raw_call(sym, 0, 4, buf), (_lib.GM_ERR_INVALID, 0, 0))
        assert b"ascending" in _lib.load().gm_last_error()
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        check("no edges", raw_call(sym, 0, 4, buf), (_lib.GM_OK, 0, 0))
        total, tri = tc_list(sym)
        check("no edges, mirror", (total, tri.shape), (0, (0, 3)))
