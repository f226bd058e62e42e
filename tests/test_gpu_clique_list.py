"""k-clique listing on the GPU (gm_clique_list, csrc/gm_clique_list.hip): every k-clique once, k ascending ids of the caller's numbering, in
the documented order, against the plain reference of tests/clique_list_ref.py; count only and guard words; the windows of one (handle, k)
tile its fixed order; complete graphs by unranking, slots past 2^32; planted graphs (tests/planted_cliques.py) with a root's row on both
sides of every row-length constant the kernels export and beyond 2048 entries; shuffled and offset numberings; the other solvers of the
handle; the refusals.  Every value is printed before it is asserted."""
import ctypes as C
import functools
import itertools
from math import comb

import numpy as np
import pytest

import planted_cliques as P
import twin_graphs as T
from clique_list_ref import check_list, clique_list_ref, lex_window, order_keys, planted_expected, sort_rows
from common import GOLDEN, check_rows, load_graph
from graphminer_amd import CliqueSolver, Graph, TCSolver, _lib, clique_list, clique_local, tc_list
from graphminer_amd._lib import dev_live_blocks
from graphminer_amd.rmat import csr_from_pairs
from list_windows import U64_MAX, clique_call, guarded_window, root_boundaries

pytestmark = pytest.mark.gpu
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42"]
RMAT10 = "rmat10_ef16_s42"
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def ref(name, k):
    r = clique_list_ref(load_graph(name), k)
    r.setflags(write=False)
    return r


def golden(name, k):
    return GOLDEN[name]["tc"] if k == 3 else GOLDEN[name][f"clique{k}"]


@functools.lru_cache(maxsize=None)
def constants():
    """the row lengths at which the listing kernels change path, read from the library"""
    out = {}
    for key, name in (("l2", "kcl_list_regs2_row"), ("l8", "kcl_list_regs8_row"), ("lds", "kcl_local_lds_row")):
        v = C.c_int64(0)
        _lib.check(_lib.load().gm_constant(name.encode(), C.byref(v)), "gm_constant")
        out[key] = int(v.value)
    out["big"] = 2048  # no constant of the listing: a row of more entries than any LDS stage of the library holds
    return out


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def raw_call(sym, k, first, cap, buf, la=None):
    """gm_clique_list itself: (status, total, n_written); buf a torch int32 tensor or None"""
    total, written = C.c_uint64(99), C.c_uint64(99)
    rc = _lib.load().gm_clique_list(sym.handle, k, C.byref(la) if la is not None else None, first, cap, buf.data_ptr() if buf is not None else None,
                                    C.byref(total), C.byref(written), None)
    return rc, int(total.value), int(written.value)


def windows(sym, k, size, start, count):
    """gm_clique_list in the windows [start, start + size), ... up to `count` rows: every call writes behind the one before it into one device
    buffer (pre-filled with the sentinel, with slack), which comes back once"""
    import torch

    buf = torch.full((k * count + 64,), SENTINEL, dtype=torch.int32, device=f"cuda:{sym.device}")
    lib, written = _lib.load(), C.c_uint64(0)
    for f in range(0, count, size):
        want = min(size, count - f)
        rc = lib.gm_clique_list(sym.handle, k, None, start + f, want, buf.data_ptr() + 4 * k * f, None, C.byref(written), None)
        assert (rc, int(written.value)) == (_lib.GM_OK, want), (f, rc, written.value)
    host = buf.cpu().numpy()
    assert bool((host[k * count:] == SENTINEL).all()), "nothing behind the last window"
    return host[:k * count].reshape(-1, k)


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs(dev, name):
    g = load_graph(name)
    with g.to_device(dev) as sym:
        for k in range(3, 9):
            rows, total, st = clique_list(sym, k, return_stats=True)
            check(f"{name} k={k} total", total, golden(name, k))
            check_rows(f"{name} k={k} rows in order", rows, ref(name, k))
            print(f"{name} k={k} kernel_ms {st.kernel_ms}", flush=True)
            assert st.kernel_ms > 0
        with sym.orient() as dag:
            check(f"{name} total against CliqueSolver", clique_list(sym, 4, cap=0)[1], CliqueSolver(dag, 4))
        rows3 = clique_list(sym, 3)[0]
        check_rows(f"{name} k=3 is tc_list's set", sort_rows(rows3), sort_rows(tc_list(sym)[1]))


@pytest.mark.parametrize("k", [3, 4])
def test_rmat10_in_order(dev, k):
    with load_graph(RMAT10).to_device(dev) as sym:
        rows, total = clique_list(sym, k)
        check(f"rmat10 k={k} total", total, golden(RMAT10, k))
        check_rows(f"rmat10 k={k} rows in order", rows, ref(RMAT10, k))


def test_rmat10_six_cliques_pass_the_checker(dev):
    g = load_graph(RMAT10)
    with g.to_device(dev) as sym:
        rows, total = clique_list(sym, 6)
    check("rmat10 k=6 total", total, 5707838)
    check("rmat10 k=6 golden", total, golden(RMAT10, 6))
    check("rmat10 k=6 rows", rows.shape, (total, 6))
    check_list(g, 6, rows, 0)  # (ascending cliques, strictly increasing in the order, as many as the golden count: the list)


def test_no_cliques_leaves_the_buffer_alone(dev):
    import torch

    check("cora has no 6-clique", golden("cora", 6), 0)
    buf = torch.full((600,), SENTINEL, dtype=torch.int32, device=f"cuda:{dev}")
    with load_graph("cora").to_device(dev) as sym:
        check("cora k=6", raw_call(sym, 6, 0, 100, buf), (_lib.GM_OK, 0, 0))
        check("buffer untouched", bool((buf.cpu().numpy() == SENTINEL).all()), True)
        rows, total = clique_list(sym, 6)
        check("mirror", (rows.shape, total), ((0, 6), 0))


def test_count_only_and_guard_words(dev):
    import torch

    k = 4
    T_ = golden(RMAT10, k)
    with load_graph(RMAT10).to_device(dev) as sym:
        check("count only", raw_call(sym, k, 0, 12345, None), (_lib.GM_OK, T_, 0))
        full = clique_list(sym, k)[0]
        call = clique_call(sym, k)
        # (guarded_window asserts: both pads all sentinel, exactly k n_written ints changed, nothing behind row n_written)
        rc, total, n, rows = guarded_window(call, k, 0, T_ - 5, rows=T_ + 16, sentinel=SENTINEL)
        check("cap = T - 5", (rc, total, n), (_lib.GM_OK, T_, T_ - 5))
        check_rows("the first T - 5 rows", rows, full[:T_ - 5])
        rc, total, n, rows = guarded_window(call, k, 1000, 77, sentinel=SENTINEL)
        check("a window in the middle", (rc, total, n), (_lib.GM_OK, T_, 77))
        check_rows("rows 1000 .. 1076", rows, full[1000:1077])
        for first in (T_, T_ + 1, 2**40):
            rc, total, n, rows = guarded_window(call, k, first, 10, sentinel=SENTINEL)
            check(f"first = {first}", (rc, total, n, rows.shape), (_lib.GM_OK, T_, 0, (0, k)))
        rc, total, n, rows = guarded_window(call, k, 5, 0, rows=10, sentinel=SENTINEL)
        check("cap = 0", (rc, total, n, rows.shape), (_lib.GM_OK, T_, 0, (0, k)))
        rc, total, n, rows = guarded_window(call, k, T_ - 5, U64_MAX, rows=10, sentinel=SENTINEL)
        check("first = T - 5, cap = 2^64 - 1", (rc, total, n), (_lib.GM_OK, T_, 5))
        check_rows("the last five rows", rows, full[T_ - 5:])
        rc, total, n, rows = guarded_window(call, k, 0, U64_MAX, rows=T_, sentinel=SENTINEL)
        check("first = 0, cap = 2^64 - 1", (rc, total, n), (_lib.GM_OK, T_, T_))
        check_rows("the whole list", rows, full)
        buf = torch.full((64,), SENTINEL, dtype=torch.int32, device=f"cuda:{dev}")
        check("first = 2^64 - 1, cap = 2^64 - 1", raw_call(sym, k, U64_MAX, U64_MAX, buf), (_lib.GM_OK, T_, 0))
        check("nothing written", bool((buf.cpu().numpy() == SENTINEL).all()), True)


@pytest.mark.parametrize("name,k,other", [("cora", 4, 3), (RMAT10, 5, 4)])
def test_windows_tile_the_list(dev, name, k, other):
    """small windows tile a stretch that starts in the middle of the list (every root / entry / pair boundary inside it falls inside some
    window or between two), windows of 1000 tile the whole list"""
    with load_graph(name).to_device(dev) as sym:
        full, total = clique_list(sym, k)
        check(f"{name} k={k} total", total, golden(name, k))
        for size, count in ((1, 200), (7, 2100), (64, 64 * 150), (67, 67 * 150), (1000, total)):
            count = min(count, total)
            start = 0 if count == total else (total - count) // 2 + 3
            check_rows(f"{name} k={k} windows of {size} from {start}", windows(sym, k, size, start, count), full[start:start + count])
        parts = [clique_list(sym, k, first=f, cap=250000)[0] for f in range(0, total, 250000)]
        check_rows(f"{name} k={k} windows through the mirror", np.concatenate(parts), full)
        rows_other, total_other = clique_list(sym, other)
        check(f"{name} k={other} on the same handle", total_other, golden(name, other))
        check_rows(f"{name} k={other} rows", rows_other, ref(name, other))
        again, total_again = clique_list(sym, k)
        check(f"{name} k={k} again total", total_again, total)
        check_rows(f"{name} k={k} again, the same sequence", again, full)


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("m", ["k-1", 63, 64, 65])
def test_complete_graphs_whole(dev, k, m):
    """K_n with n - 1 = m entries in the longest row: the list is the lexicographic list of k-subsets"""
    n = (k - 1 if m == "k-1" else m) + 1
    want = np.array(list(itertools.combinations(range(n), k)), dtype=np.int32).reshape(-1, k)
    with T.graph("complete", (n,)).to_device(dev) as sym:
        rows, total = clique_list(sym, k)
        check(f"K_{n} k={k} total", total, comb(n, k))
        check_rows(f"K_{n} k={k} rows", rows, want)
        count = min(total, 2000)
        check_rows(f"K_{n} k={k} windows of 50", windows(sym, k, 50, 0, count), rows[:count])


@pytest.mark.parametrize("k", [5, 6])
@pytest.mark.parametrize("n", [130, 200])
def test_complete_graphs_window_by_unranking(dev, n, k):
    first = comb(n, k) // 2
    want = lex_window(n, k, first, 4096)
    with T.graph("complete", (n,)).to_device(dev) as sym:
        rows, total = clique_list(sym, k, first=first, cap=4096)
        check(f"K_{n} k={k} total", total, comb(n, k))
        check_rows(f"K_{n} k={k} rows {first} ..", rows, want)


def test_slots_past_2_32(dev):
    n, k = 256, 5
    T_ = comb(n, k)
    check("C(256, 5)", T_, 8809549056)
    with T.graph("complete", (n,)).to_device(dev) as sym:
        check("count only", raw_call(sym, k, 0, 0, None), (_lib.GM_OK, T_, 0))
        for first in (2**32 - 5, 2**32 - 10, 2**32):
            rows, total = clique_list(sym, k, first=first, cap=10)
            check(f"window at {first} total", total, T_)
            check_rows(f"window at {first}", rows, lex_window(n, k, first, 10))
        rows, total = clique_list(sym, k, first=T_ - 10, cap=10)
        check_rows("the last ten", rows, lex_window(n, k, T_ - 10, 10))
        rows, total = clique_list(sym, k, first=T_ - 4, cap=10)
        check("four are left", rows.shape, (4, k))
        check_rows("the last four", rows, lex_window(n, k, T_ - 4, 10))


# ---- path boundaries: planted graphs ----------------------------------------------------------------------------------------------------
def _cells():
    out = []
    for base, off in (("l2", 0), ("l2", 1), ("l8", 0), ("l8", 1), ("lds", 0), ("lds", 1), ("big", 1)):
        # (big + 1 at k = 5: a stride of 65 words, the second trip of KclListWalk's loop over 64 words at a time)
        ks = (3, 4, 5) if (base, off) in (("lds", 1), ("big", 1)) else (3, 4)
        out.append(P.Cell(f"{base}{off:+d}", "L", base, off, ks, True, P.LOW))
    # k = 6, 7, 8 from a long row of every class: blocks of 13 .. 18 vertices at p = 0.9 hold 8-cliques.  The pair values come from
    # kcl_list_pair_small<M, 2 / 8 / 16> and kcl_list_pair_any<M> at M = 3, 4, 5, the walk is KclListWalk<M, K> at M = 3, 4, 5 over 3, 9, 16
    # and 17 words
    for base, off in (("l2", 1), ("l8", 0), ("l8", 1), ("lds", 0), ("lds", 1)):
        out.append(P.Cell(f"{base}{off:+d}-high", "L", base, off, (6, 7, 8), True, P.HIGH))
    return out


CELLS = _cells()
CELL = {c.name: c for c in CELLS}


def planted_cell(cell):
    consts = constants()
    p = P.cell_graph(cell, tuple(sorted(consts.items())))
    d = consts[cell.base] + cell.off
    check(f"{cell.name}: the DAG's longest row is the root's", (p.max_row, max(p.root_rows())), (d, d))
    order = ["l2", "l8", "lds", "big"]
    for name in order:  # the row lies where the cell says: beyond every constant below its base (and the base itself at + 1), within the others
        beyond = order.index(name) < order.index(cell.base) or (name == cell.base and cell.off > 0)
        check(f"{cell.name}: row of {d} beyond {name} = {consts[name]}", d > consts[name], beyond)
    return p


@pytest.mark.parametrize("cell", CELLS, ids=[c.name for c in CELLS])
def test_planted_rows_on_both_sides_of_every_constant(dev, cell):
    p = planted_cell(cell)
    for k in cell.ks:
        cond = p.conditions(k)
        want = planted_expected(p, k)
        print(f"{cell.name} k={k}: {cond}, expected rows {len(want)}", flush=True)
        assert cond["blocks_with_clique"] >= 0.9 and len(want) >= 1000 and len(want) == p.expected(k)[2]
    with p.graph.to_device(dev) as sym:
        for k in cell.ks:
            rows, total = clique_list(sym, k)
            want = planted_expected(p, k)
            check(f"{cell.name} k={k} total", total, len(want))
            check_rows(f"{cell.name} k={k} the expected set", sort_rows(rows), want)
            check_list(p.graph, k, rows, 0)
            mid = total // 2
            rc, total2, n, part = guarded_window(clique_call(sym, k), k, mid, 300, sentinel=SENTINEL)
            check(f"{cell.name} k={k} a window in the middle", (rc, total2, n), (_lib.GM_OK, total, min(300, total - mid)))
            check_rows(f"{cell.name} k={k} the window's rows", part, rows[mid:mid + 300])


def mixed_graph():
    """roots within the 2-register rows, within the LDS matrix and two beyond it (scratch slots) in one graph"""
    c = constants()
    rows_wanted = (c["l2"] - 4, c["l8"] + 44, c["lds"] + 1, 2 * c["lds"] + 76)
    consts = {"split": rows_wanted[0] + 28, "regs8": rows_wanted[1] - 44, "lds": c["lds"]}
    p = P.cell_graph(P.Cell("mixed", "D", "lds", 0, (4, 5), True, P.LOW, special="mixed"), tuple(sorted(consts.items())))
    check("the roots' rows", tuple(sorted(p.root_rows())), rows_wanted)
    check("the longest row", p.max_row, rows_wanted[3])
    assert rows_wanted[0] <= c["l2"] < rows_wanted[1] <= c["lds"] < rows_wanted[2]
    return p


def test_planted_three_kinds_of_root_in_one_graph(dev):
    """roots within the 2-register rows, within the LDS matrix and two beyond it (scratch slots), one call"""
    p = mixed_graph()
    with p.graph.to_device(dev) as sym:
        for k in (4, 5):
            cond, want = p.conditions(k), planted_expected(p, k)
            print(f"mixed k={k}: {cond}, expected rows {len(want)}", flush=True)
            assert cond["blocks_with_clique"] >= 0.9 and len(want) >= 1000
            rows, total = clique_list(sym, k)
            check(f"mixed k={k} total", total, len(want))
            check_rows(f"mixed k={k} the expected set", sort_rows(rows), want)
            check_list(p.graph, k, rows, 0)
            check_rows(f"mixed k={k} windows of 997", np.concatenate([clique_list(sym, k, first=f, cap=997)[0] for f in range(0, total, 997)]), rows)


# ---- windows at root, entry and pair boundaries --------------------------------------------------------------------------------------------
EDGE_CASES = [("l2+1", 4), ("l2+1-high", 6), ("l8+1", 5), ("l8+1-high", 8), ("lds+1", 4), ("lds+1", 5), ("lds+1-high", 6), ("lds+1-high", 8),
              ("mixed", 5)]
EDGE_STARTS, EDGE_CAPS = (-1, 0), (1, 63, 64, 65, 129)


@pytest.mark.parametrize("name,k", EDGE_CASES, ids=[f"{n}-k{k}" for n, k in EDGE_CASES])
def test_windows_at_root_entry_and_pair_boundaries(dev, name, k):
    """a window that starts or ends exactly on the first slot of a long root, of one of its entries or of one of its pairs, a slot before
    it, and on either side of a flush of 64 rows inside a pair: the root filter of the WIDE fill, the root and entry skips of the LDS
    fill, the pair filter with a carried base and a seek, in every register class.  The reference is the one-call list once the expected
    set and the checker have pinned it; every window has guard words on both sides."""
    p = mixed_graph() if name == "mixed" else planted_cell(CELL[name])
    want = planted_expected(p, k)
    cond = p.conditions(k)
    print(f"{name} k={k}: {cond}, expected rows {len(want)}", flush=True)
    assert cond["blocks_with_clique"] >= 0.9 and len(want) >= 1000 and len(want) == p.expected(k)[2]
    roots = sorted((int(p.row_len[p.i_id[x]]), int(p.i_id[x])) for x, m in enumerate(p.members) if not m.top)
    targets = [roots[-1]] + ([roots[-2]] if name == "mixed" else [])  # the longest root; mixed: also the shorter WIDE root
    assert name != "mixed" or roots[-2][0] > constants()["lds"]
    with p.graph.to_device(dev) as sym:
        rows, total = clique_list(sym, k)
        check(f"{name} k={k} total", total, len(want))
        check_rows(f"{name} k={k} the expected set", sort_rows(rows), want)
        check_list(p.graph, k, rows, 0)
        rows.setflags(write=False)
        keys = order_keys(p.graph, rows)
        call = clique_call(sym, k)
        calls = 0
        for d, root in targets:
            bounds, exact, info = root_boundaries(p.graph, keys, root)
            print(f"{name} k={k} root {root} (row of {d}): {info}\n  boundaries {bounds}\n  exact {exact}", flush=True)
            # (two windows of the largest cap fit inside the root: a window at one of its inner boundaries stays inside it)
            assert info["row"] == d and info["rows"] >= 2 * max(EDGE_CAPS) and info["entries"] >= 3 and info["pairs of the fattest entry"] >= 3
            if d >= 128:  # (in a row of 65 entries the second chunk holds the last position alone, and nothing lies above it: no such pair)
                assert info["cross pairs behind a carried base"] >= 1 and info["cross pair"][1] // 64 > info["cross pair"][0] // 64
                assert info["cross pair"][2] >= 1, "an earlier pair of the same entry holds rows"
            else:
                assert info["cross pairs"] == 0
            for label, b in bounds:
                for first in sorted({min(max(b + o, 0), total - 1) for o in EDGE_STARTS}):
                    for cap in EDGE_CAPS:
                        rc, total2, n, part = guarded_window(call, k, first, cap, sentinel=SENTINEL)
                        calls += 1
                        assert (rc, total2, n) == (_lib.GM_OK, total, min(cap, total - first)), (label, first, cap, rc, total2, n)
                        if not np.array_equal(part, rows[first:first + cap]):
                            check_rows(f"{name} k={k} {label}: first={first} cap={cap}", part, rows[first:first + cap])
            for label, first, cap in exact:
                rc, total2, n, part = guarded_window(call, k, first, cap, sentinel=SENTINEL)
                calls += 1
                check(f"{name} k={k} {label}: first={first} cap={cap}", (rc, total2, n), (_lib.GM_OK, total, cap))
                check_rows(f"{name} k={k} {label}: rows", part, rows[first:first + cap])
        print(f"{name} k={k}: {calls} windows, every one the list's slice", flush=True)


# ---- the caller's numbering -------------------------------------------------------------------------------------------------------------
def permuted_rmat10():
    g = load_graph(RMAT10)
    perm = np.random.default_rng(5).permutation(g.V()).astype(np.uint64)
    src = np.repeat(np.arange(g.V()), np.diff(g.row_ptr))
    return csr_from_pairs(g.V(), perm[src], perm[g.col_idx])


@pytest.mark.parametrize("which", ["rmat10 permuted", "multipartite (4, 12) at 517 of 1000"])
def test_the_callers_numbering(dev, which):
    g = permuted_rmat10() if which.startswith("rmat10") else T.graph("multipartite", (4, 12), nv=1000, offset=517)
    with g.to_device(dev) as sym:
        for k in (3, 4):
            want = clique_list_ref(g, k)
            check(f"{which} k={k} expected rows", len(want), golden(RMAT10, k) if which.startswith("rmat10") else (4 * 12**3 if k == 3 else 12**4))
            rows, total = clique_list(sym, k)
            check(f"{which} k={k} total", total, len(want))
            check_rows(f"{which} k={k} rows in order", rows, want)


# ---- the other solvers of the handle -----------------------------------------------------------------------------------------------------
def test_neighbours_on_the_handle(dev):
    g = load_graph(RMAT10)
    want4, want5 = ref(RMAT10, 4), clique_list_ref(g, 5)
    with g.to_device(dev) as fresh:
        want_tri = tc_list(fresh)
    with g.to_device(dev) as fresh:
        want_local = clique_local(fresh, 4)
    before = dev_live_blocks()

    def same_list(label, sym, k=4):
        rows, total = clique_list(sym, k)
        check(label + " total", total, golden(RMAT10, k))
        check_rows(label + " sequence", rows, want4 if k == 4 else want5)

    def same_tri(label, sym):
        total, tri = tc_list(sym)
        check(label + " total", total, want_tri[0])
        check_rows(label + " sequence", tri, want_tri[1])

    def same_local(label, sym):
        total, kv, ke = clique_local(sym, 4)
        check(label, (total, bool(np.array_equal(kv, want_local[1])), bool(np.array_equal(ke, want_local[2]))), (want_local[0], True, True))

    def same_counts(label, sym):
        with sym.orient() as dag:
            check(label, (TCSolver(dag), CliqueSolver(dag, 4), CliqueSolver(dag, 5)), (golden(RMAT10, 3), golden(RMAT10, 4), golden(RMAT10, 5)))

    with g.to_device(dev) as sym:  # the list first, then each neighbour, the list after each
        same_list("list first", sym)
        for label, other in (("tc_list", same_tri), ("clique_local", same_local), ("TCSolver / CliqueSolver", same_counts)):
            other(f"{label} after the list", sym)
            same_list(f"list after {label}", sym)
        same_list("k = 5 after all of them", sym, 5)
    for label, other in (("tc_list", same_tri), ("clique_local", same_local), ("TCSolver / CliqueSolver", same_counts)):
        with g.to_device(dev) as sym:  # the neighbour first on a fresh handle
            other(f"{label} first", sym)
            same_list(f"list after a first {label}", sym)
            other(f"{label} again", sym)
    check("device blocks are back after the handles are freed", dev_live_blocks(), before)


def test_refusals_and_the_empty_graph(dev, devopt):
    import torch

    g = load_graph("citeseer")
    buf = torch.zeros(64, dtype=torch.int32, device=f"cuda:{dev}")
    check("a null handle", _lib.load().gm_clique_list(None, 4, None, 0, 4, buf.data_ptr(), None, None, None), _lib.GM_ERR_INVALID)
    with g.to_device(dev) as sym:
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("world = 2", raw_call(sym, 4, 0, 4, buf, la), (_lib.GM_ERR_UNSUPPORTED, 0, 0))
        la = _lib.gm_launch()
        counts = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = counts.data_ptr()
        check("d_counts", raw_call(sym, 4, 0, 4, buf, la), (_lib.GM_ERR_UNSUPPORTED, 0, 0))
        for k in (-1, 0, 2, 13, 100):
            check(f"k = {k}", raw_call(sym, k, 0, 4, buf), (_lib.GM_ERR_INVALID, 0, 0))
        for k in (9, 10, 12):
            check(f"k = {k}", raw_call(sym, k, 0, 4, buf), (_lib.GM_ERR_UNSUPPORTED, 0, 0))
        check("nothing was written", bool((buf.cpu().numpy() == 0).all()), True)
        check("the handle still lists", clique_list(sym, 4)[1], 255)
    devopt("GM_BIG_NE", "1")  # a handle of "2^31 entries or more" (the developer option gives a small graph such a handle)
    big = g.to_device(dev)
    devopt("GM_BIG_NE", None)
    with big:
        check("a big handle", raw_call(big, 4, 0, 4, buf), (_lib.GM_ERR_TOO_LARGE, 0, 0))
    rev = g.col_idx.copy()
    for v in range(g.V()):
        a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
        rev[a:b] = rev[a:b][::-1]
    with Graph(row_ptr=g.row_ptr.copy(), col_idx=rev, name="citeseer_descending").to_device(dev) as sym:
        check("unsorted rows", raw_call(sym, 4, 0, 4, buf), (_lib.GM_ERR_INVALID, 0, 0))
        assert b"ascending" in _lib.load().gm_last_error()
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        check("no edges", raw_call(sym, 4, 0, 4, buf), (_lib.GM_OK, 0, 0))
        rows, total = clique_list(sym, 5)
        check("no edges, mirror", (total, rows.shape), (0, (0, 5)))
