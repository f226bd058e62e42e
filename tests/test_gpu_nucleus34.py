"""Triangle nuclei on the GPU (gm_tri_clique4_local / gm_nucleus34 / gm_nucleus34_decompose, csrc/gm_nucleus34.hip) against the plain Python
rounds of tests/nucleus34_ref.py and against closed forms.  The reference keys its results by the sorted triple; the wanted arrays are
built through the rows of tc_list, so every comparison also pins "a triangle's id is its row in gm_tc_list's listing".  On the five small
graphs, on the shapes where a concurrent round goes wrong (a whole clique in one frontier, a level jump, tens of thousands of decrements
on one counter) and with rows on both sides of the length at which a triangle goes from a group of lanes to the whole wave.  Every value
is printed before it is asserted."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

import nucleus34_ref as R
from common import gm_constant, load_graph
from graphminer_amd import (CliqueSolver, Graph, TCSolver, _lib, clique_local, clique_truss_decompose, nucleus34, nucleus34_decompose, tc_list,
                            tri_clique4_local)
from graphminer_amd._lib import dev_live_blocks
from graphminer_amd.rmat import csr_from_pairs

pytestmark = pytest.mark.gpu
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
TABLE = {"citeseer": (1166, 255, 3, 11), "cora": (1630, 220, 2, 8), "rmat6_ef4_s1": (220, 167, 4, 14), "rmat8_ef8_s42": (3835, 7296, 8, 37),
         "rmat10_ef16_s42": (76537, 421914, 20, 170)}  # T, 4-cliques, c_max, rounds
REMOVED = R.REMOVED


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_arrays(label, got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got != want) if got.shape == want.shape else np.zeros(0, np.int64)
    print(f"{label}: {want.shape} values, {bad.size} differ, first at {bad[:5].tolist()}: got {got[bad[:5]].tolist()} "
          f"want {want[bad[:5]].tolist()}", flush=True)
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, label


def pairs_graph(nv, pairs):
    s, d = np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint64)
    return csr_from_pairs(nv, s, d)


def complete_pairs(ids):
    return [(ids[i], ids[j]) for i in range(len(ids)) for j in range(i + 1, len(ids))]


def gnp_pairs(ids, p, seed):
    rng = np.random.default_rng(seed)
    return [e for e in complete_pairs(ids) if rng.random() < p]


def book(m):
    """the triangle {0, 1, 2} and m pairwise non-adjacent pages, each joined to all three corners"""
    pages = np.arange(3, 3 + m, dtype=np.uint64)
    s = np.concatenate([np.array([0, 0, 1], dtype=np.uint64)] + [np.full(m, c, dtype=np.uint64) for c in (0, 1, 2)])
    d = np.concatenate([np.array([1, 2, 2], dtype=np.uint64), pages, pages, pages])
    return csr_from_pairs(3 + m, s, d)


@functools.lru_cache(maxsize=None)
def prepared(name):
    return R.prepare(load_graph(name))


@functools.lru_cache(maxsize=None)
def ref_decompose(name):
    return R.decompose(prepared(name))


def rows_of(sym):
    total, rows = tc_list(sym)
    assert rows.shape == (total, 3)
    return rows


def check_decompose(label, sym, want, rows=None):
    """want: R.Decomposition.  Returns (theta, round, c_max, rounds, rows)"""
    rows = rows_of(sym) if rows is None else rows
    theta, rnd, c_max, rounds, st = nucleus34_decompose(sym, return_stats=True)
    check(f"{label} T", theta.shape[0], len(want.theta))
    check_arrays(f"{label} theta", theta, R.ordered(rows, want.theta))
    check_arrays(f"{label} round per triangle", rnd, R.ordered(rows, want.round))
    check(f"{label} (c_max, rounds)", (c_max, rounds), (want.c_max, want.rounds))
    check(f"{label} c_max against theta", c_max, int(theta.max()) if theta.size else 0)
    assert rounds >= 1 and st.tasks == rows.shape[0]
    return theta, rnd, c_max, rounds, rows


def check_nucleus(label, sym, c, want, rows=None):
    """want: R.Nucleus"""
    rows = rows_of(sym) if rows is None else rows
    ntri, ncl, cnt, rounds, st = nucleus34(sym, c, return_stats=True)
    check_arrays(f"{label} c={c} per triangle", cnt, R.ordered(rows, want.cnt))
    check(f"{label} c={c} (triangles, cliques, rounds)", (ntri, ncl, rounds), (want.triangles, want.cliques, want.rounds))
    inside = cnt != REMOVED
    check(f"{label} c={c} 4 x cliques against the surviving counts", 4 * ncl, sum(int(x) for x in cnt[inside]))
    check(f"{label} c={c} triangles against the counts", ntri, int(inside.sum()))
    assert rounds >= 1 and st.tasks == rows.shape[0]
    return cnt


# ---- 1. the decomposition on the five small graphs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_decompose_small_graphs(dev, name):
    want = ref_decompose(name)
    check(f"{name} the reference (T, 4-cliques, c_max, rounds)", (len(want.theta), want.destroyed, want.c_max, want.rounds), TABLE[name])
    with load_graph(name).to_device(dev) as sym:
        check_decompose(name, sym, want)


# ---- 2. the local counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_local_counts_small_graphs(dev, name):
    g = load_graph(name)
    p = prepared(name)
    want = {t: len(p.on[i]) for i, t in enumerate(p.tris)}
    with g.to_device(dev) as sym:
        rows = rows_of(sym)
        total, k4, st = tri_clique4_local(sym, return_stats=True)
        check(f"{name} (T, total)", (k4.shape[0], total), (TABLE[name][0], TABLE[name][1]))
        check_arrays(f"{name} K4(t)", k4, R.ordered(rows, want))
        assert st.tasks == rows.shape[0]
        with sym.orient() as dag:
            check(f"{name} total against CliqueSolver(dag, 4)", total, CliqueSolver(dag, 4))
        _, _, ent = clique_local(sym, 4, vertex=False)
    # every 4-clique on an edge has two triangles on it: the sum of K4(t) over the triangles of an entry's edge = 2 x the entry's count
    nv = g.V()
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(g.row_ptr))
    keys = src * nv + np.asarray(g.col_idx).astype(np.int64)  # ascending: the rows are
    sums = np.zeros(keys.shape[0], dtype=np.uint64)
    r = rows.astype(np.int64)
    for x, y in ((0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)):
        at = np.searchsorted(keys, r[:, x] * nv + r[:, y])
        assert np.array_equal(keys[at], r[:, x] * nv + r[:, y])
        np.add.at(sums, at, k4.astype(np.uint64))
    check_arrays(f"{name} per entry: the sum over its triangles against 2 x gm_clique_local(k = 4)", sums, 2 * ent)


# ---- 3. a fixed c ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [(n, w) for n in SMALL for w in range(5)])
def test_fixed_c_small_graphs(dev, name, which):
    d = ref_decompose(name)
    c = (0, 1, d.c_max // 2, d.c_max, d.c_max + 1)[which]
    with load_graph(name).to_device(dev) as sym:
        rows = rows_of(sym)
        cnt = check_nucleus(name, sym, c, R.nucleus(prepared(name), c), rows)
        check_arrays(f"{name} c={c} the set is the triangles of theta >= c", cnt != REMOVED, R.ordered(rows, d.theta) >= c)
        if which == 0:
            check(f"{name} c = 0 removes nothing", int((cnt != REMOVED).sum()), rows.shape[0])
        if which == 4:
            check(f"{name} the (c_max + 1)-nucleus set is empty", int((cnt != REMOVED).sum()), 0)


# ---- 4. a whole clique in one frontier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 8, 64, 65, 70])
def test_complete_graph(dev, n):
    """K_n: every 4-clique has its four triangles in one frontier, all degrees tie so the orientation falls to the ids, and segments of
    every length up to n - 2 are searched at every position.  Rows of n - 1 entries: 63 is the longest a group of lanes takes, 64 the
    shortest the whole wave takes, 69 goes past one 64-lane tile"""
    check("the length from which the whole wave takes a row", gm_constant("nuc_whole_wave"), 64)
    T, each = comb(n, 3), n - 3
    with pairs_graph(n, complete_pairs(list(range(n)))).to_device(dev) as sym:
        total, k4 = tri_clique4_local(sym)
        check(f"K_{n} (T, 4-cliques, the counts)", (k4.shape[0], total, np.unique(k4).tolist()), (T, comb(n, 4), [each]))
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)  # (the call checks that it destroyed C(n, 4))
        check(f"K_{n} (theta, round, c_max, rounds)", (np.unique(theta).tolist(), np.unique(rnd).tolist(), c_max, rounds), ([each], [1], each, 2))
        ntri, ncl, cnt, rounds = nucleus34(sym, each)
        check(f"K_{n} c = {each}", (ntri, ncl, np.unique(cnt).tolist(), rounds), (T, comb(n, 4), [each], 1))
        ntri, ncl, cnt, rounds = nucleus34(sym, each + 1)
        check(f"K_{n} c = {each + 1}", (ntri, ncl, np.unique(cnt).tolist(), rounds), (0, 0, [REMOVED], 2))


# ---- 5. a level jump -----------------------------------------------------------------------------------------------------------------------------
def test_two_cliques_sharing_a_triangle(dev):
    """K_6 on {0 .. 5} and K_9 on {3 .. 11} share the triangle {3, 4, 5}: it gets theta 6, the rest of K_6 gets 3, the level jumps"""
    g = pairs_graph(12, complete_pairs(list(range(6))) + complete_pairs(list(range(3, 12))))
    want = R.decompose(g)
    inside9 = {t for t in want.theta if t[0] >= 3}
    check("the reference: theta", ({want.theta[t] for t in inside9}, {want.theta[t] for t in want.theta if t not in inside9}, want.c_max), ({6}, {3}, 6))
    with g.to_device(dev) as sym:
        theta, _, _, _, rows = check_decompose("K_6 + K_9", sym, want)
        shared = int(np.flatnonzero((rows == (3, 4, 5)).all(axis=1))[0])
        check("the shared triangle", int(theta[shared]), 6)
        for c in (3, 4, 6, 7):
            check_nucleus("K_6 + K_9", sym, c, R.nucleus(g, c), rows)


# ---- 6. many decrements on one counter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [35000, 70000])
def test_book(dev, m):
    """in round 1 every page triangle leaves and the centre's counter takes m decrements; the centre leaves in round 2.  The three hub rows
    hold m + 2 entries.  By closed form"""
    with book(m).to_device(dev) as sym:
        rows = rows_of(sym)
        centre = int(np.flatnonzero((rows == (0, 1, 2)).all(axis=1))[0])
        total, k4 = tri_clique4_local(sym)
        check(f"book {m} (T, 4-cliques, the centre's count, the others)", (k4.shape[0], total, int(k4[centre]), np.unique(np.delete(k4, centre)).tolist()),
              (3 * m + 1, m, m, [1]))
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)
        check(f"book {m} (theta, c_max, rounds)", (np.unique(theta).tolist(), c_max, rounds), ([1], 1, 3))
        check(f"book {m} rounds per triangle: the centre in round 2", (int(rnd[centre]), int((rnd == 2).sum()), int((rnd == 1).sum())), (2, 1, 3 * m))
        ntri, ncl, cnt, rounds = nucleus34(sym, 1)
        check(f"book {m} c = 1", (ntri, ncl, int(cnt[centre]), rounds), (3 * m + 1, m, m, 1))
        ntri, ncl, cnt, rounds = nucleus34(sym, 2)
        check(f"book {m} c = 2", (ntri, ncl, np.unique(cnt).tolist(), rounds), (0, 0, [REMOVED], 3))


# ---- 7. a hub triangle whose common neighbours lie on both sides of the tile length -------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_hub_triangle_over_a_sparse_graph(dev, m):
    """three hubs joined to each other and to m pages, a seeded G(m, 0.2) among the pages: the hub triangle has m common neighbours, the
    counts differ from triangle to triangle"""
    hubs = [m, m + 1, m + 2]
    g = pairs_graph(m + 3, complete_pairs(hubs) + [(h, p) for h in hubs for p in range(m)] + gnp_pairs(list(range(m)), 0.2, m))
    want = R.decompose(g)
    check(f"m={m}: the hub triangle's count, different counts", (R.k4(g)[tuple(hubs)], len(set(R.k4(g).values())) >= 3), (m, True))
    with g.to_device(dev) as sym:
        rows = rows_of(sym)
        _, k4 = tri_clique4_local(sym)
        check_arrays(f"m={m} K4(t)", k4, R.ordered(rows, R.k4(g)))
        check_decompose(f"hub triangle m={m}", sym, want, rows)
        for c in (want.c_max // 2, want.c_max):
            check_nucleus(f"hub triangle m={m}", sym, c, R.nucleus(g, c), rows)


# ---- 8. dense random graphs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(96, 0.5), (200, 0.3)])
def test_dense_random_graphs(dev, n, p):
    g = pairs_graph(n, gnp_pairs(list(range(n)), p, n))
    state = R.prepare(g)
    want = R.decompose(state)
    print(f"G({n}, {p}): {len(want.theta)} triangles, {want.destroyed} cliques, c_max {want.c_max}, rounds {want.rounds}", flush=True)
    with g.to_device(dev) as sym:
        rows = rows_of(sym)
        check_decompose(f"G({n}, {p})", sym, want, rows)
        c = max(1, want.c_max // 2)
        check_nucleus(f"G({n}, {p})", sym, c, R.nucleus(state, c), rows)


# ---- 9. the contract -------------------------------------------------------------------------------------------------------------------------------
def raw_local(sym, n_tri, la=None, buf=None):
    total = C.c_uint64(5)
    rc = _lib.load().gm_tri_clique4_local(sym.handle if sym is not None else None, C.byref(la) if la is not None else None, n_tri,
                                          buf.data_ptr() if buf is not None else None, C.byref(total), None)
    return rc, int(total.value)


def raw_nucleus(sym, c, n_tri, la=None, buf=None):
    n, m, rounds = C.c_uint64(5), C.c_uint64(5), C.c_int32(5)
    rc = _lib.load().gm_nucleus34(sym.handle if sym is not None else None, c, C.byref(la) if la is not None else None, n_tri,
                                  buf.data_ptr() if buf is not None else None, C.byref(n), C.byref(m), C.byref(rounds), None)
    return rc, int(n.value), int(m.value), int(rounds.value)


def raw_decompose(sym, n_tri, la=None, theta=None, rnd=None):
    cmax, rounds = C.c_uint32(5), C.c_int32(5)
    rc = _lib.load().gm_nucleus34_decompose(sym.handle if sym is not None else None, C.byref(la) if la is not None else None, n_tri,
                                            theta.data_ptr() if theta is not None else None, rnd.data_ptr() if rnd is not None else None,
                                            C.byref(cmax), C.byref(rounds), None)
    return rc, int(cmax.value), int(rounds.value)


def test_refusals(dev):
    import torch

    g = load_graph("citeseer")
    T = TABLE["citeseer"][0]
    buf = torch.zeros(T + 8, dtype=torch.int32, device=f"cuda:{dev}")
    check("local, a null handle", raw_local(None, T, buf=buf)[0], _lib.GM_ERR_INVALID)
    check("nucleus, a null handle", raw_nucleus(None, 1, T, buf=buf)[0], _lib.GM_ERR_INVALID)
    check("decompose, a null handle", raw_decompose(None, T, theta=buf)[0], _lib.GM_ERR_INVALID)
    with g.to_device(dev) as sym:
        for n_tri in (0, T - 1, T + 1):
            check(f"local n_tri = {n_tri}", raw_local(sym, n_tri, buf=buf)[0], _lib.GM_ERR_INVALID)
            check(f"nucleus n_tri = {n_tri}", raw_nucleus(sym, 1, n_tri, buf=buf)[0], _lib.GM_ERR_INVALID)
            check(f"decompose n_tri = {n_tri}", raw_decompose(sym, n_tri, theta=buf)[0], _lib.GM_ERR_INVALID)
        assert b"triangles" in _lib.load().gm_last_error()
        check("decompose without a theta array", raw_decompose(sym, T)[0], _lib.GM_ERR_INVALID)
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("local world = 2", raw_local(sym, T, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("nucleus world = 2", raw_nucleus(sym, 1, T, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose world = 2", raw_decompose(sym, T, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        counts = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = counts.data_ptr()
        check("local d_counts", raw_local(sym, T, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("nucleus d_counts", raw_nucleus(sym, 1, T, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        check("decompose d_counts", raw_decompose(sym, T, la, buf)[0], _lib.GM_ERR_UNSUPPORTED)
        with sym.orient() as dag:
            check("local, an oriented copy", raw_local(dag, T, buf=buf)[0], _lib.GM_ERR_INVALID)
            check("nucleus, an oriented copy", raw_nucleus(dag, 1, T, buf=buf)[0], _lib.GM_ERR_INVALID)
            check("decompose, an oriented copy", raw_decompose(dag, T, theta=buf)[0], _lib.GM_ERR_INVALID)
        check("nothing was written", bool((buf.cpu().numpy() == 0).all()), True)
        # the arrays may be left out: the numbers alone
        d = ref_decompose("citeseer")
        q = R.nucleus(prepared("citeseer"), 2)
        check("local without an array", raw_local(sym, T), (_lib.GM_OK, TABLE["citeseer"][1]))
        check("nucleus without an array", raw_nucleus(sym, 2, T), (_lib.GM_OK, q.triangles, q.cliques, q.rounds))
        check("decompose without a round array", raw_decompose(sym, T, theta=buf), (_lib.GM_OK, d.c_max, d.rounds))
        check_arrays("... its theta", buf.cpu().numpy().view(np.uint32)[:T], R.ordered(rows_of(sym), d.theta))
        check("... and nothing behind it", bool((buf.cpu().numpy()[T:] == 0).all()), True)
    rev = g.col_idx.copy()
    for v in range(g.V()):
        a, b = int(g.row_ptr[v]), int(g.row_ptr[v + 1])
        rev[a:b] = rev[a:b][::-1]
    with Graph(row_ptr=g.row_ptr.copy(), col_idx=rev, name="citeseer_descending").to_device(dev) as sym:
        check("decompose, unsorted rows", raw_decompose(sym, T, theta=buf)[0], _lib.GM_ERR_INVALID)
        assert b"ascending" in _lib.load().gm_last_error()


def test_graphs_without_triangles(dev):
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)
        check("no edges", (theta.tolist(), rnd.tolist(), c_max, rounds), ([], [], 0, 1))
        check("no edges c = 1", (lambda r: (r[0], r[1], r[2].tolist(), r[3]))(nucleus34(sym, 1)), (0, 0, [], 1))
        check("no edges, local", (lambda r: (r[0], r[1].tolist()))(tri_clique4_local(sym)), (0, []))
    with pairs_graph(6, [(0, 1), (1, 2), (2, 3), (3, 0), (3, 4), (4, 5)]).to_device(dev) as sym:  # a 4-cycle with a tail
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)
        check("edges without a triangle", (theta.tolist(), rnd.tolist(), c_max, rounds), ([], [], 0, 1))
        check("edges without a triangle c = 1", (lambda r: (r[0], r[1], r[2].tolist(), r[3]))(nucleus34(sym, 1)), (0, 0, [], 1))
        check("edges without a triangle, local", (lambda r: (r[0], r[1].tolist()))(tri_clique4_local(sym)), (0, []))
    # triangles without a 4-clique: theta 0 everywhere, one round removes them all
    g = pairs_graph(5, [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)])
    with g.to_device(dev) as sym:
        check_decompose("two triangles", sym, R.decompose(g))
        check_nucleus("two triangles", sym, 0, R.nucleus(g, 0))
        check_nucleus("two triangles", sym, 1, R.nucleus(g, 1))


def test_beside_other_solvers_and_twice(dev):
    """after tc_list, gm_clique_truss_decompose and TCSolver on the same handle and before them on a fresh one: the same arrays, and the
    other solvers' results do not change; two calls in a row give identical arrays"""
    name = "rmat8_ef8_s42"
    g = load_graph(name)
    want = ref_decompose(name)
    with g.to_device(dev) as fresh:
        first = check_decompose(name + " on a fresh handle", fresh, want, rows=None)
        again = nucleus34_decompose(fresh)
        check_arrays("two calls, identical theta", again[0], first[0])
        check_arrays("two calls, identical rounds", again[1], first[1])
        rows_after = rows_of(fresh)
        theta4_after = clique_truss_decompose(fresh, 4)
        with fresh.orient() as dag:
            tc_after = TCSolver(dag)
    with g.to_device(dev) as sym:
        rows = rows_of(sym)
        theta4 = clique_truss_decompose(sym, 4)
        with sym.orient() as dag:
            tc = TCSolver(dag)
        later = check_decompose(name + " after the other solvers", sym, want, rows)
        check_arrays("fresh handle against used handle, theta", later[0], first[0])
        check_arrays("fresh handle against used handle, rounds", later[1], first[1])
        c = want.c_max // 2
        a = check_nucleus(name, sym, c, R.nucleus(prepared(name), c), rows)
        b = nucleus34(sym, c)[2]
        check_arrays("nucleus twice, identical arrays", a, b)
        check_arrays("tc_list unchanged", rows_of(sym), rows)
        check_arrays("tc_list on both handles", rows_after, rows)
        again4 = clique_truss_decompose(sym, 4)
        for i, what in enumerate(("theta", "round")):
            check_arrays(f"gm_clique_truss_decompose {what} unchanged", again4[i], theta4[i])
            check_arrays(f"gm_clique_truss_decompose {what} on both handles", theta4_after[i], theta4[i])
        check("gm_clique_truss_decompose (c_max, rounds) unchanged", again4[2:], theta4[2:])
        with sym.orient() as dag:
            check("TCSolver unchanged", (TCSolver(dag), tc_after), (tc, tc))
        check("TCSolver against the triangles listed", tc, rows.shape[0])


def test_every_block_goes_back_with_the_handle(dev):
    g = load_graph("rmat8_ef8_s42")
    before = dev_live_blocks()
    sym = g.to_device(dev)
    assert dev_live_blocks() > before
    for _ in range(2):
        theta, _, c_max, rounds = nucleus34_decompose(sym)
        check("rmat8 (c_max, rounds)", (c_max, rounds), TABLE["rmat8_ef8_s42"][2:])
    nucleus34(sym, 2)
    sym.free()
    check("live device blocks after the handle is freed", dev_live_blocks(), before)
