"""Local motif counts on the GPU (gm_motif_local, csrc/gm_orbit_local.hip): the 15 graphlet-degree orbits of every vertex, every value of
every orbit against the numpy composition of tests/motif_local_ref.py (b) -- itself checked against the enumeration, the goldens and
closed forms in tests/test_motif_local_host.py -- and `counts` against the goldens' motif3 / motif4 and MotifSolver.  Every cell runs on
the default copy and under GM_T6_AS_NUMBERED.  The cells: the small goldens (citeseer and rmat10 also on the hashed set's global-memory
lookup); K_1300 and K_2060 with satellites -- the 2048-entry stage of the credit pass (also with both stages in one launch) and its
wave-per-edge form; the hub-corner branch of the credit pass (rmat10, the last 512 rows left to the matrix cores); rows on both sides of the gather kernels' split and one of 5,200 entries; K_{1,3000} and the book B_70000 past 2^32
and 2^16; a triangle-free graph with hubs inside sentinels; k = 3; outputs left out; the other solvers of the handle; the device blocks;
the refusals.
The two dense cells are NOT a K_n with 1-2 % of its edges removed: clique_local_ref cannot enumerate the 4-cliques of such a graph in
seconds.  They are a plain K_n with a few hundred satellites, each attached to 2 .. 12 seeded random clique vertices: degrees, supports and
diamond counts of the clique's vertices and edges differ, K_v is C(n - 1, 3) plus a closed term per satellite, and t(e), R_v and the diamond
term come from float64 products of the dense adjacency matrix (motif_local_ref.dense_inputs; checked against the enumeration on a small
instance by the host test).  Every figure is printed before it is asserted."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

import motif_local_ref as M
import oracle as O
import planted_squares as P
import rect_local_ref as RR
import truss_ref as TR
from common import GOLDEN, load_graph, random_graph, sup_core_info
from graphminer_amd import MotifSolver, SglSolver, _lib, clique_local, motif_local, rect_local, tc_local

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
HSET_FALLBACK = 0x800000
SMALL = ["rmat6_ef4_s1", "rmat8_ef8_s42", "citeseer", "cora", "rmat10_ef16_s42"]
DENSE = {"stage-2048": (1300, 400), "beyond-stage": (2060, 500)}


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@functools.lru_cache(maxsize=None)
def wave_row():
    v = C.c_int64(0)
    assert _lib.load().gm_constant(b"orbit_wave_row", C.byref(v)) == _lib.GM_OK
    return int(v.value)


def gather_rows_graph():
    """a sparse random base of 5,400 vertices and four more: rows of orbit_wave_row - 1, + 0, + 1 entries and one of 5,200, each attached to
    seeded random base vertices (the base rows stay far below the split)"""
    w = wave_row()
    base = random_graph(5400, 16000, 17)
    nb = base.V()
    src = np.repeat(np.arange(nb, dtype=np.int64), np.diff(base.row_ptr))
    col = base.col_idx.astype(np.int64)
    half = src < col
    s, d = [src[half]], [col[half]]
    rng = np.random.default_rng(23)
    want = [w - 1, w, w + 1, 5200]
    for i, k in enumerate(want):
        att = rng.choice(nb, size=k, replace=False)
        s.append(att.astype(np.int64))
        d.append(np.full(k, nb + i, dtype=np.int64))
    g = P._graph(nb + 4, np.concatenate(s), np.concatenate(d))
    deg = np.diff(g.row_ptr)
    assert deg[nb:].tolist() == want and int(deg[:nb].max()) < w - 1, "the four planted rows straddle the split, no base row reaches it"
    return g


def hubs_graph(n=2500, leaves=3000):
    """K_{2,n} (hubs 0 and 1) with `leaves` further leaves on hub 0: no triangle, C(n, 2) 4-cycles at each hub"""
    mid = np.arange(2, n + 2, dtype=np.int64)
    lf = np.arange(n + 2, n + 2 + leaves, dtype=np.int64)
    s = np.concatenate([np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64), np.zeros(leaves, dtype=np.int64)])
    return P._graph(n + 2 + leaves, s, np.concatenate([mid, mid, lf]))


def book_graph(n):
    pages = np.arange(2, n + 2, dtype=np.int64)
    s = np.concatenate([[0], np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)])
    return P._graph(n + 2, s, np.concatenate([[1], pages, pages]))


def star_graph(m):
    return P._graph(m + 1, np.zeros(m, dtype=np.int64), np.arange(1, m + 1, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def case(name):
    """(graph, the 15 x nv reference) of a cell, computed once and left unchanged"""
    if name in DENSE:
        core, n_out = DENSE[name]
        g = M.clique_with_satellites(core, n_out, seed=core)
        want = M.compose_from(g, *M.dense_inputs(g, core))
    elif name == "gather-rows":
        g = gather_rows_graph()
        want = M.compose(g)
    elif name == "hubs":
        g = hubs_graph()
        want = M.compose(g)
    elif name == "star":
        g, want = star_graph(3000), M.star_orbits(3000)
    elif name == "book":
        g, want = book_graph(70000), M.book_orbits(70000)
    else:
        g = load_graph(name)
        want = M.compose(g)
    want.setflags(write=False)
    return g, want


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_orbits(label, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    per_orbit = np.bincount(bad[:, 0], minlength=want.shape[0]).tolist() if len(bad) else []
    print(f"{label}: {want.shape} values, {len(bad)} differ {per_orbit}, first at {bad[:4].tolist()}: got {[int(got[tuple(i)]) for i in bad[:4]]} "
          f"want {[int(want[tuple(i)]) for i in bad[:4]]}", flush=True)
    assert len(bad) == 0, label


def distinct_enough(name, want, per_orbit=True):
    """the cell can tell a credit on the wrong entry: at least 32 distinct non-zero values in the orbits 10, 12 and 13 -- in each of them,
    except on rmat6_ef4_s1, whose 64 vertices show 24 distinct values in orbit 13: there the three orbits together (the triangle-free
    cells -- the hubs, the star -- and the book are there for other reasons)"""
    n = [int(np.unique(want[o][want[o] > 0]).size) for o in (10, 12, 13)]
    rows = want[[10, 12, 13]]
    together = int(np.unique(rows[rows > 0]).size)
    print(f"{name}: distinct non-zero values in orbits 10, 12, 13: {n}, together {together}", flush=True)
    assert together >= 32 and (min(n) >= 32 or not per_orbit), name


def longest_dag_row(g):
    return int(np.diff(O.orient(O.OGraph(g.row_ptr, g.col_idx)).row_ptr).max())


def compare(label, g, dev, want, tunes=(None, t6(AS_NUMBERED)), sym=None):
    want_counts = M.counts(want)
    own = sym is None
    sym = g.to_device(dev) if own else sym
    try:
        for tune in tunes:
            counts, orb, st = motif_local(sym, 4, tune=tune, return_stats=True)
            where = f"{label} tune={tune[6] if tune else 0:#x}"
            print(f"{where}: kernel_ms {st.kernel_ms}", flush=True)
            check_orbits(f"{where} orbits", orb, want)
            check(f"{where} counts", counts, want_counts)
            check(f"{where} stats.tasks", st.tasks, g.E())
            assert st.kernel_ms > 0
    finally:
        if own:
            sym.free()
    return want_counts


@pytest.mark.parametrize("name", SMALL)
def test_small_graphs(dev, name):
    g, want = case(name)
    distinct_enough(name, want, per_orbit=name != "rmat6_ef4_s1")
    check(f"{name} reference counts against the golden", M.counts(want), GOLDEN[name]["motif4"])
    tunes = (None, t6(AS_NUMBERED)) + ((t6(HSET_FALLBACK),) if name in ("citeseer", "rmat10_ef16_s42") else ())
    with g.to_device(dev) as sym:
        compare(name, g, dev, want, tunes=tunes, sym=sym)
        check(f"{name} counts against MotifSolver(4)", motif_local(sym, 4, orbits=False)[0], MotifSolver(sym, 4))
        c3, o3 = motif_local(sym, 3)
        check(f"{name} k = 3 counts", c3, GOLDEN[name]["motif3"])
        check(f"{name} k = 3 counts against MotifSolver(3)", c3, MotifSolver(sym, 3))
        check_orbits(f"{name} k = 3 orbits", o3, want[:4])


def test_shuffled_ids(dev):
    name = "rmat10_ef16_s42"
    g, want = case(name)
    h, newid = P.shuffled(g, seed=11)
    want_h = np.empty_like(want)
    want_h[:, newid] = want
    compare(f"{name} shuffled", h, dev, want_h)


@pytest.mark.parametrize("split", [None, "1"])
def test_stage_2048(dev, devopt, split):
    """K_1300 with satellites: DAG rows of about 1,290 entries -- the 2048-entry stage of the credit pass; GM_TCT_SPLIT_ALWAYS=1: both
    stages in one launch, each on the hosts of its own table (a fresh handle: the option is read when its tables are built)"""
    g, want = case("stage-2048")
    row = longest_dag_row(g)
    print(f"stage-2048: longest DAG row {row}", flush=True)
    assert 1024 < row <= 2048
    distinct_enough("stage-2048", want)
    devopt("GM_TCT_SPLIT_ALWAYS", split)
    if split is None:
        compare(f"K_1300 + satellites split={split}", g, dev, want)
    else:  # (with shuffled ids: the satellites' rows lie among the clique's)
        h, newid = P.shuffled(g, seed=7)
        want_h = np.empty_like(want)
        want_h[:, newid] = want
        compare(f"K_1300 + satellites shuffled split={split}", h, dev, want_h)


def test_rows_beyond_the_stage(dev):
    """K_2060 with satellites: the DAG rows beyond 2,048 entries host nothing -- their out-edges are the wave-per-edge kernel's"""
    g, want = case("beyond-stage")
    row = longest_dag_row(g)
    print(f"beyond-stage: longest DAG row {row}", flush=True)
    assert row > 2048
    distinct_enough("beyond-stage", want)
    compare("K_2060 + satellites", g, dev, want)


def test_hub_corner(dev, devopt):
    """the branch `corner_from < nv` of the credit pass: the task lists leave the rows of the last 512 vertices out (the set-up of
    tests/test_gpu_supcorner.py), and the wave-per-edge credit kernel walks their out-edges from the rows themselves -- no row list, the tail
    of N+(u) beyond v.  gm_sup_core_info proves that the handle has that corner (a fresh handle: the options are read when its tables are built)"""
    devopt("GM_TOPO_MIN_ROW", "0")
    devopt("GM_SUP_CORE_H", "512")
    name = "rmat10_ef16_s42"
    g, want = case(name)
    distinct_enough(name, want)
    with g.to_device(dev) as sym:
        compare(f"{name} corner 512", g, dev, want, sym=sym)
        info = sup_core_info(sym)
        check("corner vertices", info["vertices"], 512)
        assert info["entries"] > 0


def test_gather_rows_on_both_sides_of_the_split(dev):
    g, want = case("gather-rows")
    distinct_enough("gather-rows", want)
    compare("gather rows", g, dev, want)


def test_star_past_2_32(dev):
    m = 3000
    g, want = case("star")
    assert int(want[7, 0]) == comb(m, 3) == 4495501000 > 2 ** 32 and int(want[6, 1]) == comb(m - 1, 2)
    compare(f"K_1,{m}", g, dev, want)


@pytest.mark.timeout(300)
def test_book_supports_past_2_16(dev):
    n = 70000
    g, want = case("book")
    assert n > 65535 and int(want[6, 2]) > 2 ** 32 and int(want[12, 2]) == n - 1 == 69999
    compare(f"B_{n}", g, dev, want)


def test_triangle_free_with_hubs_inside_sentinels(dev):
    import torch

    g, want = case("hubs")
    assert not want[[3, 9, 10, 11, 12, 13, 14]].any() and int(want[8].max()) == comb(2500, 2)
    lib, pad, sentinel, nv = _lib.load(), 1024, -7, g.V()
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            buf = torch.full((15 * nv + 2 * pad,), sentinel, dtype=torch.int64, device=f"cuda:{dev}")
            la, counts = _lib.gm_launch(), (C.c_uint64 * 6)()
            if tune:
                la.tune[6] = tune[6]
            rc = lib.gm_motif_local(sym.handle, 4, C.byref(la), buf.data_ptr() + 8 * pad, counts, 6, None)
            host = buf.cpu().numpy()
            check(f"hubs tune={tune} rc", rc, _lib.GM_OK)
            check_orbits(f"hubs tune={tune} orbits", host[pad:-pad].view(np.uint64).reshape(15, nv), want)
            check(f"hubs tune={tune} counts", [int(x) for x in counts], M.counts(want))
            assert (host[:pad] == sentinel).all() and (host[-pad:] == sentinel).all()


def test_k3_builds_nothing_of_k4(dev):
    """k = 3 on a fresh handle: orbits 0 .. 3, and nothing of the rectangles or the k-cliques is built.  The rectangle plan of
    gm_rect_local has no info call of its own (gm_map_plan_info reports the plans of SglSolver's map kernels), so the device blocks are
    compared instead: k = 3 leaves exactly the blocks gm_tc_local leaves plus its one array; k = 4 afterwards adds the plan, the credits and
    the k-clique arrays."""
    from graphminer_amd._lib import dev_live_blocks

    g, want = case("cora")
    before = dev_live_blocks()
    with g.to_device(dev) as sym:
        tc_local(sym, vertex=False, entries=False)
        after_tc = dev_live_blocks()
    with g.to_device(dev) as sym:
        counts, orb, st3 = motif_local(sym, 3, return_stats=True)
        after_k3 = dev_live_blocks()
        check_orbits("k = 3 orbits", orb, want[:4])
        check("k = 3 counts", counts, GOLDEN["cora"]["motif3"])
        with pytest.raises(Exception):
            from graphminer_amd import map_plan_info

            map_plan_info(sym, "rectangle")  # (no map plan either)
        _, _, st4 = motif_local(sym, 4, return_stats=True)
        after_k4 = dev_live_blocks()
    print(f"live blocks: before {before}, tc_local {after_tc}, k = 3 {after_k3}, then k = 4 {after_k4}; kernel_ms k = 3 {st3.kernel_ms} k = 4 {st4.kernel_ms}", flush=True)
    assert after_k3 - before == after_tc - before + 1
    assert after_k4 > after_k3 + 3
    assert dev_live_blocks() == before


def test_outputs_left_out_and_repeated_calls(dev):
    g, want = case("rmat8_ef8_s42")
    lib, nv = _lib.load(), g.V()
    import torch

    with g.to_device(dev) as sym:
        counts, orb = motif_local(sym, 4, orbits=False)
        check("counts only", (counts, orb), (M.counts(want), None))
        buf = torch.zeros(15 * nv, dtype=torch.int64, device=f"cuda:{dev}")
        check("orbits only rc", lib.gm_motif_local(sym.handle, 4, None, buf.data_ptr(), None, 0, None), _lib.GM_OK)
        check_orbits("orbits only", buf.cpu().numpy().view(np.uint64).reshape(15, nv), want)
        check("neither rc", lib.gm_motif_local(sym.handle, 4, None, None, None, 0, None), _lib.GM_OK)
        first, second = motif_local(sym, 4), motif_local(sym, 4)
        check_orbits("two calls in a row", second[1], first[1])
        check_orbits("two calls in a row against the reference", second[1], want)
        check("counts, two calls", (first[0], second[0]), (M.counts(want), M.counts(want)))


def test_other_solvers_keep_their_results_and_blocks_come_back(dev):
    from graphminer_amd._lib import dev_live_blocks

    name = "rmat10_ef16_s42"
    g, want = case(name)
    want_sup = TR.supports(g)
    want_rect = RR.rect_local(g)[0]
    before = dev_live_blocks()

    def others(sym, when):
        total, tv, sup = tc_local(sym)
        check_orbits(f"supports {when}", sup, want_sup)
        check_orbits(f"T_v {when}", tv, want[3])
        check_orbits(f"rectangle entries {when}", rect_local(sym)[2], want_rect)
        check(f"4-clique total {when}", clique_local(sym, 4)[0], GOLDEN[name]["clique4"])
        check(f"MotifSolver(4) {when}", MotifSolver(sym, 4), GOLDEN[name]["motif4"])
        check(f"diamond {when}", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
        return clique_local(sym, 4)[2]

    with g.to_device(dev) as sym:
        k4_before = others(sym, "before")
        for tune in (None, t6(AS_NUMBERED), None):
            counts, orb = motif_local(sym, 4, tune=tune)
            check_orbits(f"orbits between, tune={tune}", orb, want)
        k4_after = others(sym, "after")
        check_orbits("4-clique entries before and after", k4_after, k4_before)
        during = dev_live_blocks()
    with g.to_device(dev) as sym:  # the local motif counts first on a fresh handle
        check_orbits("orbits first", motif_local(sym, 4)[1], want)
        others(sym, "after a first motif_local")
    after = dev_live_blocks()
    print(f"live blocks: before {before} during {during} after {after}", flush=True)
    assert during > before and after == before


def test_refusals_and_the_empty_graph(dev):
    import torch

    from graphminer_amd import Graph

    lib = _lib.load()
    counts = (C.c_uint64 * 6)(*[5] * 6)
    with load_graph("citeseer").to_device(dev) as sym:
        la = _lib.gm_launch()
        la.rank, la.world = 0, 2
        check("world = 2", lib.gm_motif_local(sym.handle, 4, C.byref(la), None, counts, 6, None), _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        buf = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = buf.data_ptr()
        check("d_counts", lib.gm_motif_local(sym.handle, 4, C.byref(la), None, counts, 6, None), _lib.GM_ERR_UNSUPPORTED)
        check("null handle", lib.gm_motif_local(None, 4, None, None, counts, 6, None), _lib.GM_ERR_INVALID)
        for k in (2, 5, 0, -1):
            check(f"k = {k}", lib.gm_motif_local(sym.handle, k, None, None, counts, 6, None), _lib.GM_ERR_INVALID)
        check("k = 4, ncounts = 2", lib.gm_motif_local(sym.handle, 4, None, None, counts, 2, None), _lib.GM_ERR_INVALID)
        check("k = 3, ncounts = 6", lib.gm_motif_local(sym.handle, 3, None, None, counts, 6, None), _lib.GM_ERR_INVALID)
        check("k = 3, ncounts = 2", lib.gm_motif_local(sym.handle, 3, None, None, counts, 2, None), _lib.GM_OK)
        check("k = 3 counts", [int(counts[0]), int(counts[1])], GOLDEN["citeseer"]["motif3"])
    with Graph(row_ptr=[0, 2, 3, 4], col_idx=[2, 1, 0, 0]).to_device(dev) as sym:  # row 0 descends
        check("unsorted rows", lib.gm_motif_local(sym.handle, 4, None, None, counts, 6, None), _lib.GM_ERR_INVALID)
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        for k, n in ((3, 2), (4, 6)):
            c, orb = motif_local(sym, k)
            check(f"no edges, k = {k}", (c, orb.tolist()), ([0] * n, [[0, 0, 0]] * M.N_ORBITS[k]))
