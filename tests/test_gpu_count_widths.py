"""Counts at the widths of the kernels' counters and past 2^32, on twin-class graphs whose exact counts tests/twin_graphs.py gives at any
size (closed forms, or exact interpolation from the CPU oracle at small sizes: tests/test_twin_reference.py pins both):
  * rect_lds_kernel keeps 8-, 16- or 32-bit counters per id range, the width from the range's largest degree (255 / 256 / 65535 / 65536
    straddle the steps), and sums C(c, 2) over the fields it reads back: K_{4,b} and S_{4,b} put up to eight ends of one aligned group
    at c = 60 K .. 65 K -- the rectangle through every implementation, rank shares and the 4-motif that reuses the kernel;
  * house_lds_kernel's packed fields (6+10 / 11+21 bits for centres of at most 32 / 1024 neighbours, 24 | 40 bits else): K_33, K_34,
    K_1025, K_1026 and S_{4,65532}; pentagon past 2^32 on S_{4,65532} (the rank shares of both are exact modulo 2^64, as dist.py sums);
  * the book B_70000: one edge with 70,000 triangles (supports of 2^16 and more), diamond / TC / 3-motif / 4-motif and the closed-form
    patterns past 2^32;
  * k-cliques of complete multipartite graphs past 2^32, the 4-cliques on DAG rows of more than 256 entries (the matrix-core classes);
  * every family at the top of an id space of 2^24 and 2^24 + 1 vertices.
Every value is printed before it is asserted."""
import ctypes as C
from math import comb

import numpy as np
import pytest

import twin_graphs as T
from common import MotifSolverE
from graphminer_amd import CliqueSolver, MotifSolver, SglSolver, TCSolver, _lib
from graphminer_amd.solvers import sgl4_finish, sgl4_partial

pytestmark = pytest.mark.gpu
GLOBAL_MAPS = 0x20000
FLAT = 0x800  # rectangle / pentagon as wedges + flat intersections, house flattened over (v0, v1, v3)
AS_NUMBERED = 0x200
HOUSE_NO_BITMAP = 0x8000
PER_EDGE = 0x10000000
SUP_ATOMIC = 0x40000000
HSET_FALLBACK = 0x800000
SORTED_COPY_CLASSES = 0x400000  # per-edge kernels: the sorted LDS copy + bisection instead of the hashed rows
CLIQUE_MINING = 0x40000  # 4-clique in the mining kernel alone
CLIQUE_ROW_GATHER = 0x8000000  # 4-clique: the wide rows gathered row by row from the core bitmap
M64 = 2**64


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def ranks(fn, world=3, policy=0, mod=None):
    tot = sum(fn(rank=r, world=world, policy=policy) for r in range(world))
    return tot % mod if mod else tot


def motif4_ranks(sym, world=3, policy=0, tune=None):
    """4-motif split over ranks: every rank's raw sums (gm_motif4_partial) added modulo 2^64, then one gm_motif4_finish"""
    lib, tot = _lib.load(), [0] * 6
    for r in range(world):
        la = _lib.gm_launch()
        la.rank, la.world, la.policy = r, world, policy
        for i, t in enumerate(tune or []):
            la.tune[i] = t
        raw = (C.c_uint64 * 6)()
        assert lib.gm_motif4_partial(sym.handle, C.byref(la), raw, None) == 0
        tot = [(a + int(b)) % M64 for a, b in zip(tot, raw)]
    out = (C.c_uint64 * 6)()
    assert lib.gm_motif4_finish((C.c_uint64 * 6)(*tot), out) == 0
    return [int(x) for x in out]


def hub_b(family, deg):
    """b such that the largest degree of family(4, b) is `deg` (K_{4,b}: the hubs have b; S_{4,b}: clique vertex 0 has b + 4)"""
    return deg if family == "kab" else deg - 4


# ---- rectangle: counter widths ---------------------------------------------------------------------------------------------------
RECT = [("kab", d) for d in (255, 256, 60000, 65535, 65536)] + [("split", d) for d in (255, 256, 65535, 65536)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("family,deg", RECT, ids=[f"{f}-{d}" for f, d in RECT])
def test_rectangle_counter_widths(dev, devopt, family, deg):
    p = (4, hub_b(family, deg))
    want = T.expected(family, p, "rectangle")
    want4 = T.expected(family, p, "motif4")
    g = T.graph(family, p, "degree")
    assert int(np.diff(g.row_ptr).max()) == deg
    tag = f"{family}{p}"
    with T.graph(family, p, "random", seed=deg).to_device(dev) as sym:
        check(f"{tag} random numbering, default", SglSolver(sym, "rectangle"), want)
    with g.to_device(dev) as sym:
        check(f"{tag} default", SglSolver(sym, "rectangle"), want)
        check(f"{tag} global maps", SglSolver(sym, "rectangle", tune=t6(GLOBAL_MAPS)), want)
        check(f"{tag} flattened", SglSolver(sym, "rectangle", tune=t6(FLAT)), want)
        check(f"{tag} as numbered", SglSolver(sym, "rectangle", tune=t6(AS_NUMBERED)), want)
        for policy in (0, 1):
            check(f"{tag} ranks policy {policy}", ranks(lambda **kw: SglSolver(sym, "rectangle", **kw), policy=policy), want)
        check(f"{tag} motif4", MotifSolver(sym, 4), want4)
        check(f"{tag} motif4 global maps", MotifSolver(sym, 4, tune=t6(GLOBAL_MAPS)), want4)
        check(f"{tag} motif4 ranks", motif4_ranks(sym, policy=1), want4)
    devopt("GM_RECT_LDS_MIN", "1")
    with g.to_device(dev) as sym:
        check(f"{tag} LDS_MIN=1", SglSolver(sym, "rectangle"), want)
        check(f"{tag} LDS_MIN=1 motif4", MotifSolver(sym, 4), want4)
    for nr in ("1", "2"):
        devopt("GM_RECT_LDS_RANGES", nr)
        with g.to_device(dev) as sym:
            check(f"{tag} LDS_MIN=1 RANGES={nr}", SglSolver(sym, "rectangle"), want)
            check(f"{tag} LDS_MIN=1 RANGES={nr} ranks", ranks(lambda **kw: SglSolver(sym, "rectangle", **kw), policy=1), want)


# ---- house: packed fields ----------------------------------------------------------------------------------------------------------
HOUSE = [("complete", (33,)), ("complete", (34,)), ("complete", (1025,)), ("complete", (1026,)), ("split", (4, 65532))]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("family,p", HOUSE, ids=[f"{f}-{p[-1]}" for f, p in HOUSE])
def test_house_fields(dev, devopt, family, p):
    want = T.expected(family, p, "house")
    tag = f"{family}{p}"
    g = T.graph(family, p, "degree")
    with g.to_device(dev) as sym:
        check(f"{tag} default", SglSolver(sym, "house"), want)
        check(f"{tag} ranks", ranks(lambda **kw: SglSolver(sym, "house", **kw), mod=M64), want)
        for t in (GLOBAL_MAPS, FLAT, HOUSE_NO_BITMAP, FLAT | AS_NUMBERED):
            check(f"{tag} tune {t:#x}", SglSolver(sym, "house", tune=t6(t)), want)
    devopt("GM_RECT_LDS_MIN", "1")
    with g.to_device(dev) as sym:
        check(f"{tag} LDS_MIN=1", SglSolver(sym, "house"), want)
        check(f"{tag} LDS_MIN=1 ranks", ranks(lambda **kw: SglSolver(sym, "house", **kw), mod=M64), want)


# ---- pentagon past 2^32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_pentagon_past_2_32(dev):
    p = (4, 65532)
    want = T.expected("split", p, "pentagon")
    assert want > 2**32
    with T.graph("split", p, "degree").to_device(dev) as sym:
        check("pentagon default", SglSolver(sym, "pentagon"), want)
        check("pentagon flattened", SglSolver(sym, "pentagon", tune=t6(FLAT)), want)
        check("pentagon flattened as numbered", SglSolver(sym, "pentagon", tune=t6(FLAT | AS_NUMBERED)), want)
        check("pentagon ranks", ranks(lambda **kw: SglSolver(sym, "pentagon", **kw), mod=M64), want)  # (partials are exact modulo 2^64)


# ---- supports of 2^16 and more: the book B_70000 ------------------------------------------------------------------------------------
BOOK = (70000,)


@pytest.fixture(scope="module")
def book(dev):
    g = T.graph("book", BOOK, "degree")
    sym = g.to_device(dev)
    dag = sym.orient()
    yield sym, dag
    dag.free()
    sym.free()


@pytest.mark.timeout(300)
def test_book_diamond(book):
    sym, _ = book
    want = T.expected("book", BOOK, "diamond")
    check("diamond default", SglSolver(sym, "diamond"), want)
    for t in (PER_EDGE, SUP_ATOMIC, HSET_FALLBACK):
        check(f"diamond tune {t:#x}", SglSolver(sym, "diamond", tune=t6(t)), want)
    check("diamond ranks", ranks(lambda **kw: SglSolver(sym, "diamond", **kw)), want)


@pytest.mark.timeout(300)
def test_book_tc_and_motif3(book):
    sym, dag = book
    want = T.expected("book", BOOK, "tc")
    check("tc", TCSolver(dag), want)
    check("tc as numbered", TCSolver(dag, tune=t6(AS_NUMBERED)), want)
    check("tc ranks", ranks(lambda **kw: TCSolver(dag, **kw)), want)
    m3 = T.expected("book", BOOK, "motif3")
    assert m3[0] > 2**32
    check("motif3 default", MotifSolver(sym, 3), m3)
    check("motif3 formula", MotifSolver(sym, 3, formula=True), m3)
    check("motif3 enumeration", MotifSolverE(sym, 3), m3)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("pattern", ["tailedtriangle", "4path", "3star"])
def test_book_closed_form_patterns(book, pattern):
    sym, _ = book
    want = T.expected("book", BOOK, pattern)
    assert want > 2**32
    check(pattern, SglSolver(sym, pattern), want)
    check(f"{pattern} sorted-copy classes", SglSolver(sym, pattern, tune=t6(SORTED_COPY_CLASSES)), want)
    raw = [sum(x) for x in zip(*(sgl4_partial(sym, rank=r, world=3) for r in range(3)))]
    check(f"{pattern} ranks", sgl4_finish(pattern, raw), want)


@pytest.mark.timeout(300)
def test_book_motif4(book):
    sym, _ = book
    want = T.expected("book", BOOK, "motif4")
    check("motif4", MotifSolver(sym, 4), want)
    check("motif4 sorted-copy classes", MotifSolver(sym, 4, tune=t6(SORTED_COPY_CLASSES)), want)
    check("motif4 ranks", motif4_ranks(sym), want)


# ---- k-cliques past 2^32 ---------------------------------------------------------------------------------------------------------
# (r, s, ks): r parts of s ids. The first three: the 4-clique count past 2^32 with DAG rows of more than 256 entries (the matrix-core
# classes); k = 5 on the smallest of them. The deep cliques on graphs where the k-clique count passes 2^32 and the (k-1)-cliques that
# are enumerated stay below 2 * 10^9.
CLIQUE = [(6, 131, (4, 5)), (7, 106, (4,)), (8, 89, (4,)), (6, 41, (6,)), (7, 24, (7,)), (8, 17, (8,)), (6, 60, (5,))]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r,s,ks", CLIQUE, ids=[f"r{r}-s{s}" for r, s, _ in CLIQUE])
def test_cliques_past_2_32(dev, r, s, ks):
    assert (r - 1) * s > 256 or min(ks) > 4
    with T.graph("multipartite", (r, s), "random", seed=r * s).to_device(dev) as sym, sym.orient() as dag:
        for k in ks:
            want = T.expected("multipartite", (r, s), f"clique{k}")
            assert want == comb(r, k) * s**k > 2**32
            tag = f"K_{{{s}x{r}}} {k}-clique"
            check(f"{tag} default", CliqueSolver(dag, k), want)
            for t in (CLIQUE_MINING, CLIQUE_ROW_GATHER):
                check(f"{tag} tune {t:#x}", CliqueSolver(dag, k, tune=t6(t)), want)
            check(f"{tag} ranks", ranks(lambda **kw: CliqueSolver(dag, k, **kw)), want)


# ---- ids at 2^24 -----------------------------------------------------------------------------------------------------------------
TOP = [("kab", (4, 1500)), ("book", (3000,)), ("split", (4, 1500)), ("complete", (200,)), ("multipartite", (5, 60))]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("nv", [1 << 24, (1 << 24) + 1])
@pytest.mark.parametrize("family,p", TOP, ids=[f for f, _ in TOP])
def test_ids_at_2_24(dev, family, p, nv):
    g = T.graph(family, p, "random", seed=nv, nv=nv, offset=T.top_offset(family, p, nv))
    assert g.row_ptr[-1] > g.row_ptr[-2]  # the last id is used
    tag = f"{family}{p} nv={nv}"
    with g.to_device(dev) as sym, sym.orient() as dag:
        check(f"{tag} tc", TCSolver(dag), T.expected(family, p, "tc"))
        check(f"{tag} diamond", SglSolver(sym, "diamond"), T.expected(family, p, "diamond"))
        check(f"{tag} diamond per edge", SglSolver(sym, "diamond", tune=t6(PER_EDGE)), T.expected(family, p, "diamond"))
        check(f"{tag} motif3", MotifSolver(sym, 3), T.expected(family, p, "motif3"))
        check(f"{tag} motif3 enumeration", MotifSolverE(sym, 3), T.expected(family, p, "motif3"))
        check(f"{tag} rectangle", SglSolver(sym, "rectangle"), T.expected(family, p, "rectangle"))
        check(f"{tag} rectangle global maps", SglSolver(sym, "rectangle", tune=t6(GLOBAL_MAPS)), T.expected(family, p, "rectangle"))
