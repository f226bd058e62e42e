"""Local k-clique counts on the GPU (gm_clique_local, csrc/gm_kcl_local.hip): the k-cliques at every vertex and on every entry, in the
caller's numbering and entry order, against the plain Python reference of tests/clique_local_ref.py -- entry by entry, vertex by vertex --
and the total against the goldens and CliqueSolver; k = 3 against tc_local; as numbered and renumbered; a shuffled numbering; complete
graphs whose DAG rows lie on both sides of every row length at which the kernel changes path; an edge in more than 2^32 cliques; the
other solvers of the handle; the device blocks; the refusals.  Every value is printed before it is asserted."""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

import clique_local_ref as R
import truss_ref as TR
import twin_graphs as T
from common import GOLDEN, load_graph
from graphminer_amd import CliqueSolver, SglSolver, _lib, clique_local, tc_local

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
KCL_ROW_CONSTANTS = ["kcl_local_regs2_row", "kcl_local_regs8_row", "kcl_local_regs12_row", "kcl_local_lds_row"]  # every row length at which the kernel changes path (gm_constant)
SMALL = [(n, k) for n in ("citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42") for k in range(3, 9)] + [("rmat10_ef16_s42", 4), ("rmat10_ef16_s42", 5)]


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def golden(name, k):
    return GOLDEN[name]["tc"] if k == 3 else GOLDEN[name][f"clique{k}"]


@functools.lru_cache(maxsize=None)
def ref(name, k):
    g = load_graph(name)
    ent = R.entry_cliques(g, k)
    ent.setflags(write=False)
    kv = R.vertex_cliques(g, k, ent)
    kv.setflags(write=False)
    return ent, kv


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def check_arrays(label, got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    print(f"{label}: {len(want)} values, {bad.size} differ, first at {bad[:5].tolist()}: got {np.asarray(got)[bad[:5]].tolist()} "
          f"want {np.asarray(want)[bad[:5]].tolist()}", flush=True)
    assert got.dtype == want.dtype and got.shape == want.shape and bad.size == 0, label


@pytest.mark.parametrize("name,k", SMALL)
def test_small_graphs(dev, name, k):
    g = load_graph(name)
    want_ent, want_kv = ref(name, k)
    with g.to_device(dev) as sym:
        total, kv, ent, st = clique_local(sym, k, return_stats=True)
        check_arrays(f"{name} k={k} entries", ent, want_ent)
        check_arrays(f"{name} k={k} K_v", kv, want_kv)
        assert ent.dtype == np.uint64 and ent.shape == (g.E(),) and kv.dtype == np.uint64 and kv.shape == (g.V(),)
        check(f"{name} k={k} total", total, golden(name, k))
        check(f"{name} k={k} stats.tasks", st.tasks, g.E())
        print(f"{name} k={k} kernel_ms {st.kernel_ms}", flush=True)
        assert st.kernel_ms > 0
        with sym.orient() as dag:
            check(f"{name} k={k} total against CliqueSolver", total, CliqueSolver(dag, k))
        # each output left out in turn, and both; every one of them is a further call on the same handle
        total, kv, ent = clique_local(sym, k, vertex=False)
        check(f"{name} k={k} entries only", (total, kv), (golden(name, k), None))
        check_arrays(f"{name} k={k} entries only", ent, want_ent)
        total, kv, ent = clique_local(sym, k, entries=False)
        check(f"{name} k={k} vertices only", (total, ent), (golden(name, k), None))
        check_arrays(f"{name} k={k} vertices only", kv, want_kv)
        check(f"{name} k={k} neither", clique_local(sym, k, vertex=False, entries=False), (golden(name, k), None, None))
        total, kv, ent = clique_local(sym, k)
        check_arrays(f"{name} k={k} entries again", ent, want_ent)
        check_arrays(f"{name} k={k} K_v again", kv, want_kv)


def test_k3_agrees_with_tc_local(dev):
    name = "rmat10_ef16_s42"
    with load_graph(name).to_device(dev) as sym:
        t_total, tv, sup = tc_local(sym)
        total, kv, ent = clique_local(sym, 3)
    check_arrays("k=3 entries against the supports", ent, sup.astype(np.uint64))
    check_arrays("k=3 K_v against T_v", kv, tv)
    check("k=3 total", total, t_total)


@pytest.mark.parametrize("name", ["citeseer", "rmat10_ef16_s42"])
def test_as_numbered(dev, name):
    want_ent, want_kv = ref(name, 4)
    with load_graph(name).to_device(dev) as sym:
        total, kv, ent = clique_local(sym, 4, tune=t6(AS_NUMBERED))
        check_arrays(f"{name} as numbered entries", ent, want_ent)
        check_arrays(f"{name} as numbered K_v", kv, want_kv)
        check(f"{name} as numbered total", total, golden(name, 4))
        # the default numbering after the other one on the same handle
        total, kv, ent = clique_local(sym, 4)
        check_arrays(f"{name} default after as numbered entries", ent, want_ent)
        check_arrays(f"{name} default after as numbered K_v", kv, want_kv)
        check(f"{name} default total", total, golden(name, 4))


@pytest.mark.parametrize("family,params,seed", [("split", (6, 5), 3), ("multipartite", (4, 7), 11), ("book", (90,), 5)])
def test_shuffled_numbering(dev, family, params, seed):
    g = T.graph(family, params, order="random", seed=seed)
    assert not np.array_equal(T.numbering(*T.pairs(family, params), "random", seed), np.arange(g.V()))
    want_ent = R.entry_cliques(g, 4)
    want_kv = R.vertex_cliques(g, 4, want_ent)
    with g.to_device(dev) as sym:
        for tune in (None, t6(AS_NUMBERED)):
            total, kv, ent = clique_local(sym, 4, tune=tune)
            check_arrays(f"{family}{params} shuffled tune={tune} entries", ent, want_ent)
            check_arrays(f"{family}{params} shuffled tune={tune} K_v", kv, want_kv)
            check(f"{family}{params} total", total, sum(int(x) for x in want_kv) // 4)


def path_boundaries():
    lib, out = _lib.load(), []
    for name in KCL_ROW_CONSTANTS:
        v = C.c_int64(0)
        _lib.check(lib.gm_constant(name.encode(), C.byref(v)), "gm_constant")
        out.append((name, int(v.value)))
    return out


@pytest.mark.parametrize("name", KCL_ROW_CONSTANTS)
def test_every_path_boundary(dev, name):
    """complete (t + 2,): the DAG rows of K_n have every length 0 .. n - 1, so both sides of t and the row of t entries itself are reached"""
    t = dict(path_boundaries())[name]
    n = t + 2
    g = T.graph("complete", (n,))
    with g.to_device(dev) as sym:
        total, kv, ent, st = clique_local(sym, 4, return_stats=True)
    print(f"{name} = {t}: K_{n} kernel_ms {st.kernel_ms}", flush=True)
    check(f"K_{n} entries", np.unique(ent).tolist(), [comb(n - 2, 2)])
    check(f"K_{n} K_v", np.unique(kv).tolist(), [comb(n - 1, 3)])
    check(f"K_{n} total", total, comb(n, 4))
    assert ent.shape == (g.E(),) and kv.shape == (n,)


def test_split_rows(dev):
    """k >= 5 shares a root of more than kcl_local_split_row out-neighbours among several workgroups: complete (t + 2,) at k = 5"""
    v = C.c_int64(0)
    _lib.check(_lib.load().gm_constant(b"kcl_local_split_row", C.byref(v)), "gm_constant")
    n = int(v.value) + 2
    g = T.graph("complete", (n,))
    with g.to_device(dev) as sym:
        total, kv, ent, st = clique_local(sym, 5, return_stats=True)
    print(f"kcl_local_split_row = {n - 2}: K_{n} k=5 kernel_ms {st.kernel_ms}", flush=True)
    check(f"K_{n} k=5 entries", np.unique(ent).tolist(), [comb(n - 2, 3)])
    check(f"K_{n} k=5 K_v", np.unique(kv).tolist(), [comb(n - 1, 4)])
    check(f"K_{n} k=5 total", total, comb(n, 5))


def test_rows_of_several_lane_words(dev):
    """K_2060: rows of up to 2059 entries -- candidate sets of more than 64 words, more than one word per lane of the wide kernel"""
    n = 2060
    g = T.graph("complete", (n,))
    with g.to_device(dev) as sym:
        total, kv, ent, st = clique_local(sym, 4, return_stats=True)
    print(f"K_{n} kernel_ms {st.kernel_ms}", flush=True)
    check(f"K_{n} entries", np.unique(ent).tolist(), [comb(n - 2, 2)])
    check(f"K_{n} K_v", np.unique(kv).tolist(), [comb(n - 1, 3)])
    check(f"K_{n} total", total, comb(n, 4))


def test_beyond_32_bits(dev):
    """A(5, 85) at k = 7: 427 vertices, the edge (a, b) lies in 85^5 = 4,437,053,125 > 2^32 cliques"""
    p, s = 5, 85
    g, part = R.apex(p, s)
    want_ent, want_kv = R.apex_expected(g, part, p, s)
    assert s ** p > 2 ** 32 and g.V() == 427
    with g.to_device(dev) as sym:
        total, kv, ent, st = clique_local(sym, p + 2, return_stats=True)
    print(f"A({p},{s}) kernel_ms {st.kernel_ms}", flush=True)
    check_arrays(f"A({p},{s}) entries", ent, want_ent)
    check_arrays(f"A({p},{s}) K_v", kv, want_kv)
    check(f"A({p},{s}) entry classes", sorted(np.unique(ent).tolist()), [s ** (p - 2), s ** (p - 1), s ** p])
    check(f"A({p},{s}) total", total, s ** p)


def test_other_solvers_keep_their_results(dev):
    name = "rmat10_ef16_s42"
    g = load_graph(name)
    want_sup = TR.supports(g)

    def others(sym, dag, when):
        check(f"4-clique {when}", CliqueSolver(dag, 4), GOLDEN[name]["clique4"])
        check(f"diamond {when}", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])
        check_arrays(f"supports {when}", tc_local(sym)[2], want_sup)

    with g.to_device(dev) as sym, sym.orient() as dag:
        others(sym, dag, "before")
        total, kv, ent = clique_local(sym, 4)
        check_arrays("k=4 entries between", ent, ref(name, 4)[0])
        check_arrays("k=4 K_v between", kv, ref(name, 4)[1])
        others(sym, dag, "after")
        total, kv, ent = clique_local(sym, 5)
        check_arrays("k=5 entries after", ent, ref(name, 5)[0])
        check_arrays("k=5 K_v after", kv, ref(name, 5)[1])
        check("k=5 total", total, GOLDEN[name]["clique5"])
    with g.to_device(dev) as sym:  # the local clique counts first on a fresh handle
        check_arrays("k=4 entries first", clique_local(sym, 4)[2], ref(name, 4)[0])
        check("diamond after a first clique_local", SglSolver(sym, "diamond"), GOLDEN[name]["diamond"])


def test_blocks_come_back(dev):
    from graphminer_amd._lib import dev_live_blocks

    g = load_graph("rmat8_ef8_s42")
    before = dev_live_blocks()
    with g.to_device(dev) as sym:
        for k in (4, 4, 5, 5, 3, 3):
            check(f"k={k} total", clique_local(sym, k)[0], golden("rmat8_ef8_s42", k))
        during = dev_live_blocks()
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
        check("world = 2", lib.gm_clique_local(sym.handle, 4, C.byref(la), None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
        la = _lib.gm_launch()
        buf = torch.zeros(8, dtype=torch.int64, device=f"cuda:{dev}")
        la.d_counts = buf.data_ptr()
        check("d_counts", lib.gm_clique_local(sym.handle, 4, C.byref(la), None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
        check("k = 2", lib.gm_clique_local(sym.handle, 2, None, None, None, C.byref(total), None), _lib.GM_ERR_INVALID)
        check("k = 13", lib.gm_clique_local(sym.handle, 13, None, None, None, C.byref(total), None), _lib.GM_ERR_INVALID)
        check("k = 9", lib.gm_clique_local(sym.handle, 9, None, None, None, C.byref(total), None), _lib.GM_ERR_UNSUPPORTED)
        check("null handle", lib.gm_clique_local(None, 4, None, None, None, C.byref(total), None), _lib.GM_ERR_INVALID)
    with Graph(row_ptr=[0, 0, 0, 0], col_idx=[]).to_device(dev) as sym:
        total, kv, ent = clique_local(sym, 4)
        check("no edges", (total, kv.tolist(), ent.tolist()), (0, [0, 0, 0], []))
