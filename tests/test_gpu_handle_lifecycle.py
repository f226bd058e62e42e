"""A handle gives back every device block it took.  gm_dev_live_blocks (include/graphminer_amd.h) is read before a handle is created and again
after it is freed; in between every solver family that caches something on the handle runs, twice (the second call goes through what the
first one cached), and every count is checked against the CPU oracle / the host references.  Other tests' handles may be alive: the two
readings are compared with each other, never with zero.

Graphs, the smallest that reach the ownership cases:
  (a) 4096 random vertices (~40 k edges) + one hub joined to 3000 of them: a row beyond kBitmapMinDeg = 2048, so the chunk tables of the
      per-edge kernels borrow their bitmaps from a BitmapSet of the graph;
  (b) the same graph adopted from the caller's device arrays (gm_graph_from_device): col_idx is borrowed and must read back unchanged;
  (c) the dense random graph of test_gpu_parity.test_clique4_wide_vertices_two_phases (n = 700, p = 0.6): the wide k-clique plan and, with a
      4 MiB arena, its rounds (k = 4: the oracle needs a minute for k = 5 there; graph (a) runs k = 5)."""
import json
import os

import numpy as np
import pytest

import list_ref as RL
import oracle as O
import sgl5_ref as R5
import sgl6_ref as R6
import truss_ref as RT
from common import ROOT, MotifSolverE, csr_sha, random_graph
from graphminer_amd import CliqueSolver, DeviceGraph, MotifSolver, SglSolver, TCSolver
from graphminer_amd._lib import dev_live_blocks, dev_option
from graphminer_amd.rmat import csr_from_pairs
from graphminer_amd.solvers import (diamond_support_finish, diamond_support_partial, diamond_support_size, ktruss, sgl5_raw, sgl6_raw, tc_list,
                                    tc_local, truss_decompose)

pytestmark = pytest.mark.gpu

GLOBAL_MAPS, SGL_FLAT, NO_CLASSES = 0x20000, 0x800, 0x80000  # GM_T6_GLOBAL_MAPS, GM_T6_SGL_FLAT, GM_T6_NO_CLASSES
TRUSS_K = 4
# what the CPU oracle and the host references take many seconds for on graph (a) (the hub's 3000 neighbours: pentagon 26 s, 4-motif 13 s,
# the 6-vertex sums 30 s; the 4-cliques of graph (c) 3 s), recorded once together with the graph's hash: `python tests/test_gpu_handle_lifecycle.py` writes the file again
RECORDED = os.path.join(ROOT, "tests", "golden", "handle_lifecycle.json")


def _t6(flags):
    return [0, 0, 0, 0, 0, 0, flags]


def _hub_graph():
    base = random_graph(4096, 40000, 11)
    rp, ci = np.asarray(base.row_ptr), np.asarray(base.col_idx)
    s = np.repeat(np.arange(4096, dtype=np.uint64), np.diff(rp))
    d = ci.astype(np.uint64)
    leaves = np.random.default_rng(12).permutation(4096)[:3000].astype(np.uint64)
    return csr_from_pairs(4097, np.concatenate([s, np.full(3000, 4096, dtype=np.uint64)]), np.concatenate([d, leaves]))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def _dense_graph():
    n, p = 700, 0.6  # (test_gpu_parity._dense_random_graph(700, 0.6, 700): DAG rows beyond 256 entries, the two-phase wide path)
    rng = np.random.default_rng(n)
    s, d = np.triu_indices(n, 1)
    keep = rng.random(s.size) < p
    return csr_from_pairs(n, s[keep].astype(np.uint64), d[keep].astype(np.uint64))


def _slow_references():
    g, dense = _hub_graph(), _dense_graph()
    osym = O.OGraph(g.row_ptr, g.col_idx)
    r5, r6 = R5.raw_sums(g), R6.raw_sums(g)
    hub = {"csr_sha256": csr_sha(g), "rectangle": O.rectangle(osym), "house": O.house(osym), "pentagon": O.pentagon(osym), "motif4": O.motif4(osym),
           "sgl5": [r5[k] for k in R5.RAW], "sgl6": [r6[k] for k in R6.RAW]}
    return {"hub": hub, "dense700": {"csr_sha256": csr_sha(dense), "clique4": O.clique(O.orient(O.OGraph(dense.row_ptr, dense.col_idx)), 4)}}


@pytest.fixture(scope="module")
def hub():
    """graph (a) and what every family must count on it, computed once"""
    g = _hub_graph()
    assert int(np.diff(g.row_ptr).max()) >= 3000
    with open(RECORDED) as f:
        want = json.load(f)["hub"]
    assert want.pop("csr_sha256") == csr_sha(g), "the recorded counts belong to another graph"
    osym = O.OGraph(g.row_ptr, g.col_idx)
    odag = O.orient(osym)
    sup = RT.supports(g)
    src = np.repeat(np.arange(g.V(), dtype=np.int64), np.diff(np.asarray(g.row_ptr)))
    kt_sup, kt_n = RT.ktruss(g, TRUSS_K)[:2]
    want.update({
        "tc": O.tc(odag), "diamond": O.diamond(osym), "clique4": O.clique(odag, 4), "clique5": O.clique(odag, 5), "motif3": O.motif3(osym),
        "sup": sup, "tv": (np.bincount(src, weights=sup.astype(np.float64), minlength=g.V()).astype(np.uint64) >> 1),
        "ktruss_n": kt_n, "ktruss_sup": kt_sup, "tau": RT.trussness(g)[0],
        "tri": RL.list_ref(g),
    })
    return g, want


def _run_families(sym, dag, g, want, dev):
    """every family once; called twice per handle"""
    import torch

    assert TCSolver(dag) == want["tc"]
    for pat in ("diamond", "rectangle", "house", "pentagon"):
        assert SglSolver(sym, pat) == want[pat], pat
        assert SglSolver(sym, pat, tune=_t6(GLOBAL_MAPS)) == want[pat], pat
    assert SglSolver(sym, "rectangle", tune=_t6(SGL_FLAT)) == want["rectangle"]
    assert CliqueSolver(dag, 4) == want["clique4"] and CliqueSolver(dag, 5) == want["clique5"]
    assert MotifSolver(sym, 3, formula=True) == want["motif3"]
    assert MotifSolverE(sym, 3) == want["motif3"]
    assert MotifSolverE(sym, 3, tune=_t6(NO_CLASSES)) == want["motif3"]  # (the hub row through the general kernel: SPLIT chunks, borrowed bitmaps)
    assert MotifSolver(sym, 4) == want["motif4"]
    assert sgl5_raw(sym, "all") == want["sgl5"]
    assert sgl6_raw(sym, "all") == want["sgl6"]
    total, tv, sup = tc_local(sym)
    assert total == want["tc"] and np.array_equal(tv, want["tv"]) and np.array_equal(sup, want["sup"])
    n, ksup, _ = ktruss(sym, TRUSS_K)
    assert n == want["ktruss_n"] and np.array_equal(ksup, want["ktruss_sup"])
    tau, kmax, _ = truss_decompose(sym)
    assert np.array_equal(tau, want["tau"]) and kmax == int(want["tau"].max())
    total, tri = tc_list(sym)
    assert total == want["tc"] and np.array_equal(RL.sort_rows(tri), want["tri"])
    # the diamond support partial / finish pair, one rank
    n = diamond_support_size(sym, 1)
    buf = torch.full((n,), 7, dtype=torch.int32, device=f"cuda:{dev}")
    diamond_support_partial(sym, buf.data_ptr(), n)
    assert diamond_support_finish(sym, buf.data_ptr(), n) == want["diamond"]
    # both ranks of a world of two on the one handle (the ShareOrders of its tables)
    assert sum(TCSolver(dag, rank=r, world=2) for r in range(2)) == want["tc"]
    assert sum(CliqueSolver(dag, 4, rank=r, world=2) for r in range(2)) == want["clique4"]


def test_uploaded_handle_returns_every_block(dev, hub):
    g, want = hub
    before = dev_live_blocks()
    sym = g.to_device(dev)
    dag = sym.orient()
    assert dev_live_blocks() > before
    for _ in range(2):
        _run_families(sym, dag, g, want, dev)
    dag.free()
    sym.free()
    assert dev_live_blocks() == before


def test_adopted_handle_returns_every_block_and_leaves_col_idx_alone(dev, hub):
    import torch

    g, want = hub
    rp = torch.from_numpy(np.asarray(g.row_ptr).astype(np.int64)).to(f"cuda:{dev}")
    ci = torch.from_numpy(np.asarray(g.col_idx).astype(np.int32)).to(f"cuda:{dev}")
    before = dev_live_blocks()
    sym = DeviceGraph.from_device_ptrs(g.V(), g.E(), rp.data_ptr(), ci.data_ptr(), dev, keepalive=(rp, ci))
    dag = sym.orient()
    for _ in range(2):
        _run_families(sym, dag, g, want, dev)
    dag.free()
    sym.free()
    assert dev_live_blocks() == before
    assert np.array_equal(ci.cpu().numpy(), np.asarray(g.col_idx).astype(np.int32))  # the borrowed array was not freed or written


def test_wide_clique_plan_and_its_rounds_return_every_block(dev):
    g = _dense_graph()
    with open(RECORDED) as f:
        rec = json.load(f)["dense700"]
    assert rec["csr_sha256"] == csr_sha(g), "the recorded count belongs to another graph"
    want4 = rec["clique4"]
    assert int(np.diff(O.orient(O.OGraph(g.row_ptr, g.col_idx)).row_ptr).max()) > 256
    before = dev_live_blocks()
    sym = g.to_device(dev)
    dag = sym.orient()
    for _ in range(2):
        assert CliqueSolver(dag, 4) == want4
        assert sum(CliqueSolver(dag, 4, rank=r, world=2) for r in range(2)) == want4
    dev_option("GM_WIDE_ARENA_MB", "4")  # (plans are cached per (rank, world, policy): a fresh share builds its plan in several rounds)
    try:
        for _ in range(2):
            assert sum(CliqueSolver(dag, 4, rank=r, world=2, policy=1) for r in range(2)) == want4
    finally:
        dev_option("GM_WIDE_ARENA_MB", None)
    dag.free()
    sym.free()
    assert dev_live_blocks() == before


if __name__ == "__main__":  # record the slow references of graph (a) again
    with open(RECORDED, "w") as f:
        json.dump(_slow_references(), f, indent=1)
        f.write("\n")
