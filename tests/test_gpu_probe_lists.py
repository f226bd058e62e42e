"""The list-streaming kernels on the probe graphs of tests/probe_graphs.py: one streamed list of a known length against one host row, the
matches at known positions, non-members everywhere else (see that module; tests/test_probe_graphs_host.py confirms every expected value
against the CPU oracle).  Every comparison is exact.

  * triangle count (tch_kernel, gm_tch.hip) and 3-clique on every graph: default, as numbered, the global fallback lookup, the sorted-copy
    kernel, parts, rank shares, always renumbered (GM_TOPO_MIN_ROW=0), both stages (GM_TCT_SPLIT_ALWAYS=1).  A total cannot say which list
    went wrong, so the single-list graphs also run as SLICES -- one match pattern, one class of lengths, same hubs and rows: the id of a
    failing test names graph, pattern and class (`s1024:last:long`), family (`salt`, `surplus`) or batch length (`batch1024_128`);
  * local counts (gm_sup.hip): every entry's support and every vertex's triangles; a failure prints the gadget (L, A, pattern) of the
    first wrong entry; with the key stream forced on and off and without match masks;
  * listing (gm_list.hip): the set of triples, and windows of 1, 64 and 65 triangles that tile the list;
  * diamond, 3-motif (formula and enumeration), and the 4-cliques of the `k4` graph (the position set of gm_cbuild.hip)."""
import ctypes as C

import numpy as np
import pytest

import probe_graphs as PG
from common import MotifSolverE, check_rows, list_windows
from list_ref import sort_rows
from graphminer_amd import CliqueSolver, MotifSolver, SglSolver, TCSolver, _lib, tc_list
from graphminer_amd.solvers import _launch

pytestmark = pytest.mark.gpu
AS_NUMBERED, FALLBACK, SORTED_COPY, PARTS, PER_EDGE = 0x200, 0x800000, 0x4000000, 0x1000, 0x10000000
TC_TUNES = (0, AS_NUMBERED, AS_NUMBERED | FALLBACK, FALLBACK, SORTED_COPY, 0x20000000, PARTS)

BATCHES = [f"batch{M}_{ell}" for M in (1024, 2048) for ell in PG.BATCH_ELLS]
GRAPHS = ["s1024", "s2048", "k4", "salt", "surplus"] + BATCHES
SLICES = [f"{n}:{pat}:{cls}" for n in PG.SINGLE for pat in PG.SLICE_PATTERNS for cls in PG.SLICE_CLASSES]


def probe(name: str) -> PG.Probe:
    if name.startswith("batch"):
        M, ell = name[5:].split("_")
        return PG.batch(int(M), int(ell))
    if ":" in name:
        return PG.single(*name.split(":"))
    return {"s1024": lambda: PG.single("s1024"), "s2048": lambda: PG.single("s2048"), "k4": PG.k4, "salt": PG.salt, "surplus": PG.surplus}[name]()


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


class Handles:
    def __init__(self, name, dev):
        self.name, self.p = name, probe(name)
        self.sym = self.p.graph.to_device(dev)
        self.dag = self.sym.orient()

    def free(self):
        self.dag.free()
        self.sym.free()


@pytest.fixture(scope="module")
def h(request, dev):
    """the probe graph named by the (indirect) parameter, uploaded and oriented once for the module"""
    x = Handles(request.param, dev)
    yield x
    x.free()


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def tc_every_way(label, dag, want):
    for t in TC_TUNES:
        check(f"{label} TCSolver tune[6]={t:#x}", TCSolver(dag, tune=t6(t)), want)
        check(f"{label} CliqueSolver 3 tune[6]={t:#x}", CliqueSolver(dag, 3, tune=t6(t)), want)
    for t in (0, AS_NUMBERED):
        check(f"{label} rank shares of 3, tune[6]={t:#x}", sum(TCSolver(dag, rank=r, world=3, tune=t6(t)) for r in range(3)), want)
        check(f"{label} 3-clique rank shares of 3, tune[6]={t:#x}", sum(CliqueSolver(dag, 3, rank=r, world=3, tune=t6(t)) for r in range(3)), want)


def big_stage(name):
    return name.startswith(("s2048", "batch2048")) or name == "k4"


@pytest.mark.parametrize("h", GRAPHS + SLICES, indirect=True)
def test_tc(h, dev, devopt):
    """the module's handle with the default options; then fresh handles (the options are read when a handle's tables are built):
    GM_TOPO_MIN_ROW=0 -- always on the topological copy, the trimmed tails of L keys -- and, where rows of more than 1024 entries host,
    GM_TCT_SPLIT_ALWAYS=1 -- those hosts on the 2048-entry kernel, the others on the 1024-entry one -- with and without it"""
    p = h.p
    tc_every_way(h.name, h.dag, p.tri_total)
    variants = [{"GM_TOPO_MIN_ROW": "0"}]
    if big_stage(h.name):
        variants += [{"GM_TCT_SPLIT_ALWAYS": "1"}, {"GM_TCT_SPLIT_ALWAYS": "1", "GM_TOPO_MIN_ROW": "0"}]
    for opts in variants:
        devopt(None)
        for k, v in opts.items():
            devopt(k, v)
        with p.graph.to_device(dev) as sym:
            dag = sym.orient()
            tc_every_way(f"{h.name} {opts}", dag, p.tri_total)
            dag.free()


# ---- localisation: supports and triangles per vertex -----------------------------------------------------------------------------------
def local_check(label, p, sym, tune, want_tv, want_sup):
    """gm_tc_local into device buffers, compared there (the arrays of the large graphs stay on the device); the first wrong entries and
    vertices are brought back and named by their gadget"""
    import torch

    la, total = _launch(0, 1, 0, tune=tune), C.c_uint64(0)
    tv = torch.empty(sym.nv, dtype=torch.int64, device=want_tv.device)
    sup = torch.empty(max(sym.ne, 1), dtype=torch.int32, device=want_tv.device)
    _lib.check(_lib.load().gm_tc_local(sym.handle, C.byref(la), tv.data_ptr(), sup.data_ptr(), C.byref(total), None), "gm_tc_local")
    bad_e = torch.nonzero(sup[:sym.ne] != want_sup)[:4, 0].cpu().tolist()
    bad_v = torch.nonzero(tv != want_tv)[:4, 0].cpu().tolist()
    msg = [f"entry {e} of {p.gadget_of_entry(e)}: support {int(sup[e])} want {int(want_sup[e])}" for e in bad_e]
    msg += [f"vertex {x} of {p.gadget_of_vertex(x)}: triangles {int(tv[x])} want {int(want_tv[x])}" for x in bad_v]
    print(f"{label}: total {total.value} want {p.tri_total}; wrong: {msg or 'none'}", flush=True)
    assert not msg and int(total.value) == p.tri_total, (label, msg)


def local_expected(p, dev):
    import torch

    return (torch.from_numpy(p.vertex_triangles().view(np.int64)).to(f"cuda:{dev}"), torch.from_numpy(p.supports().view(np.int32)).to(f"cuda:{dev}"))


@pytest.mark.parametrize("h", GRAPHS, indirect=True)
def test_local_counts(h, dev, devopt):
    """the module's handle, then fresh ones with the supports forced onto the task lists, onto the key stream, and with one atomic per
    streamed edge instead of match masks (the masks belong to the task lists)"""
    p = h.p
    want = local_expected(p, dev)
    for t in (0, AS_NUMBERED, FALLBACK):
        local_check(f"{h.name} tc_local tune[6]={t:#x}", p, h.sym, t6(t), *want)
    for opts in ({"GM_SUP_STREAM": "0"}, {"GM_SUP_STREAM": "1"}, {"GM_SUP_STREAM": "0", "GM_SUP_NO_MASKS": "1"}):
        devopt(None)
        for k, v in opts.items():
            devopt(k, v)
        with p.graph.to_device(dev) as sym:
            for t in (0, AS_NUMBERED):
                local_check(f"{h.name} {opts} tc_local tune[6]={t:#x}", p, sym, t6(t), *want)


# ---- listing -------------------------------------------------------------------------------------------------------------------------------
def rows_check(label, p, got, want):
    """common.check_rows, after the gadget of the first differing row"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and (got != want).any():
        i = int(np.flatnonzero((got != want).any(axis=1))[0])
        print(f"{label}: first wrong row {i}, of {p.gadget_of_vertex(int(want[i][0]))}", flush=True)
    check_rows(label, got, want)


@pytest.mark.parametrize("h", GRAPHS, indirect=True)
def test_list(h):
    p = h.p
    for t in (0, AS_NUMBERED):
        total, tri = tc_list(h.sym, tune=t6(t))
        check(f"{h.name} tc_list tune[6]={t:#x} total", total, p.tri_total)
        rows_check(f"{h.name} tc_list tune[6]={t:#x} sorted rows", p, sort_rows(tri), p.triangles)
    total, full = tc_list(h.sym)
    for size in (1, 64, 65):  # every size tiles the WHOLE list, one launch per window (the longest list, s2048's, has 2520 triangles)
        rows_check(f"{h.name} windows of {size}", p, list_windows(h.sym, size, total), full)


# ---- the other solvers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", GRAPHS, indirect=True)
def test_diamond_and_motif(h):
    p = h.p
    want = p.diamonds()
    if h.name in ("s1024", "s2048", "k4", "surplus") or h.name.startswith("batch"):
        assert want > 0  # (the tile-edge gadgets have supports >= 2)
    for t in (0, PER_EDGE, FALLBACK):
        check(f"{h.name} diamond tune[6]={t:#x}", SglSolver(h.sym, "diamond", tune=t6(t)), want)
    check(f"{h.name} 3-motif, enumerated", MotifSolverE(h.sym, 3), [p.wedges(), p.tri_total])
    check(f"{h.name} 3-motif", MotifSolver(h.sym, 3), [p.wedges(), p.tri_total])


@pytest.mark.parametrize("h", ["k4", "s1024", "salt"], indirect=True)
def test_clique4(h):
    want = len(h.p.cliques4)
    check("expected 4-cliques", want, 10 if h.name == "k4" else 0)
    for t in (0, AS_NUMBERED, 0x40000, FALLBACK):
        check(f"{h.name} CliqueSolver 4 tune[6]={t:#x}", CliqueSolver(h.dag, 4, tune=t6(t)), want)
    check(f"{h.name} 4-clique rank shares of 3", sum(CliqueSolver(h.dag, 4, rank=r, world=3) for r in range(3)), want)
