"""Python mirror of the reference's four solver entry points over the C ABI.

    void TCSolver    (Graph&, uint64_t& total, int n_gpu, int chunk)            src/triangle/main.cc:5
    void SglSolver   (Graph&, Pattern&, uint64_t& total, int n_dev, int chunk)  src/sgl/main.cc:7
    void CliqueSolver(Graph&, int k, uint64_t& total, int, int)                 src/clique/main.cc:6
    void MotifSolver (Graph&, int k, std::vector<uint64_t>&, int, int)          src/motif/main.cc:7

Same names, argument meaning and error behaviour; results are returned instead of written
through references. Each call goes straight to the HIP library -- no host compute path.
Multi-GPU: one process per GPU; pass ``rank``/``world`` (the task-chunk share) and sum the
returned per-rank counts with one all-reduce (see graphminer_amd.dist).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _lib
from ._lib import GM_ERR_UNSUPPORTED, gm_launch, gm_stats
from .graph import DeviceGraph

# include/pattern.hh:4-15
num_possible_patterns = [0, 1, 1, 2, 6, 21, 112, 853, 11117, 261080]


@dataclass
class Stats:
    kernel_ms: float = 0.0
    tasks: int = 0
    chunks: int = 0
    grid: int = 0
    block: int = 0


def _launch(rank=0, world=1, chunk=0, policy=_lib.GM_PART_ROUND_ROBIN, stream=0, d_counts=0, tune=None):
    la = gm_launch()
    la.stream = stream or None
    la.rank, la.world, la.policy, la.chunk = rank, world, policy, chunk
    la.d_counts = d_counts or None
    for i, t in enumerate(tune or []):
        la.tune[i] = int(t)
    return la


def _stats(st: gm_stats) -> Stats:
    return Stats(st.kernel_ms, int(st.tasks), int(st.chunks), int(st.grid), int(st.block))


def TCSolver(g: DeviceGraph, *, rank=0, world=1, chunk=0, return_stats=False, **kw):
    """Triangle count of an ORIENTED graph: sum over DAG edges (u,v) of |N+(u) ^ N+(v)|."""
    lib = _lib.load()
    la, st, total = _launch(rank, world, chunk, **kw), gm_stats(), C.c_uint64(0)
    _lib.check(lib.gm_tc(g.handle, C.byref(la), C.byref(total), C.byref(st)), "gm_tc")
    return (int(total.value), _stats(st)) if return_stats else int(total.value)


def tc_core_info(g: DeviceGraph) -> dict:
    """the hub corner the triangle count of this ORIENTED graph takes on the matrix cores (gm_tc_core_info; after a first TCSolver call)"""
    info = (C.c_int64 * 4)()
    _lib.check(_lib.load().gm_tc_core_info(g.handle, info), "gm_tc_core_info")
    return {"h": int(info[0]), "edges": int(info[1]), "blocks": int(info[2]), "core_h": int(info[3])}


def tc_pairs_info(g: DeviceGraph) -> dict:
    """the block pairs of the hub corner the product takes on this ORIENTED graph (gm_tc_pairs_info; after a first TCSolver call)"""
    info = (C.c_int64 * 6)()
    _lib.check(_lib.load().gm_tc_pairs_info(g.handle, info), "gm_tc_pairs_info")
    return {"region": int(info[0]), "pairs": int(info[1]), "pairs_possible": int(info[2]), "edges": int(info[3]),
            "keys_moved": int(info[4]), "R": int(info[5])}


def tc_pair_rule(keys, nb: int, region: int, R: int):
    """the rule that chooses the pairs (gm_tc_pair_rule; host only): keys = nb * nb uint32 cells, row IB, column JB -> nb x nb bool array"""
    import numpy as np

    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    if keys.size != nb * nb:
        raise ValueError("tc_pair_rule: keys must hold nb * nb cells")
    bits = np.zeros(max((nb * nb + 31) // 32, 1), dtype=np.uint32)
    n = _lib.load().gm_tc_pair_rule(keys.ctypes.data, nb, region, R, bits.ctypes.data)
    if n < 0:
        raise ValueError("gm_tc_pair_rule: invalid arguments")
    sel = ((bits[np.arange(nb * nb) >> 5] >> (np.arange(nb * nb, dtype=np.uint32) & 31)) & 1).astype(bool).reshape(nb, nb)
    assert int(sel.sum()) == n
    return sel


def SglSolver(g: DeviceGraph, pattern: str, *, rank=0, world=1, chunk=0, return_stats=False, **kw):
    """Edge-induced subgraph listing on the SYMMETRIC graph; pattern by name (include/pattern.hh:62-78).

    Unknown / unimplemented names behave like the reference's omp solver: "Not implemented",
    total 0 (src/sgl/omp_base.cc:51-53)."""
    lib = _lib.load()
    la, st, total = _launch(rank, world, chunk, **kw), gm_stats(), C.c_uint64(0)
    rc = lib.gm_sgl(g.handle, pattern.encode(), C.byref(la), C.byref(total), C.byref(st))
    if rc == GM_ERR_UNSUPPORTED:
        print("Not implemented")
        return (0, Stats()) if return_stats else 0
    _lib.check(rc, "gm_sgl")
    return (int(total.value), _stats(st)) if return_stats else int(total.value)


def map_constants() -> dict:
    """the sizes at which the map kernels of the rectangle / the house change path (gm_constant "map_*"), by their short names"""
    out = {}
    for name in ("rect_block", "one_task_rows", "long_row", "tile_group", "mark_window", "house_ids", "house_wg_row", "house_wg_queue",
                 "heavy_centre", "house_fw16_rows", "lds_min_default", "house_walk_min_default"):
        v = C.c_int64(0)
        _lib.check(_lib.load().gm_constant(("map_" + name).encode(), C.byref(v)), "gm_constant")
        out[name] = int(v.value)
    return out


def map_plan_info(g: DeviceGraph, pattern: str) -> dict:
    """the plan SglSolver(g, "rectangle" | "house") built for its LDS maps (gm_map_plan_info; after a first such call on this handle), on
    the copy that call ran on: ranges "n", "cut", the numbers of tasks by kind, and for the rectangle the range bounds "rb" (n + 1 ids) and
    "lb" (log2 of every range's counter width)"""
    out = (C.c_int64 * 80)()
    _lib.check(_lib.load().gm_map_plan_info(g.handle, pattern.encode(), out, 80), "gm_map_plan_info")
    n = int(out[0])
    info = {"n": n, "cut": int(out[1]), "lds_range_tasks": int(out[2]), "lds_whole_tasks": int(out[3]), "front_tasks": int(out[4]),
            "heavy_tasks": int(out[5]), "light_tasks": int(out[6]), "front_heavy_tasks": int(out[7])}
    if pattern == "rectangle":
        info["rb"] = [int(out[8 + k]) for k in range(n + 1)]
        info["lb"] = [int(out[9 + n + k]) for k in range(n)]
    return info


def clique_plan_info(dag: DeviceGraph, as_numbered: bool = False) -> dict:
    """what the plan of a whole-graph CliqueSolver(dag, 4) holds (gm_clique_plan_info; after a first such call on this handle), on the copy
    that call ran on (as_numbered: a call with tune[6] & 0x200): "topo", "stage", "core_base" (-1: no core), "rounds", "wide" vertices and
    "wide_by_class" (matrix-core classes 0 / 1 / 2), build "tasks", "gather_units", "gather_items", and the "arena_chunks" / "arena_entries"
    of the rows beyond cb_max_deg that stay with the mining kernel (-1: that launch built no table)"""
    out = (C.c_int64 * 13)()
    _lib.check(_lib.load().gm_clique_plan_info(dag.handle, 1 if as_numbered else 0, out, 13), "gm_clique_plan_info")
    return {"topo": bool(out[0]), "stage": int(out[1]), "core_base": int(out[2]), "rounds": int(out[3]), "wide": int(out[4]),
            "wide_by_class": [int(out[5]), int(out[6]), int(out[7])], "tasks": int(out[8]), "gather_units": int(out[9]),
            "gather_items": int(out[10]), "arena_chunks": int(out[11]), "arena_entries": int(out[12])}


def CliqueSolver(g: DeviceGraph, k: int, *, rank=0, world=1, chunk=0, return_stats=False, **kw):
    """k-clique count on the ORIENTED graph."""
    lib = _lib.load()
    la, st, total = _launch(rank, world, chunk, **kw), gm_stats(), C.c_uint64(0)
    _lib.check(lib.gm_clique(g.handle, k, C.byref(la), C.byref(total), C.byref(st)), "gm_clique")
    return (int(total.value), _stats(st)) if return_stats else int(total.value)


def MotifSolver(g: DeviceGraph, k: int, *, rank=0, world=1, chunk=0, return_stats=False, formula=False, **kw):
    """k-motif counts on the SYMMETRIC graph; k=3 -> [wedges, triangles] (CPU order).

    formula=True is the reference's motif_omp_formula / motif_gpu_formula variant (enumerate triangles only,
    derive the wedges); with world > 1 its per-rank wedge value is a partial modulo 2**64 -- sum the ranks."""
    lib = _lib.load()
    n = num_possible_patterns[k] if 0 <= k < len(num_possible_patterns) else 0
    la, st = _launch(rank, world, chunk, **kw), gm_stats()
    out = (C.c_uint64 * max(n, 1))()
    fn = lib.gm_motif_formula if formula else lib.gm_motif
    _lib.check(fn(g.handle, k, C.byref(la), out, n, C.byref(st)), "gm_motif")
    res = [int(out[i]) for i in range(n)]
    return (res, _stats(st)) if return_stats else res


# ---- tailedtriangle / 4path / 3star on several ranks (include/graphminer_amd.h: gm_sgl4_*) ------------------------------------------------
def sgl4_partial(g: DeviceGraph, *, rank=0, world=1, chunk=0, return_stats=False, **kw):
    """this rank's share of the four per-edge sums the three patterns are closed forms of; sum the ranks' lists, then sgl4_finish"""
    la, st, raw = _launch(rank, world, chunk, **kw), gm_stats(), (C.c_uint64 * 4)()
    _lib.check(_lib.load().gm_sgl4_partial(g.handle, C.byref(la), None if la.d_counts else raw, C.byref(st)), "gm_sgl4_partial")
    res = [int(x) for x in raw]
    return (res, _stats(st)) if return_stats else res


def sgl4_finish(pattern: str, raw) -> int:
    """summed (mod 2**64) raw sums of every rank -> the count of `pattern`"""
    total = C.c_uint64(0)
    _lib.check(_lib.load().gm_sgl4_finish(pattern.encode(), (C.c_uint64 * 4)(*[int(x) & (2**64 - 1) for x in raw]), C.byref(total)), "gm_sgl4_finish")
    return int(total.value)


# ---- the six 5-vertex patterns as closed forms of eleven raw sums (include/graphminer_amd.h: gm_sgl5_*) ----------------------------------------
SGL5_PATTERNS = ("hourglass", "taileddiamond", "taileddiamond2", "closedhouse", "semihouse", "5path")
SGL5_RAW = ("T", "D", "W", "A", "B", "H", "S", "P", "K4", "R", "Q")


def sgl5_raw(g: DeviceGraph, pattern="all", *, chunk=0, return_stats=False, **kw):
    """the raw sums `pattern` needs -- one of SGL5_PATTERNS, "all", an iterable of names of SGL5_RAW, or a bit mask -- in the order of
    SGL5_RAW; the others are 0.  One GPU."""
    la, st, raw = _launch(0, 1, chunk, **kw), gm_stats(), (C.c_uint64 * len(SGL5_RAW))()
    if isinstance(pattern, str):
        _lib.check(_lib.load().gm_sgl5_raw(g.handle, pattern.encode(), C.byref(la), raw, C.byref(st)), "gm_sgl5_raw")
    else:
        need = pattern if isinstance(pattern, int) else sum(1 << SGL5_RAW.index(k) for k in set(pattern))
        _lib.check(_lib.load().gm_sgl5_raw_need(g.handle, need, C.byref(la), raw, C.byref(st)), "gm_sgl5_raw_need")
    res = [int(x) for x in raw]
    return (res, _stats(st)) if return_stats else res


def sgl5_finish(pattern: str, raw) -> int:
    """the eleven raw sums (mod 2**64) -> the count of `pattern`; host-only"""
    total = C.c_uint64(0)
    arr = (C.c_uint64 * len(SGL5_RAW))(*[int(x) & (2**64 - 1) for x in raw])
    _lib.check(_lib.load().gm_sgl5_finish(pattern.encode(), arr, C.byref(total)), "gm_sgl5_finish")
    return int(total.value)


# ---- 6path and dumbbell as closed forms of nine raw sums (include/graphminer_amd.h: gm_sgl6_*) ---------------------------------------------
SGL6_PATTERNS = ("6path", "dumbbell")
SGL6_RAW = ("X", "Y", "Z", "R", "D", "C5", "M", "B", "K4")


def sgl6_need(pattern: str) -> int:
    """the raw sums `pattern` (one of SGL6_PATTERNS, or "all") needs, as a bit mask over SGL6_RAW; host-only"""
    mask = C.c_uint32(0)
    _lib.check(_lib.load().gm_sgl6_need(pattern.encode(), C.byref(mask)), "gm_sgl6_need")
    return int(mask.value)


def sgl6_raw(g: DeviceGraph, need="all", *, chunk=0, return_stats=False, **kw):
    """the raw sums of `need` -- a pattern name, "all", an iterable of names of SGL6_RAW, or a bit mask -- in the order of SGL6_RAW; the
    others are 0.  One GPU."""
    if isinstance(need, str):
        need = sgl6_need(need)
    elif not isinstance(need, int):
        need = sum(1 << SGL6_RAW.index(k) for k in set(need))
    la, st, raw = _launch(0, 1, chunk, **kw), gm_stats(), (C.c_uint64 * len(SGL6_RAW))()
    _lib.check(_lib.load().gm_sgl6_raw(g.handle, need, C.byref(la), raw, C.byref(st)), "gm_sgl6_raw")
    res = [int(x) for x in raw]
    return (res, _stats(st)) if return_stats else res


def sgl6_finish(pattern: str, raw) -> int:
    """the nine raw sums (mod 2**64) -> the count of `pattern`; host-only"""
    total = C.c_uint64(0)
    arr = (C.c_uint64 * len(SGL6_RAW))(*[int(x) & (2**64 - 1) for x in raw])
    _lib.check(_lib.load().gm_sgl6_finish(pattern.encode(), arr, C.byref(total)), "gm_sgl6_finish")
    return int(total.value)


def sgl6(g: DeviceGraph, pattern: str, *, chunk=0, return_stats=False, **kw):
    """the count of "6path" or "dumbbell" on the SYMMETRIC graph (SglSolver keeps answering "Not implemented" for the two names).  One GPU."""
    la, st, total = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0)
    _lib.check(_lib.load().gm_sgl6(g.handle, pattern.encode(), C.byref(la), C.byref(total), C.byref(st)), "gm_sgl6")
    return (int(total.value), _stats(st)) if return_stats else int(total.value)


# ---- diamond on several ranks with the one-GPU algorithm (include/graphminer_amd.h: gm_diamond_support_*) ------------------------------
def diamond_support_size(g: DeviceGraph, world: int = 1) -> int:
    """uint32 entries of a rank's support array: |E+| of the oriented copy, padded so that every rank's reduce-scatter slice is equal"""
    n = C.c_int64(0)
    _lib.check(_lib.load().gm_diamond_support_size(g.handle, world, C.byref(n)), "gm_diamond_support_size")
    return int(n.value)


def diamond_support_partial(g: DeviceGraph, d_support: int, n_entries: int, *, rank=0, world=1, chunk=0, return_stats=False, **kw):
    """this rank's share of the triangle pass adds its increments into the caller's DEVICE buffer (zeroed by the call); asynchronous on
    `stream` when `d_counts` is given"""
    la, st = _launch(rank, world, chunk, **kw), gm_stats()
    _lib.check(_lib.load().gm_diamond_support_partial(g.handle, C.byref(la), d_support, n_entries, C.byref(st)), "gm_diamond_support_partial")
    return _stats(st) if return_stats else None


def diamond_support_finish(g: DeviceGraph, d_support: int, count: int, *, return_stats=False, **kw):
    """sum C(t, 2) over `count` reduced support entries at `d_support` (a rank's slice) -> this rank's part of the diamond count"""
    la, st, total = _launch(0, 1, 0, **kw), gm_stats(), C.c_uint64(0)
    _lib.check(_lib.load().gm_diamond_support_finish(g.handle, C.byref(la), d_support, count, None if la.d_counts else C.byref(total), C.byref(st)),
               "gm_diamond_support_finish")
    return (int(total.value), _stats(st)) if return_stats else int(total.value)


# ---- local counts and the k-truss (include/graphminer_amd.h: gm_tc_local / gm_ktruss / gm_truss_decompose) -----------------------------
TRUSS_REMOVED = _lib.GM_TRUSS_REMOVED


def _dev_array(g: DeviceGraph, n: int, dtype):
    """a device buffer of n elements on the graph's GPU: a torch tensor (uint32 / uint64 travel as int32 / int64 of the same bytes)"""
    import torch

    return torch.empty(max(int(n), 1), dtype=dtype, device=torch.device("cuda", g.device))


def _to_numpy(t, n: int, dtype):
    return t[:n].cpu().numpy().view(dtype)


def tc_local(g: DeviceGraph, *, vertex=True, entries=True, chunk=0, return_stats=False, **kw):
    """(total, T_v as np.uint64[nv] or None, edge supports as np.uint32[ne] or None) of a SYMMETRIC graph, in the caller's numbering and
    entry order: T_v the triangles at v, the support of entry (u, v) = |N(u) ^ N(v)|.  One GPU."""
    import torch

    la, st, total = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0)
    tv = _dev_array(g, g.nv, torch.int64) if vertex else None
    sup = _dev_array(g, g.ne, torch.int32) if entries else None
    _lib.check(_lib.load().gm_tc_local(g.handle, C.byref(la), tv.data_ptr() if vertex else None, sup.data_ptr() if entries else None,
                                       C.byref(total), C.byref(st)), "gm_tc_local")
    res = (int(total.value), _to_numpy(tv, g.nv, "uint64") if vertex else None, _to_numpy(sup, g.ne, "uint32") if entries else None)
    return (*res, _stats(st)) if return_stats else res


def ktruss(g: DeviceGraph, k: int, *, chunk=0, return_stats=False, **kw):
    """(undirected edges of the k-truss, per entry its edge's support inside the truss or TRUSS_REMOVED as np.uint32[ne], peeling rounds)"""
    import torch

    la, st, n, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_int32(0)
    sup = _dev_array(g, g.ne, torch.int32)
    _lib.check(_lib.load().gm_ktruss(g.handle, int(k), C.byref(la), sup.data_ptr(), C.byref(n), C.byref(rounds), C.byref(st)), "gm_ktruss")
    res = (int(n.value), _to_numpy(sup, g.ne, "uint32"), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


def truss_decompose(g: DeviceGraph, *, chunk=0, return_stats=False, **kw):
    """(trussness of every entry's edge as np.uint32[ne], the largest of them, peeling rounds)"""
    import torch

    la, st, kmax, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_int32(0), C.c_int32(0)
    tau = _dev_array(g, g.ne, torch.int32)
    _lib.check(_lib.load().gm_truss_decompose(g.handle, C.byref(la), tau.data_ptr(), C.byref(kmax), C.byref(rounds), C.byref(st)),
               "gm_truss_decompose")
    res = (_to_numpy(tau, g.ne, "uint32"), int(kmax.value), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


# ---- local k-clique counts (include/graphminer_amd.h: gm_clique_local) --------------------------------------------------------------------
def clique_local(g: DeviceGraph, k: int, *, vertex=True, entries=True, chunk=0, return_stats=False, **kw):
    """(total, K_v as np.uint64[nv] or None, K_uv per entry as np.uint64[ne] or None) of a SYMMETRIC graph, in the caller's numbering and
    entry order: K_v the k-cliques that contain v, K_uv the k-cliques that contain the edge of entry (u, v).  3 <= k <= 8.  One GPU."""
    import torch

    la, st, total = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0)
    kv = _dev_array(g, g.nv, torch.int64) if vertex else None
    ke = _dev_array(g, g.ne, torch.int64) if entries else None
    _lib.check(_lib.load().gm_clique_local(g.handle, int(k), C.byref(la), kv.data_ptr() if vertex else None, ke.data_ptr() if entries else None,
                                           C.byref(total), C.byref(st)), "gm_clique_local")
    res = (int(total.value), _to_numpy(kv, g.nv, "uint64") if vertex else None, _to_numpy(ke, g.ne, "uint64") if entries else None)
    return (*res, _stats(st)) if return_stats else res


# ---- k-clique cores (include/graphminer_amd.h: gm_clique_kcore / gm_clique_core_decompose) -----------------------------------------------
CORE_REMOVED = _lib.GM_CORE_REMOVED


def clique_kcore(g: DeviceGraph, k: int, c: int, *, chunk=0, return_stats=False, **kw):
    """(vertices of the (k, c)-core, its k-cliques, per vertex K_v inside the core or CORE_REMOVED as np.uint64[nv], peeling rounds) of a
    SYMMETRIC graph: the largest vertex set in which every vertex lies in >= c k-cliques OF THAT SET.  2 <= k <= 8.  One GPU."""
    import torch

    la, st, nvert, ncl, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
    cnt = _dev_array(g, g.nv, torch.int64)
    _lib.check(_lib.load().gm_clique_kcore(g.handle, int(k), int(c), C.byref(la), cnt.data_ptr(), C.byref(nvert), C.byref(ncl), C.byref(rounds),
                                           C.byref(st)), "gm_clique_kcore")
    res = (int(nvert.value), int(ncl.value), _to_numpy(cnt, g.nv, "uint64"), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


def clique_core_decompose(g: DeviceGraph, k: int, *, chunk=0, return_stats=False, **kw):
    """(k-clique core number of every vertex as np.uint64[nv], the 1-based round whose frontier held it as np.uint32[nv], the largest core
    number, peeling rounds, (round, vertices, cliques) of the densest of the rounds' states) of a SYMMETRIC graph.  2 <= k <= 8.  One GPU."""
    import torch

    la, st, cmax, rounds, dense = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_int32(0), _lib.gm_core_dense()
    core, rnd = _dev_array(g, g.nv, torch.int64), _dev_array(g, g.nv, torch.int32)
    _lib.check(_lib.load().gm_clique_core_decompose(g.handle, int(k), C.byref(la), core.data_ptr(), rnd.data_ptr(), C.byref(cmax), C.byref(rounds),
                                                    C.byref(dense), C.byref(st)), "gm_clique_core_decompose")
    res = (_to_numpy(core, g.nv, "uint64"), _to_numpy(rnd, g.nv, "uint32"), int(cmax.value), int(rounds.value),
           (int(dense.round), int(dense.vertices), int(dense.cliques)))
    return (*res, _stats(st)) if return_stats else res


# ---- k-clique trusses (include/graphminer_amd.h: gm_clique_ktruss / gm_clique_truss_decompose) -------------------------------------------
def clique_ktruss(g: DeviceGraph, k: int, c: int, *, chunk=0, return_stats=False, **kw):
    """(undirected edges of the (k, c)-truss, its k-cliques, per entry K_e inside the truss or CORE_REMOVED as np.uint64[ne], peeling rounds)
    of a SYMMETRIC graph: the largest edge set in which every edge lies in >= c k-cliques OF THAT SET.  3 <= k <= 8.  One GPU."""
    import torch

    la, st, nedges, ncl, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
    cnt = _dev_array(g, g.ne, torch.int64)
    _lib.check(_lib.load().gm_clique_ktruss(g.handle, int(k), int(c), C.byref(la), cnt.data_ptr(), C.byref(nedges), C.byref(ncl), C.byref(rounds),
                                            C.byref(st)), "gm_clique_ktruss")
    res = (int(nedges.value), int(ncl.value), _to_numpy(cnt, g.ne, "uint64"), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


def clique_truss_decompose(g: DeviceGraph, k: int, *, chunk=0, return_stats=False, **kw):
    """(k-clique trussness of every entry's edge as np.uint64[ne], the 1-based round whose frontier held it as np.uint32[ne], the largest
    trussness, peeling rounds) of a SYMMETRIC graph; at k = 3 the ordinary trussness - 2.  3 <= k <= 8.  One GPU."""
    import torch

    la, st, cmax, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_int32(0)
    theta, rnd = _dev_array(g, g.ne, torch.int64), _dev_array(g, g.ne, torch.int32)
    _lib.check(_lib.load().gm_clique_truss_decompose(g.handle, int(k), C.byref(la), theta.data_ptr(), rnd.data_ptr(), C.byref(cmax), C.byref(rounds),
                                                     C.byref(st)), "gm_clique_truss_decompose")
    res = (_to_numpy(theta, g.ne, "uint64"), _to_numpy(rnd, g.ne, "uint32"), int(cmax.value), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


# ---- triangle nuclei (include/graphminer_amd.h: gm_tri_clique4_local / gm_nucleus34 / gm_nucleus34_decompose) ----------------------------
def _triangle_total(g: DeviceGraph, la) -> int:
    """T of a count-only gm_tc_list: the length of every per-triangle array, whose index is the row of tc_list's listing"""
    total = C.c_uint64(0)
    _lib.check(_lib.load().gm_tc_list(g.handle, C.byref(la), 0, 0, None, C.byref(total), None, None), "gm_tc_list")
    return int(total.value)


def tri_clique4_local(g: DeviceGraph, *, chunk=0, return_stats=False, **kw):
    """(the 4-cliques of a SYMMETRIC graph, K4(t) as np.uint32[T]): the 4-cliques that contain triangle t, t = the row of tc_list(g).
    One GPU."""
    import torch

    la, st, total = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0)
    T = _triangle_total(g, la)
    cnt = _dev_array(g, T, torch.int32)
    _lib.check(_lib.load().gm_tri_clique4_local(g.handle, C.byref(la), T, cnt.data_ptr(), C.byref(total), C.byref(st)), "gm_tri_clique4_local")
    res = (int(total.value), _to_numpy(cnt, T, "uint32"))
    return (*res, _stats(st)) if return_stats else res


def nucleus34(g: DeviceGraph, c: int, *, chunk=0, return_stats=False, **kw):
    """(triangles of the (3,4)-c-nucleus set, its 4-cliques, per triangle its count inside the set or TRUSS_REMOVED as np.uint32[T], peeling
    rounds) of a SYMMETRIC graph: the largest triangle set in which every triangle lies in >= c 4-cliques all of whose triangles are IN THAT
    SET; t = the row of tc_list(g).  One GPU."""
    import torch

    la, st, ntri, ncl, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
    T = _triangle_total(g, la)
    cnt = _dev_array(g, T, torch.int32)
    _lib.check(_lib.load().gm_nucleus34(g.handle, int(c), C.byref(la), T, cnt.data_ptr(), C.byref(ntri), C.byref(ncl), C.byref(rounds), C.byref(st)),
               "gm_nucleus34")
    res = (int(ntri.value), int(ncl.value), _to_numpy(cnt, T, "uint32"), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


def nucleus34_decompose(g: DeviceGraph, *, chunk=0, return_stats=False, **kw):
    """(theta of every triangle as np.uint32[T], the 1-based round whose frontier held it as np.uint32[T], the largest theta, peeling rounds)
    of a SYMMETRIC graph: theta(t) = the largest c whose (3,4)-c-nucleus set holds t; t = the row of tc_list(g).  One GPU."""
    import torch

    la, st, cmax, rounds = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint32(0), C.c_int32(0)
    T = _triangle_total(g, la)
    theta, rnd = _dev_array(g, T, torch.int32), _dev_array(g, T, torch.int32)
    _lib.check(_lib.load().gm_nucleus34_decompose(g.handle, C.byref(la), T, theta.data_ptr(), rnd.data_ptr(), C.byref(cmax), C.byref(rounds),
                                                  C.byref(st)), "gm_nucleus34_decompose")
    res = (_to_numpy(theta, T, "uint32"), _to_numpy(rnd, T, "uint32"), int(cmax.value), int(rounds.value))
    return (*res, _stats(st)) if return_stats else res


# ---- local 4-cycle counts (include/graphminer_amd.h: gm_rect_local) -----------------------------------------------------------------------
def rect_local(g: DeviceGraph, *, vertex=True, entries=True, chunk=0, return_stats=False, **kw):
    """(total, R_v as np.uint64[nv] or None, R_uv per entry as np.uint64[ne] or None) of a SYMMETRIC graph, in the caller's numbering and
    entry order: R_v the 4-cycles that contain v, R_uv the 4-cycles that contain the edge of entry (u, v); total = the `rectangle` count.
    One GPU."""
    import torch

    la, st, total = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0)
    rv = _dev_array(g, g.nv, torch.int64) if vertex else None
    re = _dev_array(g, g.ne, torch.int64) if entries else None
    _lib.check(_lib.load().gm_rect_local(g.handle, C.byref(la), rv.data_ptr() if vertex else None, re.data_ptr() if entries else None,
                                         C.byref(total), C.byref(st)), "gm_rect_local")
    res = (int(total.value), _to_numpy(rv, g.nv, "uint64") if vertex else None, _to_numpy(re, g.ne, "uint64") if entries else None)
    return (*res, _stats(st)) if return_stats else res


# ---- local motif counts (include/graphminer_amd.h: gm_motif_local) ------------------------------------------------------------------------
def motif_local(g: DeviceGraph, k: int, *, orbits=True, chunk=0, return_stats=False, **kw):
    """(counts, orbits as np.uint64[n_orbits, nv] or None) of a SYMMETRIC graph: the graphlet-degree orbits of every vertex in the caller's
    numbering -- row o = orbit o in Przulj's numbering, 4 rows for k = 3, 15 for k = 4 -- and the list MotifSolver(g, k) returns, here
    from the column sums.  One GPU."""
    import torch

    k = int(k)
    la, st = _launch(0, 1, chunk, **kw), gm_stats()
    n = num_possible_patterns[k] if k in (3, 4) else 1
    no = 4 if k == 3 else 15
    out = (C.c_uint64 * n)()
    orb = _dev_array(g, no * g.nv, torch.int64) if orbits else None
    _lib.check(_lib.load().gm_motif_local(g.handle, k, C.byref(la), orb.data_ptr() if orbits else None, out, n, C.byref(st)), "gm_motif_local")
    res = ([int(x) for x in out], _to_numpy(orb, no * g.nv, "uint64").reshape(no, g.nv) if orbits else None)
    return (*res, _stats(st)) if return_stats else res


# ---- triangle listing (include/graphminer_amd.h: gm_tc_list) ------------------------------------------------------------------------------
def tc_list(g: DeviceGraph, *, first=0, cap=None, chunk=0, return_stats=False, **kw):
    """(total, triangles as np.int32[n_written, 3]) of a SYMMETRIC graph: rows a < b < c in the caller's numbering, every triangle once, in
    the handle's fixed listing order; the window is the `cap` triangles from index `first` (cap=None: all of them).  A count-only call sizes
    the buffer, a second call fills it; the stats add the two up.  One GPU."""
    import numpy as np
    import torch

    lib = _lib.load()
    la, st, total, written = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_uint64(0)
    _lib.check(lib.gm_tc_list(g.handle, C.byref(la), 0, 0, None, C.byref(total), None, C.byref(st)), "gm_tc_list")
    stats = _stats(st)
    first = int(first)
    n = max(int(total.value) - first, 0) if first >= 0 else 0
    n = n if cap is None else min(n, int(cap))
    tri = np.empty((0, 3), dtype=np.int32)
    if n > 0:
        buf = _dev_array(g, 3 * n, torch.int32)
        _lib.check(lib.gm_tc_list(g.handle, C.byref(la), first, n, buf.data_ptr(), C.byref(total), C.byref(written), C.byref(st)), "gm_tc_list")
        tri = _to_numpy(buf, 3 * int(written.value), "int32").reshape(-1, 3)
        stats.kernel_ms += st.kernel_ms
    return (int(total.value), tri, stats) if return_stats else (int(total.value), tri)


# ---- k-clique listing (include/graphminer_amd.h: gm_clique_list) --------------------------------------------------------------------------
def clique_list(g: DeviceGraph, k, *, first=0, cap=None, chunk=0, return_stats=False, **kw):
    """(k-cliques as np.int32[n_written, k], total) of a SYMMETRIC graph, 3 <= k <= 8: rows strictly ascending in the caller's numbering,
    every k-clique once, in the fixed listing order of (handle, k); the window is the `cap` rows from index `first` (cap=None: all of
    them).  A count-only call sizes the buffer, a second call fills it; the stats add the two up.  One GPU."""
    import numpy as np
    import torch

    lib = _lib.load()
    k = int(k)
    la, st, total, written = _launch(0, 1, chunk, **kw), gm_stats(), C.c_uint64(0), C.c_uint64(0)
    _lib.check(lib.gm_clique_list(g.handle, k, C.byref(la), 0, 0, None, C.byref(total), None, C.byref(st)), "gm_clique_list")
    stats = _stats(st)
    first = int(first)
    n = max(int(total.value) - first, 0) if first >= 0 else 0
    n = n if cap is None else min(n, int(cap))
    rows = np.empty((0, k), dtype=np.int32)
    if n > 0:
        buf = _dev_array(g, k * n, torch.int32)
        _lib.check(lib.gm_clique_list(g.handle, k, C.byref(la), first, n, buf.data_ptr(), C.byref(total), C.byref(written), C.byref(st)),
                   "gm_clique_list")
        rows = _to_numpy(buf, k * int(written.value), "int32").reshape(-1, k)
        stats.kernel_ms += st.kernel_ms
    return (rows, int(total.value), stats) if return_stats else (rows, int(total.value))
