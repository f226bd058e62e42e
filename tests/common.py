"""Shared helpers for the test-suite."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
    GOLDEN = json.load(f)

# graphs with the FULL set of golden entries (the "partial" ones only hold selected, affordable entries)
GRAPH_NAMES = [k for k in GOLDEN if not k.startswith("_") and not GOLDEN[k].get("partial")]


def load_graph(name):
    """Return a graphminer_amd.Graph for a golden entry (fixture file or regenerated R-MAT)."""
    from graphminer_amd.graph import Graph
    from graphminer_amd.rmat import rmat_csr_numpy

    e = GOLDEN[name]
    if e["kind"] == "fixture":
        return Graph(os.path.join(ROOT, "tests", "fixtures", name, "graph"))
    return rmat_csr_numpy(e["scale"], e["edge_factor"], e["seed"])


def csr_sha(g):
    h = hashlib.sha256()
    h.update(np.asarray(g.row_ptr).astype("<i8").tobytes())
    h.update(np.asarray(g.col_idx).astype("<i4").tobytes())
    return h.hexdigest()


def random_graph(nv, ne_target, seed):
    """Small random symmetric simple graph (numpy)."""
    from graphminer_amd.rmat import csr_from_pairs

    rng = np.random.default_rng(seed)
    s = rng.integers(0, nv, ne_target).astype(np.uint64)
    d = rng.integers(0, nv, ne_target).astype(np.uint64)
    return csr_from_pairs(nv, s, d)


def renumbering(keydeg, descending=False):
    """new id of every vertex under get_relabeled: ids by (degree, old id), ascending (descending: the same order counted from the top)"""
    nv = len(keydeg)
    order = np.lexsort((np.arange(nv), keydeg))
    newid = np.empty(nv, dtype=np.int64)
    newid[order] = (nv - 1 - np.arange(nv)) if descending else np.arange(nv)
    return newid


def renumbered_expected(g, keydeg, descending):
    """numpy restatement of get_relabeled: ids by (degree, old id), rows ascending"""
    nv = g.V()
    newid = renumbering(keydeg, descending)
    src = np.repeat(np.arange(nv), np.diff(g.row_ptr))
    keys = np.sort((newid[src] << 32) | newid[g.col_idx.astype(np.int64)])
    rp = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys >> 32, minlength=nv), out=rp[1:])
    return rp, (keys & 0xFFFFFFFF).astype(np.int32)


def MotifSolverE(g, k, tune=None, **kw):
    """k-motif through the ENUMERATION kernels (tune[6] & 0x10000000: automine_3motif's loop nest, one bounded intersection per edge of
    the symmetric graph); gm_motif's default for k = 3 is the reference's formula solver (triangles of the DAG, wedges derived)"""
    from graphminer_amd import MotifSolver

    t = (list(tune or []) + [0] * 7)[:7]
    t[6] |= 0x10000000
    return MotifSolver(g, k, tune=t, **kw)


def check_rows(label, got, want):
    """two int32[n, 3] lists of triangles are the same rows in the same order; the first differing rows are printed before the assertion"""
    got, want = np.asarray(got), np.asarray(want)
    same = got.shape == want.shape and got.dtype == want.dtype
    bad = np.flatnonzero((got != want).any(axis=1)) if same else np.zeros(0, np.int64)
    print(f"{label}: got {got.shape} {got.dtype} want {want.shape} {want.dtype}, {bad.size} rows differ, first at {bad[:3].tolist()}: "
          f"got {got[bad[:3]].tolist() if same else '-'} want {want[bad[:3]].tolist() if same else '-'}", flush=True)
    assert same and bad.size == 0, label


def list_windows(sym, size, upto, sentinel=-7):
    """gm_tc_list in the windows [0, size), [size, 2 size), ... up to `upto` triangles: every call writes behind the one before it into one
    device buffer (pre-filled with the sentinel, with slack), which comes back once"""
    import ctypes as C

    import torch

    from graphminer_amd import _lib

    buf = torch.full((3 * upto + 64,), sentinel, dtype=torch.int32, device=f"cuda:{sym.device}")
    lib, written = _lib.load(), C.c_uint64(0)
    for f in range(0, upto, size):
        want = min(size, upto - f)
        rc = lib.gm_tc_list(sym.handle, None, f, want, buf.data_ptr() + 12 * f, None, C.byref(written), None)
        assert (rc, int(written.value)) == (_lib.GM_OK, want), (f, rc, written.value)
    host = buf.cpu().numpy()
    assert bool((host[3 * upto:] == sentinel).all()), "nothing behind the last window"
    return host[:3 * upto].reshape(-1, 3)


def gm_constant(name: str) -> int:
    """a kernel constant of the library by name (a host call, no GPU)"""
    import ctypes as C

    from graphminer_amd import _lib

    v = C.c_int64(0)
    _lib.check(_lib.load().gm_constant(name.encode(), C.byref(v)), "gm_constant")
    return int(v.value)


def sup_core_info(sym) -> dict:
    """the hub corner the support pass of this SYMMETRIC handle leaves to the matrix cores and to the wave-per-edge kernels of the weighted
    passes (gm_sup_core_info; after a first call that built the task lists): "vertices" (0: no corner) and the DAG "entries" inside it"""
    import ctypes as C

    from graphminer_amd import _lib

    info = (C.c_int64 * 4)()
    _lib.check(_lib.load().gm_sup_core_info(sym.handle, info), "gm_sup_core_info")
    return {"vertices": int(info[0]), "entries": int(info[1])}


KCL_ROW_CONSTANTS = {"regs2": "kcl_local_regs2_row", "split": "kcl_local_split_row", "regs8": "kcl_local_regs8_row", "regs12": "kcl_local_regs12_row",
                     "lds": "kcl_local_lds_row"}


def kcl_row_constants():
    """the row lengths at which gm_clique_local changes path, read from the library (gm_constant), under the short names the cells of
    tests/planted_cliques.py use; "lanes": the entries of a row whose sets take one word per lane of the wide kernel (64 lanes of 32
    bits; not exported)"""
    import ctypes as C

    from graphminer_amd import _lib

    lib, out = _lib.load(), {"lanes": 64 * 32}
    for key, name in KCL_ROW_CONSTANTS.items():
        v = C.c_int64(0)
        _lib.check(lib.gm_constant(name.encode(), C.byref(v)), "gm_constant")
        out[key] = int(v.value)
    return out


def clique_count_constants():
    """the constants that place a DAG row on its path of the global k-clique count (gm_constant: a host call, no GPU), by the names the
    cells of tests/planted_count_cells.py use"""
    import ctypes as C

    from graphminer_amd import _lib
    from planted_count_cells import CONST_NAMES

    lib, out = _lib.load(), {}
    for name in CONST_NAMES:
        v = C.c_int64(0)
        _lib.check(lib.gm_constant(name.encode(), C.byref(v)), "gm_constant")
        out[name] = int(v.value)
    return out
