"""Graded dense random graphs and a dense reference for the support family (test helper; imported by tests/test_dense_graded_host.py and the
GPU tests of the edge supports, the 5- and 6-vertex closed forms and the local counts).  Graphs are made with numpy alone; the one thing
taken from the package is the Graph CONTAINER -- no code of the library takes part in a value.

Why: the kernels of the support family read a support t(e) or a degree d(v) at an index they compute themselves.  On K_n every support is
n - 2 and every degree n - 1, so a read one entry off goes unnoticed; the sparse references (sgl5_ref.raw_sums: one row per (edge, common
neighbour) pair) cannot run on a dense graph of 1,500 vertices.  Here:

  graded(n, lo, seed)       weights w_i uniform in [lo, 1], edge ij kept with probability w_i w_j: dense enough for DAG rows beyond 1024 /
                            2048 entries, and degrees and supports differ from entry to entry
  dense_raw5 / dense_raw6   the raw sums of gm_sgl5_raw / gm_sgl6_raw from float64 products of the 0/1 adjacency matrix Adj (every entry
                            stays below 2^53: exact), finished in Python integers modulo 2^64.  With d the degrees, T = (Adj Adj) * Adj the
                            support on each edge, X = (T - 1) * Adj, T_v = row sums of T / 2:
                              A   = sum_{uv} x(uv) ((Adj * (d - 2)[None, :]) Adj)[u, v]
                              2 B = sum_{uv} x(uv) (X Adj + Adj X)[u, v]
                              T, D, W, H, S, P and sgl6's X, Y, M from t per edge, T_v and d;  Z, R from C(c, 2) of c = Adj Adj off the diagonal
                            K4, Q, C5 have no dense form here: asking for them raises
  dense_supports(g)         t per entry in the caller's entry order (uint32), T_v (uint64)
  mutants                   what a misplaced read would compute: "supports" rotates the supports of every DAG row (oracle.orient: the rows
                            the kernels walk) by one entry, "degrees" rotates the degree array by one vertex.  A cell can tell a misplaced
                            read iff the sums under the mutant differ from the true ones
  row_facts(g, stage_max)   DAG row lengths, the rows in (1024, stage_max] and beyond stage_max, and the distinct supports / degrees the
                            kernels read on the entries of those rows
  CELLS / cell / reference  the two graphs of the GPU tests and their reference values, computed once per process and left unchanged
"""
from __future__ import annotations

import functools

import numpy as np

import sgl5_ref as R5
import sgl6_ref as R6

M64 = 2**64
MAX_NV = 4096  # (2 B's matrix entries: nv * nv < 2^53 by far; the per-edge int64 terms: nv^3 < 2^63)
DENSE5 = ("T", "D", "W", "A", "B", "H", "S", "P")
DENSE6 = ("X", "Y", "Z", "R", "D", "M", "B")
# name: (n, lo, seed) -- tests/test_dense_graded_host.py asserts where each places its DAG rows.  "corner" is the stage cell with 1504 = 47 * 32
# vertices: the supports' hub corner is a whole number of 512-vertex chunks that starts at a word of the core bitmap's rows, so the
# library takes a corner of 1024 vertices only where nv - 1024 is a multiple of 32
CELLS = {"stage": (1500, 0.90, 1500), "beyond": (2200, 0.975, 2200), "corner": (1504, 0.90, 1504)}


def graded(n: int, lo: float, seed: int):
    import planted_squares as P

    rng = np.random.default_rng(seed)
    w = rng.uniform(lo, 1.0, n)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < w[iu] * w[ju]
    return P._graph(n, iu[keep], ju[keep])


def _csr(g):
    rp, ci = np.asarray(g.row_ptr).astype(np.int64), np.asarray(g.col_idx).astype(np.int64)
    return rp, ci, np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _adjacency(g):
    rp, ci, src = _csr(g)
    nv = len(rp) - 1
    assert nv <= MAX_NV, "the dense forms are for graphs of a few thousand vertices"
    adj = np.zeros((nv, nv), np.float64)
    adj[src, ci] = 1.0
    assert bool((adj == adj.T).all()) and not adj.diagonal().any(), "a symmetric graph without loops"
    return adj


def _rotated_supports(g, t):
    """the support matrix a pass would see that reads every DAG row's supports one entry on: entry i of a row gets the support of entry
    i + 1 of the same row, the last one the first's"""
    import oracle as O

    dag = O.orient(O.OGraph(g.row_ptr, g.col_idx))
    rp, ci = dag.row_ptr.astype(np.int64), dag.col_idx.astype(np.int64)
    n = np.diff(rp)
    src = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), n)
    pos = np.arange(ci.size, dtype=np.int64) - rp[src]
    nxt = rp[src] + (pos + 1) % np.maximum(n[src], 1)
    out = np.zeros_like(t)
    out[src, ci] = t[src, ci[nxt]]
    return out + out.T


def _isum(a) -> int:
    """the exact sum of an integer-valued array whose entries fit int64"""
    return sum(np.asarray(a).astype(np.int64).ravel().tolist())


def _c2(a):
    a = np.asarray(a).astype(np.int64)
    return a * (a - 1) // 2


class _Dense:
    """the dense matrices of one graph, under a mutant or none; the sums on request"""

    def __init__(self, g, mutant=None):
        assert mutant in (None, "supports", "degrees"), mutant
        rp, ci, src = _csr(g)
        self.exact = mutant is None
        self.adj = adj = _adjacency(g)
        d = adj.sum(axis=1)
        self.t = (adj @ adj) * adj
        if mutant == "supports":
            self.t = _rotated_supports(g, self.t)
        if mutant == "degrees":
            d = np.roll(d, 1)
        self.d = d
        self.di = d.astype(np.int64)
        und = src < ci
        self.eu, self.ev = src[und], ci[und]
        self.te = self.t[self.eu, self.ev].astype(np.int64)  # t per undirected edge
        tv2 = self.t.sum(axis=1).astype(np.int64)
        assert not self.exact or not (tv2 & 1).any()
        self.tv = tv2 // 2

    def raw5(self, need) -> dict:
        need = set(need)
        if need - set(DENSE5):
            raise ValueError(f"no dense form for {sorted(need - set(DENSE5))}")
        adj, d, di, eu, ev, te, tv = self.adj, self.d, self.di, self.eu, self.ev, self.te, self.tv
        out = dict.fromkeys(R5.RAW, 0)
        tsum = _isum(te)
        assert not self.exact or tsum % 3 == 0
        out["T"] = tsum // 3
        out["D"] = _isum(_c2(te))
        out["W"] = _isum(_c2(te) * (di[eu] + di[ev] - 6))
        out["H"] = _isum(_c2(tv))
        out["S"] = _isum(tv * di)
        if need & {"A", "B"}:
            x = (self.t - 1.0) * adj
            xe = te - 1
            out["A"] = _isum(xe * ((adj * (d - 2.0)[None, :]) @ adj)[eu, ev].astype(np.int64))
            xa = x @ adj
            b2 = _isum(xe * (xa + xa.T)[eu, ev].astype(np.int64))  # (Adj X = (X Adj)^T: both are symmetric)
            assert not self.exact or b2 % 2 == 0
            out["B"] = b2 // 2
        if "P" in need:
            e1 = (adj @ (d - 1.0)).astype(np.int64)
            p2 = (adj @ ((d - 1.0) ** 2)).astype(np.int64)
            out["P"] = sum((a * a - b) // 2 for a, b in zip(e1.tolist(), p2.tolist()))
        return {k: (v % M64 if k in need else 0) for k, v in out.items()}

    def raw6(self, need) -> dict:
        need = set(need)
        if need - set(DENSE6):
            raise ValueError(f"no dense form for {sorted(need - set(DENSE6))}")
        adj, d, di, eu, ev, te, tv = self.adj, self.d, self.di, self.eu, self.ev, self.te, self.tv
        out = dict.fromkeys(R6.RAW, 0)
        if need & {"X", "Y", "M"}:
            e1 = (adj @ (d - 1.0)).astype(np.int64)
            out["X"] = _isum((e1[eu] - (di[ev] - 1) - te) * (e1[ev] - (di[eu] - 1) - te))
            out["Y"] = _isum(tv * (di - 2) ** 2)
            out["M"] = _isum((tv[eu] - te) * (tv[ev] - te))
        if need & {"Z", "R"}:
            c = adj @ adj
            np.fill_diagonal(c, 0.0)
            per_v = (c * (c - 1.0) / 2.0).sum(axis=1).astype(np.int64)  # C(c, 2) over every x != v: every 4-cycle at each of its corners
            r4 = _isum(per_v)
            assert r4 % 4 == 0
            out["R"] = r4 // 4
            out["Z"] = _isum(per_v * di)
        if need & {"D", "B"}:
            r5 = self.raw5([k for k in ("D", "B") if k in need])
            out["D"], out["B"] = r5["D"], r5["B"]
        return {k: (v % M64 if k in need else 0) for k, v in out.items()}


def dense_raw5(g, need=DENSE5, mutant=None) -> dict:
    """the sums of `need` keyed like sgl5_ref.RAW (the others 0), modulo 2^64"""
    return _Dense(g, mutant).raw5(need)


def dense_raw6(g, need=("X", "Y", "Z", "R", "M"), mutant=None) -> dict:
    """the sums of `need` keyed like sgl6_ref.RAW (the others 0), modulo 2^64"""
    return _Dense(g, mutant).raw6(need)


def _supports_of(g, dn):
    rp, ci, src = _csr(g)
    return dn.t[src, ci].astype(np.uint32), dn.tv.astype(np.uint64)


def dense_supports(g):
    """(t per entry in the caller's entry order as uint32, T_v as uint64)"""
    return _supports_of(g, _Dense(g))


def row_facts(g, tct_stage_max: int, short: int = 1024) -> dict:
    """where the DAG rows (oracle.orient) of g lie: "rows" their lengths, "stage" / "beyond" the numbers of rows in (short, tct_stage_max] /
    beyond tct_stage_max, and per group the distinct values a pass reads on the entries of those rows: their supports, the degrees of their
    keys"""
    import oracle as O

    dag = O.orient(O.OGraph(g.row_ptr, g.col_idx))
    rp, ci = dag.row_ptr.astype(np.int64), dag.col_idx.astype(np.int64)
    n = np.diff(rp)
    src = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), n)
    t = _Dense(g).t[src, ci].astype(np.int64)
    deg = np.diff(np.asarray(g.row_ptr).astype(np.int64))
    out = {"rows": n, "longest": int(n.max())}
    for name, rows in (("stage", (n > short) & (n <= tct_stage_max)), ("beyond", n > tct_stage_max)):
        on = rows[src]
        out[name] = int(rows.sum())
        out[name + "_supports"] = int(np.unique(t[on]).size)
        out[name + "_degrees"] = int(np.unique(deg[ci[on]]).size)
    out["supports"] = int(np.unique(t).size)
    out["degrees"] = int(np.unique(deg).size)
    return out


@functools.lru_cache(maxsize=None)
def cell(name: str):
    return graded(*CELLS[name])


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """{"raw5", "raw6", "sup", "tv"} of a cell: one pass over its dense matrices, shared by every test of the process, read-only"""
    g = cell(name)
    dn = _Dense(g)
    sup, tv = _supports_of(g, dn)
    sup.setflags(write=False)
    tv.setflags(write=False)
    return {"raw5": dn.raw5(DENSE5), "raw6": dn.raw6(("X", "Y", "Z", "R", "M")), "sup": sup, "tv": tv}
