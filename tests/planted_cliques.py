"""Planted cliques: symmetric graphs whose local k-clique counts are known ENTRY BY ENTRY at any row length (test helper; imported by
tests/test_planted_cliques_host.py and tests/test_gpu_clique_local_planted.py).  Graphs and expected values are made with numpy and
clique_local_ref alone; the one thing taken from the package is the Graph CONTAINER the `graph` property wraps the finished CSR in
(imported there, as tests/probe_graphs.py does) -- no code of the library takes part in a value.

gm_clique_local (csrc/gm_kcl_local.hip) attributes cliques: a pair of positions of a root's row gets a value and that value has to land
on the right entry of the right row.  On a complete graph every entry carries the same value, so a wrong position passes; a random graph
with a row of 2049 entries has no plain reference that finishes.  These graphs have long rows AND a different value on nearly every entry:

  H      d vertices that hold disjoint BLOCKS, each a small graph on its own vertex set: `complete` (a clique, closed forms), `random`
         (a seeded G(b, p), another graph per block) or `hub` (its first vertex joined to all the others, those a disjoint union of
         random blocks: one long matrix row over a sparse sub-matrix, for the global count's cells)
  I      an independent set; every member is joined to a chosen union of WHOLE blocks
  leaves every H vertex is padded with private degree-1 leaves to one common degree D (above every degree of a root), as the probe graphs
         do (tests/probe_graphs.py)
  root   a member of I left as it is: degree < D.  Under the orientation (lower degree -> higher degree, ties by id) its DAG row is exactly
         the H vertices it is joined to, in id order
  top    a member of I padded with leaves to D + 1: it sits in the DAG rows of the H vertices it is joined to -- at their end on the
         topological copy, wherever its id puts it as numbered
  leaf   one out-neighbour: no k-clique, skipped by the kernel

The layout of H is contiguous (a block's members are consecutive ids) or scattered (a seeded permutation: the set of every pair is spread
over all words of the root's row).  The members of I get their ids before the H vertex of a chosen rank (0: below all of H, d: above).

Expected values without an enumeration of the whole graph: a k-clique lies inside one block plus at most one member of I, so
  an inner entry of block B carries      K_k(B, edge) + n_I(B) K_{k-1}(B, edge)         n_I(B): the members of I joined to B
  an entry between x in I and h in B      K_{k-1}(B, h)
  a leaf entry                            0
with K_2 = 1 on an edge and the degree at a vertex.  The per-block values come from clique_local_ref on the block alone (cached per block
and k), for a complete block from binomials.  K_v = (row sum) / (k - 1), the total = (sum of all entries) / (k (k - 1)).
tests/test_planted_cliques_host.py confirms the rule against clique_local_ref on whole (small) graphs."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from math import comb

import numpy as np

import clique_local_ref as R

VARIANTS = 32  # a random block is G(b, p) of seed (b, its index mod VARIANTS): the values of (block, k) are computed once for all graphs


@dataclass(frozen=True)
class Block:
    kind: str       # "complete" | "random" | "hub" (one vertex joined to all of a disjoint union of random blocks: tests/planted_count_cells.py)
    size: int
    p: float = 1.0  # random: the edge probability
    seed: int = 0   # random: the variant


@dataclass(frozen=True)
class Member:
    """a member of I: joined to the blocks `blocks` (indices), its id just below the H vertex of rank `at` (0 .. d); top: padded to D + 1"""
    blocks: tuple
    at: int
    top: bool = False


class _Csr:
    def __init__(self, row_ptr, col_idx):
        self.row_ptr, self.col_idx = row_ptr, col_idx


def _csr(n: int, s: np.ndarray, t: np.ndarray):
    """CSR of the directed pairs (s, t), rows ascending, ids inside a row ascending; returns (row_ptr, col, order of the pairs)"""
    order = np.lexsort((t, s))
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(s, minlength=n), out=rp[1:])
    return rp, t[order], order


def hub_parts(blk: Block) -> tuple:
    """the random blocks under the hub (vertex 0) of a "hub" block, in id order"""
    return random_blocks(blk.size - 1, LOW[0], LOW[1], blk.p, seed=blk.seed)


@functools.lru_cache(maxsize=None)
def block_pairs(blk: Block):
    """the edges a < b of a block on local ids 0 .. size - 1, as two arrays"""
    if blk.kind == "hub":  # vertex 0 joined to every other vertex; those: disjoint random blocks of the LOW sizes (hub_parts), p and seed the block's
        a, b, off = [np.zeros(blk.size - 1, dtype=np.int64)], [np.arange(1, blk.size, dtype=np.int64)], 1
        for part in hub_parts(blk):
            pa, pb = block_pairs(part)
            a.append(pa + off)
            b.append(pb + off)
            off += part.size
        a, b = np.concatenate(a), np.concatenate(b)  # (rows ascending, then ids: the order block_values relies on)
        a.setflags(write=False)
        b.setflags(write=False)
        return a, b
    a, b = np.triu_indices(blk.size, 1)
    if blk.kind == "random":
        rng = np.random.default_rng([blk.size, blk.seed, int(round(blk.p * 1000))])
        keep = rng.random(a.size) < blk.p
        a, b = a[keep], b[keep]
    else:
        assert blk.kind == "complete"
    a, b = a.astype(np.int64), b.astype(np.int64)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def block_values(blk: Block, m: int):
    """(per edge a < b of block_pairs: the m-cliques of the block on it, per vertex: the m-cliques at it) as Python-int object arrays"""
    a, b = block_pairs(blk)
    n = blk.size
    if m == 2:
        e = np.ones(a.size, dtype=object)
        v = (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(object)
    elif blk.kind == "complete":
        e = np.full(a.size, comb(n - 2, m - 2), dtype=object)
        v = np.full(n, comb(n - 1, m - 1), dtype=object)
    else:
        rp, col, _ = _csr(n, np.concatenate([a, b]), np.concatenate([b, a]))
        g = _Csr(rp, col)
        ent = R.entry_cliques(g, m)
        v = np.array([int(x) for x in R.vertex_cliques(g, m, ent)], dtype=object)
        src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        up = src < col  # (the entries a < b of the CSR come in the order of block_pairs: rows ascending, then ids)
        assert np.array_equal(src[up], a) and np.array_equal(col[up], b)
        e = np.array([int(x) for x in ent[up]], dtype=object)
    e.setflags(write=False)
    v.setflags(write=False)
    return e, v


def block_sizes(total: int, lo: int, hi: int, seed: int) -> list:
    """sizes in lo .. hi that add up to `total`, seeded; no remainder block outside the range"""
    assert total >= lo
    nb = max(1, round(total / ((lo + hi) / 2)))
    nb = min(max(nb, -(-total // hi)), total // lo)
    assert nb * lo <= total <= nb * hi, (total, lo, hi)
    rng = np.random.default_rng([total, lo, hi, seed])
    sizes = np.full(nb, lo, dtype=np.int64)
    for _ in range(total - nb * lo):
        open_ = np.flatnonzero(sizes < hi)
        sizes[open_[rng.integers(open_.size)]] += 1
    return sizes.tolist()


def random_blocks(total: int, lo: int, hi: int, p: float, seed: int = 0, first: int = 0) -> tuple:
    return tuple(Block("random", b, p, (first + i) % VARIANTS) for i, b in enumerate(block_sizes(total, lo, hi, seed)))


class Planted:
    """a planted graph and what is known about it.  graph: graphminer_amd Graph; d: |H|; h_id[j]: the id of the H vertex in slot j (slots:
    block after block), first[b]: the first slot of block b; i_id[x]: the id of member x of I; row_len: the DAG row length of every CORE vertex (index: id; leaves
    have 1); max_row: the DAG's longest row; D: the common degree of H"""

    def __init__(self, blocks, members, scattered, seed=0):
        self.blocks, self.members, self.scattered = tuple(blocks), tuple(members), scattered
        sizes = np.array([b.size for b in self.blocks], dtype=np.int64)
        d = int(sizes.sum())
        self.d = d
        first = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=first[1:])
        self.first = first
        rank = np.random.default_rng([d, seed, 77]).permutation(d) if scattered else np.arange(d)  # slot -> rank among H in id order
        # ids: the members of I go in before the H vertex of rank `at`
        ats = np.array([m.at for m in self.members], dtype=np.int64)
        assert ((0 <= ats) & (ats <= d)).all()
        below = np.searchsorted(np.sort(ats), np.arange(d), side="right")  # members placed at or before rank r
        self.h_id = (rank + below[rank]).astype(np.int64)
        order = np.argsort(ats, kind="stable")
        i_id = np.empty(len(self.members), dtype=np.int64)
        i_id[order] = np.sort(ats) + np.arange(len(self.members))
        self.i_id = i_id
        n_core = d + len(self.members)
        self.n_core = n_core
        assert len(np.unique(np.concatenate([self.h_id, i_id]))) == n_core
        self.is_h = np.zeros(n_core, dtype=bool)
        self.is_h[self.h_id] = True
        self.n_i = np.zeros(len(sizes), dtype=np.int64)
        for m in self.members:
            assert len(set(m.blocks)) == len(m.blocks)
            self.n_i[list(m.blocks)] += 1
        # the core edges, both directions, with the block and the position of the value they carry
        s, t, kind, blk, idx = [], [], [], [], []  # kind 0: inner (idx: edge of block_pairs), 1: between I and H (idx: local vertex)
        for bi, b in enumerate(self.blocks):
            a, c = block_pairs(b)
            ga, gc = self.h_id[first[bi] + a], self.h_id[first[bi] + c]
            s += [ga, gc]
            t += [gc, ga]
            e = np.arange(a.size, dtype=np.int64)
            kind += [np.zeros(2 * a.size, dtype=np.int8)]
            blk += [np.full(2 * a.size, bi, dtype=np.int64)]
            idx += [e, e]
        for x, m in enumerate(self.members):
            for bi in m.blocks:
                h = self.h_id[first[bi]:first[bi + 1]]
                xs = np.full(h.size, i_id[x], dtype=np.int64)
                s += [xs, h]
                t += [h, xs]
                loc = np.arange(h.size, dtype=np.int64)
                kind += [np.ones(2 * h.size, dtype=np.int8)]
                blk += [np.full(2 * h.size, bi, dtype=np.int64)]
                idx += [loc, loc]
        s, t = np.concatenate(s), np.concatenate(t)
        crp, ccol, order = _csr(n_core, s, t)
        self._kind, self._blk, self._idx = np.concatenate(kind)[order], np.concatenate(blk)[order], np.concatenate(idx)[order]
        cdeg = np.diff(crp)
        top = np.zeros(n_core, dtype=bool)
        top[i_id[[x for x, m in enumerate(self.members) if m.top]]] = True
        self.is_top = top
        root_deg = cdeg[~self.is_h & ~top]
        self.D = int(max(cdeg[self.is_h].max(), root_deg.max() if root_deg.size else 0)) + 1
        target = np.where(self.is_h, self.D, np.where(top, self.D + 1, cdeg))
        nleaf = target - cdeg
        assert (nleaf >= 0).all()
        # the whole CSR: a core row is its core row followed by its own range of leaf ids; a leaf's row is its owner
        n_leaves = int(nleaf.sum())
        nv = n_core + n_leaves
        deg = np.ones(nv, dtype=np.int64)
        deg[:n_core] = target
        rp = np.zeros(nv + 1, dtype=np.int64)
        np.cumsum(deg, out=rp[1:])
        col = np.empty(int(rp[-1]), dtype=np.int32)
        csrc = np.repeat(np.arange(n_core, dtype=np.int64), cdeg)
        self._core_entry = rp[csrc] + (np.arange(ccol.size, dtype=np.int64) - crp[csrc])
        col[self._core_entry] = ccol
        owner = np.repeat(np.arange(n_core, dtype=np.int64), nleaf)
        lfirst = np.zeros(n_core + 1, dtype=np.int64)
        np.cumsum(nleaf, out=lfirst[1:])
        col[rp[owner] + cdeg[owner] + (np.arange(n_leaves, dtype=np.int64) - lfirst[owner])] = (n_core + np.arange(n_leaves)).astype(np.int32)
        col[rp[n_core:nv]] = owner.astype(np.int32)
        self.row_ptr, self.col_idx, self.nv = rp, col, nv
        self._csrc, self._ccol = csrc, ccol
        # the orientation, restated: u -> v when (deg, id) of v is the greater.  Leaves (degree 1 < every core degree) point at their owner
        # and nobody points at them.
        out = (target[ccol] > target[csrc]) | ((target[ccol] == target[csrc]) & (ccol > csrc))
        assert target.min() > 1, "a core vertex of degree 1 would tie with the leaves"
        self.row_len = np.bincount(csrc[out], minlength=n_core).astype(np.int64)
        self.max_row = int(max(self.row_len.max(), 1 if n_leaves else 0))
        self._out = out
        self._expected = {}

    @property
    def graph(self):
        """the CSR in the package's container (what to_device takes); nothing above or below depends on it"""
        from graphminer_amd.graph import Graph

        if not hasattr(self, "_graph"):
            self._graph = Graph(row_ptr=self.row_ptr, col_idx=self.col_idx, name="planted")
        return self._graph

    def root_rows(self) -> list:
        """the DAG row length of every root (members that are no tops), in member order"""
        return [int(self.row_len[self.i_id[x]]) for x, m in enumerate(self.members) if not m.top]

    def h_rows(self, bi: int) -> np.ndarray:
        """the DAG row lengths of the H vertices of block bi, slot order"""
        return self.row_len[self.h_id[self.first[bi]:self.first[bi + 1]]]

    def dag_position(self, u: int, v: int) -> int:
        """the position of v in the DAG row of core vertex u, as numbered (-1: not there)"""
        sel = (self._csrc == u) & self._out
        row = self._ccol[sel]
        hit = np.flatnonzero(row == v)
        return int(hit[0]) if hit.size else -1

    def expected(self, k: int):
        """(entries uint64[ne], K_v uint64[nv], total int, inner: the values of the inner entries as Python ints); kept per k"""
        if k not in self._expected:
            self._expected[k] = self._expect(k)
        return self._expected[k]

    def _expect(self, k: int):
        vals = np.zeros(self._kind.size, dtype=object)
        for bi, b in enumerate(self.blocks):
            ek, _ = block_values(b, k)
            ek1, vk1 = block_values(b, k - 1)
            inner = ek + int(self.n_i[bi]) * ek1
            sel = np.flatnonzero(self._blk == bi)
            isin = self._kind[sel] == 0
            vals[sel[isin]] = inner[self._idx[sel[isin]]]
            vals[sel[~isin]] = vk1[self._idx[sel[~isin]]]
        assert all(0 <= int(x) < 2 ** 64 for x in vals)
        ent = np.zeros(self.col_idx.size, dtype=np.uint64)
        ent[self._core_entry] = vals.astype(np.uint64)
        rows = np.zeros(self.n_core, dtype=object)
        np.add.at(rows, self._csrc, vals)
        assert all(int(x) % (k - 1) == 0 for x in rows)
        kv = np.zeros(self.nv, dtype=np.uint64)
        kv[:self.n_core] = np.array([int(x) // (k - 1) for x in rows], dtype=np.uint64)
        s = sum(int(x) for x in vals)
        assert s % (k * (k - 1)) == 0
        ent.setflags(write=False)
        kv.setflags(write=False)
        return ent, kv, s // (k * (k - 1)), [int(x) for x in vals[(self._kind == 0) & (self._csrc < self._ccol)]]

    def conditions(self, k: int) -> dict:
        """what the tests ask of a cell's inputs: the smallest block, the share of blocks that hold a k-clique, the share of non-zero inner
        entries, the distinct inner values, the largest block"""
        holds = [b.size >= k and (b.kind == "complete" or int(block_values(b, k)[1].sum()) > 0) for b in self.blocks]
        inner = self.expected(k)[3]
        return {"min_block": min(b.size for b in self.blocks), "max_block": max(b.size for b in self.blocks),
                "blocks_with_clique": sum(holds) / len(holds), "inner_nonzero": sum(1 for x in inner if x) / max(len(inner), 1),
                "inner_distinct": len(set(inner))}


# ---- the cells of tests/test_gpu_clique_local_planted.py ------------------------------------------------------------------------------
# A cell's row lengths are written against the kernel's constants (gm_constant, handed in as `consts`: "regs2", "split", "regs8",
# "regs12", "lds"; "lanes": the entries of a row of one word per lane of the wide kernel, 64 * 32), so a constant that moves takes the cell
# with it; `above` / `upto` name the constants the DAG's longest row has to lie between for the cell to run the path it claims.
WAVE = 64
LOW = (8, 14, 0.8)    # block sizes and p of the cells at k <= 5 (k + 3 <= 8)
HIGH = (13, 18, 0.9)  # ... of the cells that reach k >= 6: G(b, 0.7) of these sizes holds next to no 7-clique


@dataclass(frozen=True)
class Cell:
    name: str
    family: str          # A lane per pair, B wave per pair, C wide kernel, D all three in one call, E entry search / second build branch
    base: str            # the row of the (longest) root: consts[base] + off
    off: int
    ks: tuple
    scattered: bool
    recipe: tuple
    above: tuple = ()    # max row > each of these constants
    upto: tuple = ()     # max row <= each of these
    special: str = ""    # "k70": a complete block of 70; "mixed": family D; "find": E, the searched rows; "branch": E, b > 4 d


def _bracket(base, off):
    """the constants around a row of consts[base] + off entries on the LDS paths: (those it exceeds, those it does not)"""
    order = ["regs2", "split", "regs8", "regs12", "lds"]
    at = order.index(base) + (1 if off > 0 else 0)  # the first constant the row does not exceed
    above = tuple(order[:at])
    upto = tuple(order[at:])
    return above, upto


def _cells():
    out = []
    lay = ((False, "contig"), (True, "scat"))
    for base, off in (("regs2", -1), ("regs2", 0), ("regs2", 1)):
        for sc, ln in lay:
            for rec, rn, ks in ((LOW, "low", (3, 4, 5)), (HIGH, "high", (6, 7, 8))):
                ab, up = _bracket(base, off)
                out.append(Cell(f"A-{base}{off:+d}-{ln}-{rn}", "A", base, off, ks, sc, rec, ab, up))
    for off in (-1, 0):
        for sc, ln in lay:
            ab, up = _bracket("split", off)
            out.append(Cell(f"A-split{off:+d}-{ln}", "A", "split", off, (5, 6, 8), sc, HIGH, ab, up))
    for base, off in (("regs8", -1), ("regs8", 0), ("regs8", 1), ("regs12", -1), ("regs12", 0), ("regs12", 1), ("lds", -1), ("lds", 0)):
        for sc, ln in lay:
            ab, up = _bracket(base, off)
            out.append(Cell(f"A-{base}{off:+d}-{ln}-k34", "A", base, off, (3, 4), sc, LOW, ab, up))
    for base, off in (("split", 1), ("regs8", 0), ("regs8", 1), ("regs12", 0), ("regs12", 1), ("lds", 0)):
        for sc, ln in lay:
            ab, up = _bracket(base, off)
            out.append(Cell(f"B-{base}{off:+d}-{ln}", "B", base, off, (5, 6, 8), sc, HIGH, ab, up))
    ab, up = _bracket("lds", 0)
    out.append(Cell("B-lds+0-k70", "B", "lds", 0, (5, 6), True, HIGH, ab, up, "k70"))
    for base, off in (("lds", 1), ("lanes", 0), ("lanes", 1), ("lanes", 12)):
        out.append(Cell(f"C-{base}{off:+d}-low", "C", base, off, (3, 4, 5), True, LOW, ("lds",), ()))
        out.append(Cell(f"C-{base}{off:+d}-high", "C", base, off, (6, 8) if base == "lds" else (6,), True, HIGH, ("lds",), ()))
    out.append(Cell("D-mixed", "D", "lds", 0, (5,), True, LOW, ("lds",), (), "mixed"))
    out.append(Cell("E-find-split", "E", "regs8", 44, (5,), False, LOW, ("split",), ("lds",), "find"))
    out.append(Cell("E-find-wide", "E", "lds", 1, (5,), False, LOW, ("lds",), (), "find"))
    out.append(Cell("E-branch", "E", "", 8, (4, 5), False, (8, 8, 0.8), (), ("regs2",), "branch"))
    return tuple(out)


CELLS = _cells()
FIND_ROWS = (WAVE, WAVE + 1, 200)  # E: the rows kcl_wave_find is asked to search -- none, one and one narrowing round


def mixed_rows(consts) -> tuple:
    """D: the rows of the four roots -- lane per pair, wave per pair (k = 5), wide, and a longer wide one"""
    return (consts["split"] - 28, consts["regs8"] + 44, consts["lds"] + 1, 2 * consts["lds"] + 76)


def _standard_members(blocks, d):
    """a root on every block (its id inside the H ids), a top on the even blocks below the H ids, a top on every third block above them"""
    nb = len(blocks)
    return (Member(tuple(range(nb)), d // 3), Member(tuple(range(0, nb, 2)), 0, True), Member(tuple(range(0, nb, 3)), d, True))


def _staircase_members(blocks, d, grow=49, classes=8):
    """the members of the graphs that run k = 3, where an inner value is only (common neighbours inside the block) + n_I: a root on every
    block and step * (classes - 1) tops, top t on the blocks b with step * (b mod classes) > t, so that n_I = 1 + step * (b mod classes)
    moves the values of one block class away from the next one's.  An H row grows by at most `grow` = 49 entries: with blocks of up to 14
    vertices it stays below the shortest root of these cells (63 entries today; the host test asserts it).  Top ids below, inside and
    above the H ids in turn."""
    nb = len(blocks)
    classes = min(classes, nb)
    step = grow // (classes - 1)
    tops = [Member(tuple(b for b in range(nb) if step * (b % classes) > t), (0, d // 2, d)[t % 3], True) for t in range(step * (classes - 1))]
    return (Member(tuple(range(nb)), d // 3),) + tuple(tops)


@functools.lru_cache(maxsize=2)
def cell_graph(cell: Cell, consts_items: tuple) -> Planted:
    """the graph of a cell; consts_items: tuple(sorted(consts.items()))"""
    consts = dict(consts_items)
    d = consts.get(cell.base, 0) + cell.off  # (base "": a row length that is no path boundary)
    lo, hi, p = cell.recipe
    if cell.special == "":
        blocks = random_blocks(d, lo, hi, p)
        return Planted(blocks, (_staircase_members if 3 in cell.ks else _standard_members)(blocks, d), cell.scattered)
    if cell.special == "k70":  # the set of a pair of the complete block has 68 members: a second deal round of kcl_pair_wave
        blocks = (Block("complete", WAVE + 6),) + random_blocks(d - (WAVE + 6), lo, hi, p)
        return Planted(blocks, _standard_members(blocks, d), cell.scattered)
    if cell.special == "mixed":  # four roots on block prefixes; the blocks are cut so that every prefix ends with a block
        rows = mixed_rows(consts)
        blocks, ends, done = (), [], 0
        for r in rows:
            blocks += random_blocks(r - done, lo, hi, p, first=len(blocks))
            ends.append(len(blocks))
            done = r
        nb = len(blocks)
        # (ids: the longer wide root first, so that as numbered the shorter one follows it)
        members = (Member(tuple(range(ends[3])), 0), Member(tuple(range(ends[2])), done // 2), Member(tuple(range(ends[1])), done // 3),
                   Member(tuple(range(ends[0])), done), Member(tuple(range(0, nb, 2)), 0, True), Member(tuple(range(1, nb, 5)), done, True))
        return Planted(blocks, members, cell.scattered)
    if cell.special == "find":
        # blocks 0 and 1 get tops until their H rows hold FIND_ROWS: a row is (the block neighbours above in id order) + (the tops)
        blocks = random_blocks(d, lo, hi, p)
        bare = Planted(blocks, (Member(tuple(range(len(blocks))), d),), cell.scattered)
        ups0, ups1 = sorted(set(bare.h_rows(0).tolist())), sorted(set(bare.h_rows(1).tolist()))
        a = next(a for a in ups0 if a + 1 in ups0)
        t0, t1 = FIND_ROWS[0] - a, FIND_ROWS[2] - ups1[len(ups1) // 2]
        members = [Member(tuple(range(len(blocks))), d // 2)]
        for bi, nt in ((0, t0), (1, t1)):
            lo_id, hi_id = int(bare.h_id[bare.first[bi]:bare.first[bi + 1]].min()), int(bare.h_id[bare.first[bi]:bare.first[bi + 1]].max())
            # a third of the tops below the H ids, a third between the block's own ids, a third above all
            members += [Member((bi,), (0, (lo_id + hi_id + 1) // 2, d)[j % 3], True) for j in range(nt)]
        return Planted(blocks, tuple(members), cell.scattered)
    if cell.special == "branch":
        # 24 blocks of d = 8 vertices, a root each; 40, 42, 44, 46 tops on six blocks each (a top's degree stays below D + 1, and n_I differs
        # from group to group): an H row holds 40 .. 53 entries, more than 4 d, so the matrix build streams the root's row against it
        nb, nt, per = 24, 5 * d, 6
        blocks = random_blocks(nb * d, lo, hi, p)
        assert len(blocks) == nb
        members = [Member((bi,), bi * d) for bi in range(nb)]
        for b0 in range(0, nb, per):
            members += [Member(tuple(range(b0, b0 + per)), (0, (b0 + per // 2) * d, nb * d)[j % 3], True) for j in range(nt + 2 * (b0 // per))]
        return Planted(blocks, tuple(members), cell.scattered)
    raise ValueError(cell.special)
