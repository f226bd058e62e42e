"""The cells of tests/test_gpu_clique_count_planted.py: planted-clique graphs (tests/planted_cliques.py) for the GLOBAL k-clique count
(gm_clique), one graph per side of every row length at which the count changes path.  numpy only; nothing of the library takes part in
a graph or in an expected value.  The library's constants (gm_constant, handed in as `c`: count_constants() of the test files) place the
rows, and the class rule of csrc/gm_mine.h (clique_is_wide, clique_mma_class, clique_mma_stride, clique_mma_fits,
clique_mma_block_words) is RESTATED here from those constants, so a constant that moves takes its cells with it.

The expected total needs no enumeration: a k-clique lies inside one block plus at most one member of I, so
    total_k = sum over the blocks B of  K_k(B) + n_I(B) K_{k-1}(B)
with K_m of a complete block a binomial and K_m of a random block from clique_local_ref on the block alone (planted_cliques.block_values).

Families (DESIGN.md "k-clique count: planted cells"):
  M   k = 4, one root per cell at every row length of STEPS, scattered: a complete block of more than half the row, a second complete block
      of another size, random blocks of 8 .. 14; at cb_max_deg one more cell whose H is ONE complete block; K_(cb_max_deg + 1) plain
  Mc  the same recipe, contiguous (block-diagonal matrices), at four row lengths
  B   contiguous, the big block LAST and under tops: the root's edges into it are hosted by the far end (type B tasks)
  R   six roots on block prefixes in one graph: every class in one launch; once more with an arena of 1 MiB
  D   k >= 5: complete blocks whose members give sub-matrices of b - 1, b - 2, .. columns on both sides of every switch of csrc/gm_chunk.h;
      at 2048 / 2049 columns the long matrix row is a hub's over random blocks (planted_cliques block kind "hub")"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from math import comb

import numpy as np

import planted_cliques as P

CONST_NAMES = ("bit_words", "mma_words_small", "mma_words_big", "wide_max_deg", "cb_max_deg", "cb_min_deg", "stage_cap", "core_h_default")


# ---- the class rule of csrc/gm_mine.h, restated -------------------------------------------------------------------------------------------
def is_wide(d, c):
    return d * ((d + 31) // 32) > c["bit_words"] and d <= c["wide_max_deg"]


def mma_stride(cw_even):
    return cw_even if (cw_even & 3) == 2 else cw_even + 2


def mma_fits(d, cw_even, budget):
    return ((d + 63) & ~63) * mma_stride(cw_even) <= budget


def mma_block_words(d, budget):
    stride = (d + 31) // 32
    for nb in range(2, 8):
        cw = (((stride + nb - 1) // nb) + 1) & ~1
        if mma_fits(d, cw, budget):
            return cw
    return (((stride + 7) // 8) + 1) & ~1


def mma_class(d, c):
    cw = (((d + 31) // 32) + 1) & ~1
    if mma_fits(d, cw, c["mma_words_small"]):
        return 0
    return 1 if mma_fits(d, cw, c["mma_words_big"]) else 2


def row_class(d, c):
    """what counts the matrix of a DAG row of d entries at k = 4: "none" (no matrix), "narrow" (clique_small_kernel), ("mma", 0 | 1) (whole
    matrix in LDS), ("mma", 2, blocks, words per block) (column blocks), "arena" (the mining kernel's arena path)"""
    if d < c["cb_min_deg"]:
        return "none"
    if d > c["cb_max_deg"]:
        return "arena"
    if not is_wide(d, c):
        return "narrow"
    cls = mma_class(d, c)
    if cls < 2:
        return ("mma", cls)
    cw = mma_block_words(d, c["mma_words_big"])
    return ("mma", 2, -(-((d + 31) // 32) // cw), cw)


def class_steps(c):
    """[(d, class of d, class of d + 1)] for every d at which the class changes"""
    out, prev = [], row_class(c["cb_min_deg"], c)
    for d in range(c["cb_min_deg"] + 1, c["cb_max_deg"] + 2):
        cur = row_class(d, c)
        if cur != prev:
            out.append((d - 1, prev, cur))
        prev = cur
    return out


# what class_steps gives with the constants of today (the table of the issue; tests/test_planted_count_cells_host.py asserts it)
STEPS_TODAY = [(256, "narrow", ("mma", 0)), (512, ("mma", 0), ("mma", 1)), (1024, ("mma", 1), ("mma", 2, 2, 18)),
               (1152, ("mma", 2, 2, 18), ("mma", 2, 2, 20)), (1280, ("mma", 2, 2, 20), ("mma", 2, 2, 22)),
               (1408, ("mma", 2, 2, 22), ("mma", 2, 3, 16)), (1536, ("mma", 2, 3, 16), ("mma", 2, 3, 18)),
               (1728, ("mma", 2, 3, 18), ("mma", 2, 4, 14)), (1792, ("mma", 2, 4, 14), ("mma", 2, 4, 16)), (2048, ("mma", 2, 4, 16), "arena")]


# ---- cells ---------------------------------------------------------------------------------------------------------------------------------
AS_NUMBERED, CLIQUE4_MINING, ROW_GATHER, ANY_WIDTH, FILTER_STAGE2 = 0x200, 0x40000, 0x8000000, 0x200000, 0x20
BASE_FORMS = ("default", "as_numbered", "core_h0")
MORE_FORMS = ("row_gather", "mining", "core_cut32", "core_cut3", "world3", "world2p1")


@dataclass(frozen=True)
class Cell:
    name: str
    family: str      # M | Mc | B | R | D
    row: int         # the DAG row of the (longest) root
    between: tuple   # the description of the sides: (class of this row, class of the neighbouring row on the other side of the step)
    ks: tuple
    forms: tuple
    scattered: bool
    recipe: str      # "mix" | "one" | "typeb" | "roots" | "kblock" | "khub"
    arg: tuple = ()  # kblock: (size of the complete block, (lo, hi, p) of the filler); roots: the rows


DEEP = (15, 18, 0.9)  # the filler of the cells at k = 8, 9: G(13, 0.9) holds a 9-clique in 5 blocks of 6 only
R_ROWS = (100, 300, 600, 1100, 1500)  # family R: and one root of cb_max_deg entries


def cells(c) -> tuple:
    out = []
    steps = class_steps(c)
    designated = {steps[2][0] + 1, steps[5][0] + 1, c["cb_max_deg"]} if len(steps) >= 6 else {c["cb_max_deg"]}
    for d, lo, hi in steps:
        for row, here, there in ((d, lo, hi), (d + 1, hi, lo)):
            forms = BASE_FORMS + (MORE_FORMS if row in designated else ())
            out.append(Cell(f"M-{row}", "M", row, (here, there), (4,), forms, True, "mix"))
    top = c["cb_max_deg"]
    out.append(Cell(f"M-{top}-one-block", "M", top, (row_class(top, c), "arena"), (4,), BASE_FORMS, True, "one"))
    mc_rows = [steps[1][0] + 1, steps[2][0] + 1, steps[5][0] + 1, top] if len(steps) >= 6 else [top]
    for row in mc_rows:
        out.append(Cell(f"Mc-{row}", "Mc", row, (row_class(row, c), row_class(row, c)), (4,), BASE_FORMS, False, "mix"))
    for row in (200, steps[1][0] + 288, steps[5][0] + 92):  # narrow, class 1, class 2 (800 and 1500 today)
        out.append(Cell(f"B-{row}", "B", row, (row_class(row, c), row_class(row, c)), (4,), BASE_FORMS, False, "typeb"))
    out.append(Cell("R-roots", "R", top, (row_class(top, c), "arena"), (4,), BASE_FORMS + MORE_FORMS + ("small_arena",), True, "roots", R_ROWS + (top,)))
    # k >= 5 (csrc/gm_chunk.h): m = the set bits of a matrix row = the columns of a sub-matrix; a complete block of b members under the root
    # gives m = b - 1, b - 2, ..
    kf = ("default", "as_numbered")
    for b in (65, 66, 129, 130):  # words = ((m + 63) >> 6) * 2 and the zeroing of the words behind them
        out.append(Cell(f"D-m{b - 1}", "D", 200, ("m", b - 1), (5, 6), kf, True, "kblock", (b, P.HIGH)))
    for b in (257, 258):          # 256 set bits: sub-matrix in LDS or in the second arena slot
        out.append(Cell(f"D-m{b - 1}", "D", 300, ("m", b - 1), (5, 6), kf, True, "kblock", (b, P.HIGH)))
    for row in (steps[0][0], steps[0][0] + 1):  # bits_lds or not
        out.append(Cell(f"D-row{row}", "D", row, ("row", row), (5, 6), kf, True, "kblock", (100, P.HIGH)))
    # 2048 set bits: tile walk or any-width pair count.  A complete block of 2049 costs 24 s at k = 5 (every member is a root of its own,
    # 112 s with the any-width count), so the long matrix row is the HUB's: a "hub" block, contiguous -- the hub has the lowest id, all its
    # block is behind it -- over random blocks of 8 .. 14; the root's row is the block
    for b in (top + 1, top + 2):
        out.append(Cell(f"D-m{b - 1}", "D", b, ("m", b - 1), (5,), kf + ("any_width",), False, "khub", (b,)))
    for row in (2 * top, 2 * top + 1):  # 4096 columns: cliquek_count_sub or _sub_any
        out.append(Cell(f"D-row{row}", "D", row, ("row", row), (5,), kf, True, "kblock", (120, P.LOW)))
    out.append(Cell("D-k8", "D", 300, ("k", 8), (8,), kf + ("filter_stage2",), True, "kblock", (24, DEEP)))  # the last inlined level
    out.append(Cell("D-k9", "D", 300, ("k", 9), (9,), kf + ("filter_stage2",), True, "kblock", (24, DEEP)))  # the first called level
    return tuple(out)


def mix_blocks(d):
    """family M / Mc: (big complete block: more than half the row, second complete block of another size, random blocks of 8 .. 14)"""
    big, second = d // 2 + 2, d // 4 + 5
    lo, hi, p = P.LOW
    return (P.Block("complete", big), P.Block("complete", second)) + P.random_blocks(d - big - second, lo, hi, p)


def typeb_blocks(d):
    """family B: random blocks first, the big complete block last (contiguous: its members are the tail of the root's row)"""
    big = d // 2
    lo, hi, p = P.LOW
    return P.random_blocks(d - big, lo, hi, p) + (P.Block("complete", big),)


def roots_blocks(rows):
    """family R: blocks cut so that every root's row ends with a block; each stretch = a complete block of a size of its own + random blocks"""
    lo, hi, p = P.LOW
    blocks, ends, done = (), [], 0
    for i, r in enumerate(rows):
        need = r - done
        big = need // 2 + 3 + i
        if need - big < lo:  # (shrunken instances: the stretch is one complete block)
            big = need
        blocks += (P.Block("complete", big),) + (P.random_blocks(need - big, lo, hi, p, first=len(blocks)) if need > big else ())
        ends.append(len(blocks))
        done = r
    return blocks, ends


def build(cell: Cell, shrink: int = 1) -> P.Planted:
    """the graph of a cell.  shrink > 1: the same blocks-and-members recipe on a row of about cell.row / shrink entries (the host test holds
    it against the oracle)"""
    d = max(cell.row // shrink, 64) if shrink > 1 else cell.row
    if cell.recipe == "mix":
        blocks = mix_blocks(d)
        return P.Planted(blocks, P._standard_members(blocks, d), cell.scattered)
    if cell.recipe == "one":
        blocks = (P.Block("complete", d),)
        return P.Planted(blocks, (P.Member((0,), d // 3),), cell.scattered)
    if cell.recipe == "typeb":
        blocks = typeb_blocks(d)
        nb = len(blocks)
        # the root on every block, its id below H; two tops on the big block (ids below and above H), one on the even random blocks
        members = (P.Member(tuple(range(nb)), 0), P.Member((nb - 1,), 0, True), P.Member((nb - 1,), d, True), P.Member(tuple(range(0, nb - 1, 2)), d, True))
        return P.Planted(blocks, members, cell.scattered)
    if cell.recipe == "roots":
        rows = tuple(max(r // shrink, 12 * (i + 1)) for i, r in enumerate(cell.arg)) if shrink > 1 else cell.arg
        rows = tuple(sorted(set(rows)))
        blocks, ends = roots_blocks(rows)
        nb, dd = len(blocks), rows[-1]
        # (ids: the longest root first, the shortest last; a top on the even blocks)
        ats = (0, dd // 2, dd // 3, dd, dd // 4, 2 * dd // 3)
        members = tuple(P.Member(tuple(range(e)), ats[j % 6]) for j, e in enumerate(reversed(ends)))
        return P.Planted(blocks, members + (P.Member(tuple(range(0, nb, 2)), 0, True),), cell.scattered)
    if cell.recipe == "khub":
        blocks = (P.Block("hub", d, P.LOW[2], 1),)
        return P.Planted(blocks, (P.Member((0,), 0),), cell.scattered)
    if cell.recipe == "kblock":
        b, (lo, hi, p) = cell.arg
        b = max(b // shrink, 12) if shrink > 1 else b
        if d - b < lo:  # (shrunken instances; the cells whose row IS the block)
            b = d
        rest = d - b
        blocks = (P.Block("complete", b),) + (P.random_blocks(rest, lo, hi, p) if rest else ())
        assert sum(x.size for x in blocks) == d, (cell.name, d, b)
        members = (P.Member(tuple(range(len(blocks))), d // 3),)
        if len(blocks) > 2:
            members += (P.Member(tuple(range(1, len(blocks), 2)), 0, True),)
        return P.Planted(blocks, members, cell.scattered)
    raise ValueError(cell.recipe)


@functools.lru_cache(maxsize=2)
def cell_graph(cell: Cell) -> P.Planted:
    return build(cell)


# ---- what is known about a cell's graph ----------------------------------------------------------------------------------------------------
def block_cliques(blk: P.Block, m: int) -> int:
    """K_m of a block"""
    if m == 0:
        return 1
    if m == 1:
        return blk.size
    if blk.kind == "complete":
        return comb(blk.size, m)
    if blk.kind == "hub":  # with the hub or without it
        return sum(block_cliques(part, m) + block_cliques(part, m - 1) for part in P.hub_parts(blk)) + (1 if m == 1 else 0)
    s = sum(int(x) for x in P.block_values(blk, m)[1])
    assert s % m == 0
    return s // m


def planted_total(g: P.Planted, k: int) -> int:
    return sum(block_cliques(b, k) + int(g.n_i[bi]) * block_cliques(b, k - 1) for bi, b in enumerate(g.blocks))


def block_shares(g: P.Planted, k: int) -> list:
    """(size, share of the total) of every block"""
    tot = planted_total(g, k)
    return [(b.size, (block_cliques(b, k) + int(g.n_i[bi]) * block_cliques(b, k - 1)) / tot) for bi, b in enumerate(g.blocks)]


def blocks_with_clique(g: P.Planted, k: int) -> float:
    return sum(1 for b in g.blocks if block_cliques(b, k) > 0) / len(g.blocks)


def stated_rows(cell: Cell, g: P.Planted) -> np.ndarray:
    """the DAG row lengths of the core vertices the RECIPE implies, sorted: a root's row = the sizes of its blocks; the member of rank j (in
    id order) of a complete block of b = b - 1 - j + its tops; a top's = 0.  Random blocks: taken from the block's own edges in id order."""
    rows = []
    for x, m in enumerate(g.members):
        rows.append(0 if m.top else sum(g.blocks[bi].size for bi in m.blocks))
    ntop = np.zeros(len(g.blocks), dtype=np.int64)
    for m in g.members:
        if m.top:
            ntop[list(m.blocks)] += 1
    for bi, b in enumerate(g.blocks):
        if b.kind == "complete":
            rows += [b.size - 1 - j + int(ntop[bi]) for j in range(b.size)]
        else:
            ids = g.h_id[g.first[bi]:g.first[bi + 1]]
            a, e = P.block_pairs(b)
            lo = np.where(ids[a] < ids[e], a, e)
            rows += (np.bincount(lo, minlength=b.size) + int(ntop[bi])).tolist()
    return np.sort(np.array(rows, dtype=np.int64))


def class_census(rows, c) -> dict:
    """rows by class: {"narrow", "arena", 0, 1, 2: counts} over the rows with a matrix"""
    out = {"narrow": 0, "arena": 0, 0: 0, 1: 0, 2: 0}
    for d in np.asarray(rows).tolist():
        rc = row_class(d, c)
        if rc != "none":
            out[rc if isinstance(rc, str) else rc[1]] += 1
    return out


def topo_ids(g: P.Planted) -> np.ndarray:
    """the id of every core vertex on the topological copy: ids ascending in (degree, id) -- the leaves (degree 1) first"""
    deg = np.diff(g.row_ptr)[:g.n_core]
    order = np.lexsort((np.arange(g.n_core), deg))
    tid = np.empty(g.n_core, dtype=np.int64)
    tid[order] = (g.nv - g.n_core) + np.arange(g.n_core)
    return tid


def dag_edges(g: P.Planted):
    """(u, v) of every DAG edge between core vertices, caller's ids (a leaf's one edge, leaf -> owner, belongs to no matrix)"""
    return g._csrc[g._out], g._ccol[g._out]


def plan_tasks(g: P.Planted, c, core_base=-1) -> int:
    """the tasks of the streamed build (cb_owner_sizes_kernel): every DAG entry of an owner with a matrix; of a WIDE owner beside a core
    bitmap only the entries whose end lies below core_base (ids of the topological copy)"""
    d = g.row_len
    owner = (d >= c["cb_min_deg"]) & (d <= c["cb_max_deg"])
    wide = np.array([is_wide(int(x), c) for x in d])
    tasks = int(d[owner & ~wide].sum())
    if core_base < 0:
        return tasks + int(d[owner & wide].sum())
    u, v = dag_edges(g)
    tid = topo_ids(g)
    return tasks + int(((tid[v] < core_base) & owner[u] & wide[u]).sum())


def root_hosting(g: P.Planted, x: int, c, topo=True):
    """the edges of root x (member index) by the endpoint that hosts them (cb_task_rows_kernel): position i of the row is hosted by the far end
    v when d+(v) > tail and d+(v) <= cb_max_deg; tail = d - i - 1 on the topological copy, d as numbered.  Returns (type A, type B)."""
    u = int(g.i_id[x])
    us, vs = dag_edges(g)
    row = vs[us == u]
    key = topo_ids(g)[row] if topo else row
    row = row[np.argsort(key)]
    d = row.size
    tail = d - np.arange(d) - 1 if topo else np.full(d, d)
    dv = g.row_len[row]
    b = int(((dv > tail) & (dv <= c["cb_max_deg"])).sum())
    return d - b, b


def matrix_words(g: P.Planted, c) -> int:
    """the arena words of every matrix: d x ceil(d / 32) per owner"""
    d = g.row_len[(g.row_len >= c["cb_min_deg"]) & (g.row_len <= c["cb_max_deg"])]
    return int((d * ((d + 31) // 32)).sum())


def core_cut(g: P.Planted, x: int, plus: int):
    """GM_CORE_H whose base cuts the row of root x near its middle: base a multiple of 32 (+ plus).  Returns (h, base)."""
    u = int(g.i_id[x])
    us, vs = dag_edges(g)
    t = np.sort(topo_ids(g)[vs[us == u]])
    base = (int(t[t.size // 2]) & ~31) + plus
    assert t[0] < base <= t[-1]
    return g.nv - base, base
