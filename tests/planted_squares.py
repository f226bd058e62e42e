"""Planted squares: symmetric graphs that put the walk of gm_rect_local (csrc/gm_rect_local.hip) on a chosen path while nearly every entry
carries a different number of 4-cycles (test helper; imported by tests/test_rect_local_host.py and tests/test_gpu_rect_local.py).  Graphs
are made with numpy alone; the one thing taken from the package is the Graph CONTAINER -- no code of the library takes part in a value.
The expected values are tests/rect_local_ref.py's, on the whole graph.

  core    at most about 2,500 vertices that hold seeded random BLOCKS, each on its own vertex set: G(b, p), or bipartite G(a, b, p); every
          block draws from a seed of its own
  joined  chosen vertices (hubs, row vertices) are joined to whole blocks, to halves of blocks, or to the first vertices of one
  leaves  private degree-1 vertices that bring a core vertex to a chosen degree.  A leaf adds no 4-cycle, but it places its owner in the
          degree order -- which decides which vertex of a cycle is the centre v0 of the kernel's walk on the copy numbered ascending in
          degree -- and it is a key of its owner's row: it counts towards the row lengths at which the walk changes path

The kernel walks either the copy numbered ascending in (degree, id) or, under GM_T6_AS_NUMBERED, the graph as given; `walk_facts` restates
for one of the two, from the CSR alone, how the walk is cut: the neighbours below every centre (one task up to the one-task limit, a
task per range beyond), the keys of every row inside every range of ids (flattened below the long-row limit, strided by the wave from
it on), which ranges a centre uses.  A cell names the copy its condition holds on; the tests assert the condition against the constants
the library exports (gm_constant), handed in as `consts`: "range", "one_task", "long_row".

Conditions on the inputs of every planted cell (input_conditions; asserted in tests/test_rect_local_host.py): at least 32 distinct
non-zero entry values, at least half of the entries between two core vertices non-zero, both directions of an edge equal."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


def _graph(nv, s, d):
    from graphminer_amd.graph import Graph

    s, d = np.asarray(s, dtype=np.uint64), np.asarray(d, dtype=np.uint64)
    assert bool((s != d).all())
    keys = np.unique(np.concatenate([(s << np.uint64(32)) | d, (d << np.uint64(32)) | s]))
    assert keys.size == 2 * s.size, "an edge was planted twice"
    rp = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount((keys >> np.uint64(32)).astype(np.int64), minlength=nv), out=rp[1:])
    return Graph(row_ptr=rp, col_idx=(keys & np.uint64(0xFFFFFFFF)).astype(np.int32), name="planted_squares")


def renumbered(g, newid):
    """the same graph with vertex v called newid[v] (rows ascending again)"""
    newid = np.asarray(newid, dtype=np.int64)
    src = np.repeat(np.arange(g.V(), dtype=np.int64), np.diff(g.row_ptr))
    col = g.col_idx.astype(np.int64)
    half = src < col
    return _graph(g.V(), newid[src[half]], newid[col[half]])


def shuffled(g, seed):
    """(the graph under a seeded random numbering, newid)"""
    newid = np.random.default_rng(seed).permutation(g.V())
    assert not np.array_equal(newid, np.arange(g.V()))
    return renumbered(g, newid), newid


def entries_to(g, newid, values):
    """per-entry values of g carried to the entry order of renumbered(g, newid)"""
    newid = np.asarray(newid, dtype=np.int64)
    src = np.repeat(np.arange(g.V(), dtype=np.int64), np.diff(g.row_ptr))
    order = np.argsort((newid[src] << 32) | newid[g.col_idx.astype(np.int64)], kind="stable")
    return np.asarray(values)[order]


class Builder:
    """collects the edges of a planted graph; ids are handed out in the order of the calls, the leaves last"""

    def __init__(self, seed):
        self.seed, self.n, self.blocks, self.s, self.d = seed, 0, 0, [], []

    def add(self, k):
        ids = np.arange(self.n, self.n + k, dtype=np.int64)
        self.n += k
        return ids

    def _rng(self):
        self.blocks += 1
        return np.random.default_rng([self.seed, self.blocks])  # a stream of its own per block

    def gnp(self, b, p):
        ids, rng = self.add(b), self._rng()
        i, j = np.triu_indices(b, 1)
        m = rng.random(i.size) < p
        self.s.append(ids[i[m]])
        self.d.append(ids[j[m]])
        return ids

    def bip(self, a, b, p):
        left, right, rng = self.add(a), self.add(b), self._rng()
        m = rng.random((a, b)) < p
        i, j = np.nonzero(m)
        self.s.append(left[i])
        self.d.append(right[j])
        return left, right

    def join(self, v, ids):
        ids = np.asarray(ids, dtype=np.int64)
        self.s.append(np.full(ids.size, int(v), dtype=np.int64))
        self.d.append(ids)

    def degrees(self):
        s, d = np.concatenate(self.s), np.concatenate(self.d)
        return np.bincount(s, minlength=self.n) + np.bincount(d, minlength=self.n)

    def pad(self, ids, target):
        """private leaves bring every vertex of `ids` to the degree target[i] (at least the degree it has)"""
        ids, target = np.asarray(ids, dtype=np.int64), np.asarray(target, dtype=np.int64)
        need = target - self.degrees()[ids]
        assert bool((need >= 0).all()), "a vertex has more neighbours than the degree asked for"
        leaves = self.add(int(need.sum()))
        self.s.append(np.repeat(ids, need))
        self.d.append(leaves)
        return leaves

    def graph(self, order=None):
        """the Graph; order: the pieces of ids in the order in which they are to be numbered (every id once), default as handed out"""
        s, d = np.concatenate(self.s), np.concatenate(self.d)
        newid = np.arange(self.n, dtype=np.int64)
        if order is not None:
            seq = np.concatenate([np.asarray(o, dtype=np.int64) for o in order])
            assert np.array_equal(np.sort(seq), np.arange(self.n))
            newid[seq] = np.arange(self.n)
        return _graph(self.n, newid[s], newid[d]), newid


def degree_copy(g):
    """the copy numbered ascending in (degree, id), as the library makes it: (Graph, newid)"""
    deg = np.diff(g.row_ptr)
    newid = np.empty(g.V(), dtype=np.int64)
    newid[np.lexsort((np.arange(g.V()), deg))] = np.arange(g.V())
    return renumbered(g, newid), newid


@dataclass
class Facts:
    idx0: np.ndarray                                    # per vertex: its neighbours below it
    llens: set = field(default_factory=set)             # every number of keys a row of a centre has inside one range
    tail_hits: set = field(default_factory=set)         # (centre of a task per range, llen) of the strided rows whose LAST key has c >= 2
    head_hits: set = field(default_factory=set)         # ... whose FIRST key has c >= 2
    all_short_batch: bool = False                       # a wave whose rows are all flattened, at least two of them with a key that has c >= 2
    mixed_batch: bool = False                           # a wave with strided and flattened rows, both with a key that has c >= 2
    key_on_first: bool = False                          # a key with c >= 2 on the first id of a range
    key_on_last: bool = False                           # ... on the last id of a range
    cut_at_centre: bool = False                         # a range that ends at the centre, not at its own end, with such a key in it
    gap: bool = False                                   # a centre that uses two ranges and none of those between
    max_ranges_used: int = 0                            # the most ranges one centre has keys with c >= 2 in
    spokes_from_tasks: int = 0                          # per-range centres: the most ranges in which ONE row has a key with c >= 2


def walk_facts(g, consts, rng=None):
    """how the walk of rect_local_kernel is cut on g AS NUMBERED, with ranges of `rng` ids (default: consts["range"])"""
    W = int(rng or consts["range"])
    T, L = int(consts["one_task"]), int(consts["long_row"])
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), g.col_idx.astype(np.int64)
    nv = g.V()
    src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(rp))
    idx0 = np.bincount(src[col < src], minlength=nv)
    f = Facts(idx0)
    for v0 in np.flatnonzero(idx0 >= 2):
        rows = col[rp[v0]:rp[v0] + idx0[v0]]
        lens = rp[rows + 1] - rp[rows]
        first = np.zeros(rows.size, dtype=np.int64)
        np.cumsum(lens[:-1], out=first[1:])
        idx = np.arange(int(lens.sum()), dtype=np.int64) + np.repeat(rp[rows] - first, lens)
        i = np.repeat(np.arange(rows.size), lens)
        x = col[idx]
        below = x < v0
        i, x = i[below], x[below]
        if x.size == 0:
            continue
        k = x // W
        c = np.bincount(x, minlength=v0)[x]
        hit = c >= 2
        pair, inv, llen = np.unique(i * (nv // W + 1) + k, return_inverse=True, return_counts=True)
        pi, pk = pair // (nv // W + 1), pair % (nv // W + 1)
        f.llens.update(llen.tolist())
        pair_hit = np.bincount(inv, weights=hit, minlength=pair.size) > 0
        last_hit = np.zeros(pair.size, dtype=bool)  # (the keys of a pair are consecutive and ascending: the last one is the last of its run)
        ends = np.flatnonzero(np.r_[inv[1:] != inv[:-1], True])
        last_hit[inv[ends]] = hit[ends]
        first_hit = np.zeros(pair.size, dtype=bool)
        starts = np.flatnonzero(np.r_[True, inv[1:] != inv[:-1]])
        first_hit[inv[starts]] = hit[starts]
        hub = bool(idx0[v0] > T)
        f.tail_hits.update((hub, n) for n in llen[(llen >= L) & last_hit].tolist())
        f.head_hits.update((hub, n) for n in llen[(llen >= L) & first_hit].tolist())
        # the 64 rows a wave takes together: a batch of consecutive rows (a task per range), or the rows = w mod 4 (one task: the
        # one-task limit is four waves of 64 rows)
        batch = pi // 64 if hub else pi % (T // 64)
        wave_walk = batch * (nv // W + 1) + pk
        for key in np.unique(wave_walk):
            m = wave_walk == key
            short, strided = int((m & pair_hit & (llen < L)).sum()), int((m & pair_hit & (llen >= L)).sum())
            f.all_short_batch |= short >= 2 and not bool((m & (llen >= L)).any())
            f.mixed_batch |= short >= 1 and strided >= 1
        f.key_on_first |= bool((hit & (x % W == 0)).any())
        f.key_on_last |= bool((hit & (x % W == W - 1)).any())
        f.cut_at_centre |= v0 % W != 0 and bool((hit & (k == v0 // W)).any())
        used = np.unique(k)
        f.gap |= bool((np.diff(used) > 1).any())
        f.max_ranges_used = max(f.max_ranges_used, int(np.unique(k[hit]).size))
        if hub and pair_hit.any():
            f.spokes_from_tasks = max(f.spokes_from_tasks, int(np.bincount(pi[pair_hit]).max()))
    return f


def input_conditions(g, ent):
    """(distinct non-zero entry values, non-zero fraction of the entries between two vertices of degree >= 2, both directions equal)"""
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), g.col_idx.astype(np.int64)
    deg = np.diff(rp)
    src = np.repeat(np.arange(g.V(), dtype=np.int64), deg)
    core = (deg[src] >= 2) & (deg[col] >= 2)
    rev = np.argsort((col << 32) | src, kind="stable")  # the entry (v, u) of every entry (u, v): the entries are sorted by (u, v)
    return int(np.unique(ent[ent > 0]).size), float((ent[core] > 0).mean()), bool(np.array_equal(ent[rev], ent))


# ---- the cells ---------------------------------------------------------------------------------------------------------------------------
def centre_rows(m, seed=1):
    """A hub above every other vertex in the degree order with exactly m neighbours (all below it): a whole G(120, .3), the left half of a
    bipartite G(100, 100, .25) and the first m - 220 vertices of a G(m - 212, .4).  The block vertices carry 0 .. 6 leaves each; the hub has
    none.  On the degree copy the hub is the centre of the cycles through it and has m rows."""
    assert m >= 230
    b = Builder(seed)
    b1 = b.gnp(120, 0.3)
    left, right = b.bip(100, 100, 0.25)
    b3 = b.gnp(m - 212, 0.4)
    hub = b.add(1)
    b.join(hub[0], np.concatenate([b1, left, b3[:m - 220]]))
    blockv = np.concatenate([b1, left, right, b3])
    b.pad(blockv, b.degrees()[blockv] + np.arange(blockv.size) % 7)
    g, _ = b.graph()
    assert int(np.diff(g.row_ptr).max()) == m and int(np.argmax(np.diff(g.row_ptr))) == hub[0]
    return g


def row_lengths(consts, seed=2):
    """Two hubs over row vertices with chosen numbers of keys, numbered pool < leaves < rows < hub2 < hub1 so that AS NUMBERED everything
    but its hub lies below a row vertex: a row vertex of degree n + 1 is a row of n keys.  Every row vertex is joined to one hub and to a
    whole pool block (G(12, .5), or one side of a bipartite G(8, 8, .5)) and padded with leaves; a row of a special length to two blocks,
    one numbered below the leaves and one above them, so that as numbered its first and its last key are both credited.
      hub1  one_task + 44 rows (a task per range): five batches of 64 rows, the last one holds the six special lengths
      hub2  200 rows (one task): the special lengths on rows of three of the four waves
    special lengths: long_row - 1, long_row, long_row + 1 and 4 long_row - 1, 4 long_row, 4 long_row + 1 (the unroll of the strided rows)."""
    T, L = int(consts["one_task"]), int(consts["long_row"])
    special = [L - 1, L, L + 1, 4 * L - 1, 4 * L, 4 * L + 1]
    b = Builder(seed)
    pool = [b.gnp(12, 0.5) for _ in range(10)]
    for _ in range(4):
        pool.extend(b.bip(8, 8, 0.5))
    n1, n2 = T + 44, 200
    short1 = [2 + (5 * j) % 11 for j in range(n1 - 6)]  # (2 .. 12 keys: the whole graph stays inside one default range)
    short2 = [2 + (7 * j) % 11 for j in range(n2 - 6)]
    len1 = short1 + special
    len2 = short2[:n2 - 8] + special[:3] + short2[n2 - 8:n2 - 7] + special[3:] + short2[n2 - 7:]  # specials on rows = 0, 1, 2 mod 4
    assert (n2 - 8) % 4 == 0 and len(len1) == n1 and len(len2) == n2
    rows1, rows2, hub2, hub1 = b.add(n1), b.add(n2), b.add(1), b.add(1)
    b.join(hub1[0], rows1)
    b.join(hub2[0], rows2)
    for rows, lens in ((rows1, len1), (rows2, len2)):
        for j, (r, n) in enumerate(zip(rows, lens)):
            at = 5 * j + (0 if rows is rows1 else 7)
            blk = pool[at % len(pool)] if n < L - 1 else np.concatenate([pool[at % len(pool)], pool[(at + 1) % len(pool)]])
            b.join(r, blk[:min(n, blk.size)])
    rows = np.concatenate([rows1, rows2])
    leaves = b.pad(rows, np.asarray(len1 + len2) + 1)
    g, _ = b.graph(order=[np.concatenate(pool[0::2]), leaves, np.concatenate(pool[1::2]), rows1, rows2, hub2, hub1])
    assert g.V() <= int(consts["range"])
    return g


def three_ranges(consts, seed=3):
    """More than two default ranges of ids: six G(60, .3) and three bipartite G(50, 50, .2), six joiners on whole and half blocks, every
    core vertex padded to a degree of 26 .. 42 and then a seeded random numbering, so that AS NUMBERED the core is spread over every range;
    on the degree copy the core sits in the top range and the leaves below are ends that are reached once."""
    b = Builder(seed)
    blocks = [b.gnp(60, 0.3) for _ in range(6)]
    for _ in range(3):
        blocks.extend(b.bip(50, 50, 0.2))
    core = np.concatenate(blocks)
    joiners = b.add(6)
    for j, v in enumerate(joiners):
        b.join(v, np.concatenate([blocks[j], blocks[(j + 5) % len(blocks)][:25]]))
    deg = b.degrees()[core]
    b.pad(core, np.maximum(deg, 26 + np.arange(core.size) % 17))
    g, _ = b.graph()
    assert g.V() > 2 * int(consts["range"])
    return shuffled(g, seed)[0]


def k2n(n):
    """K_{2, n}, the two hubs last"""
    side = np.arange(n, dtype=np.int64)
    return _graph(n + 2, np.concatenate([side, side]), np.concatenate([np.full(n, n), np.full(n, n + 1)]))


def windmill(n, spokes):
    """n triangles that share one vertex (any two vertices have exactly one common neighbour: no 4-cycle), `spokes` further leaves on
    the shared vertex and a path behind every second triangle vertex: long rows, nothing to count"""
    hub = 0
    a = 1 + 2 * np.arange(n, dtype=np.int64)
    leaves = 1 + 2 * n + np.arange(spokes, dtype=np.int64)
    tails = 1 + 2 * n + spokes + np.arange(n, dtype=np.int64)
    s = np.concatenate([np.full(n, hub), np.full(n, hub), a, np.full(spokes, hub), a])
    d = np.concatenate([a, a + 1, a + 1, leaves, tails])
    return _graph(1 + 3 * n + spokes, s, d)


# ---- what every GPU cell has to show before its comparison means something ------------------------------------------------------------
def constants():
    """the constants at which rect_local_kernel changes path, read from the library (gm_constant: a host call, no GPU)"""
    import ctypes as C

    from graphminer_amd import _lib

    lib, out = _lib.load(), {}
    for key, name in (("range", "rect_local_range"), ("one_task", "rect_local_one_task"), ("long_row", "rect_local_long_row")):
        v = C.c_int64(0)
        _lib.check(lib.gm_constant(name.encode(), C.byref(v)), "gm_constant")
        out[key] = int(v.value)
    return out


SMALL_RANGE = 16  # GM_RECT_LOCAL_RANGE of the small-range cells
CELLS = ("centre-1", "centre+0", "centre+1", "rows", "small-range", "three-ranges")  # the planted cells (input_conditions holds for each)


def cell_graph(name, consts):
    T = int(consts["one_task"])
    if name.startswith("centre"):
        return centre_rows(T + int(name[6:]))
    if name == "small-range":
        return centre_rows(T + 1, seed=4)
    return {"rows": row_lengths, "three-ranges": three_ranges}[name](consts)


def cell_path(name, g, consts):
    """{claim: holds} -- what places the cell on the path it is named for, on the copy the claim names"""
    T, L, W = int(consts["one_task"]), int(consts["long_row"]), int(consts["range"])
    if name.startswith("centre"):
        m = T + int(name[6:])
        f = walk_facts(degree_copy(g)[0], consts)
        top = int(f.idx0.max())
        others = int(np.sort(f.idx0)[-2])
        return {f"degree copy: the largest centre has {m} rows (got {top})": top == m,
                f"degree copy: every other centre is one task ({others} <= {T})": others <= T,
                f"degree copy: {'a task per range' if m > T else 'one task'}": (top > T) == (m > T)}
    if name == "rows":
        special = {L - 1, L, L + 1, 4 * L - 1, 4 * L, 4 * L + 1}
        out = {}
        for label, h in (("as numbered", g), ("degree copy", degree_copy(g)[0])):
            f = walk_facts(h, consts)
            out[f"{label}: rows of {sorted(special)} keys inside one range"] = special <= f.llens
            strided = sorted(special - {L - 1})
            for hub in (True, False) if label == "as numbered" else (True,):
                kind = "a task per range" if hub else "one task"
                out[f"{label}, {kind}: strided rows of {strided} keys whose last key is credited"] = {(hub, n) for n in strided} <= f.tail_hits
                if label == "as numbered":
                    out[f"{label}, {kind}: ... whose first key is credited"] = {(hub, n) for n in strided} <= f.head_hits
            out[f"{label}: a wave of flattened rows only, and a wave with both kinds"] = f.all_short_batch and f.mixed_batch
            out[f"{label}: the largest centre has a task per range ({int(f.idx0.max())} rows)"] = int(f.idx0.max()) == T + 44
        f = walk_facts(g, consts)
        out["as numbered: the second hub is one task of 200 rows"] = int(f.idx0[g.V() - 2]) == 200 <= T and int(f.idx0[g.V() - 1]) == T + 44
        return out
    if name == "small-range":
        f = walk_facts(degree_copy(g)[0], consts, SMALL_RANGE)
        return {"degree copy, 16 ids per range: credited keys on the first and on the last id of a range": f.key_on_first and f.key_on_last,
                "... a range cut at its centre": f.cut_at_centre, "... a centre with an unused range between two used ones": f.gap,
                f"... a centre of a task per range ({int(f.idx0.max())} rows) whose rows are credited from several tasks "
                f"({f.spokes_from_tasks})": int(f.idx0.max()) > T and f.spokes_from_tasks >= 2,
                f"about 1,024 vertices ({g.V()})": 512 <= g.V() <= 2048}
    if name == "three-ranges":
        f, fd = walk_facts(g, consts), walk_facts(degree_copy(g)[0], consts)
        return {f"more than two ranges of ids ({g.V()} vertices, {W} per range)": g.V() > 2 * W,
                f"as numbered: one centre is credited in {f.max_ranges_used} ranges": f.max_ranges_used >= 3,
                "degree copy: a centre walks ranges below the one it is credited in": fd.gap or fd.max_ranges_used >= 1}
    raise KeyError(name)
