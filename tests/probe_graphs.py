"""Probe graphs: symmetric graphs whose STREAMED LISTS are known key by key (test helper, numpy only; imported by
tests/test_probe_graphs_host.py and tests/test_gpu_probe_lists.py).

The list-streaming kernels (tch_kernel, the position set of the 4-clique build, the edge supports, the listing kernels, the hashed rows,
the flattened passes) go wrong at exact places: the end of a list that is no multiple of 64 keys, the last tile group of a long list, the
switch from flattened to one list at a time, a mark window that fills exactly, the host tag of the key stream, the row salt of a chunk's
shared hash table, the surplus list when it is full.  A total on a random graph says that some key was dropped somewhere; these graphs put
ONE list of a chosen length against ONE host row, with the matches at chosen positions and non-members everywhere else, so that a wrong
count names a length and a position.

The trick all families share: a pool of HUBS that is an independent set (but for the planted hub-hub edges of `k4`), each padded with
private leaves to one common degree D above every gadget vertex's degree.  Under the reference's orientation (lower degree -> higher
degree, ties by id) every gadget vertex then points AT the hubs, hub rows are empty, a leaf's only task streams an empty row, the hubs keep
their relative order in the topological copy (ids by (degree, old id)), and the only triangles are the planted ones.

Who hosts (csrc/gm_tasks.hip task_walk_rows): the edge s -> t of the DAG is hosted by s when tail >= d+(t), else by t; tail = d+(s) as
numbered, the entries of N+(s) behind t on the topological copy.  The host's row is staged, the other list is streamed.

Families (ids: gadget vertices, then hubs, then -- `batch` only -- the high mids, then leaves):
  single  one list, one host.  Gadget = v - u joined by an edge (v < u), u on A hubs R, v on L <= A hubs S spread over the hub range; the
          matches S ^ R are the elements of S at the positions P, the rest of R comes from hubs outside S.  v -> u, row(v) = {u} + S,
          row(u) = R.  With L + 1 < A, u hosts as numbered and streams row(v): L + 1 keys, u first, the matches at P + 1; on the
          topological copy it streams the tail of L keys with the matches at P.  The gadgets with A = L and A = L + 1 sit at the tie of
          the host rule.  Triangles of a gadget = |P| = support of (u, v).
  batch   full batches of equal lists (as numbered).  u has a DAG row of M = 1024 (2048) mids; every mid has a DAG row of exactly `ell`
          keys, a third of them with one match at position 0 (a later low mid), a third at position ell - 1 (a later high mid), a third
          none.  u hosts all M tasks, each streams `ell` keys: batch offsets are multiples of ell whatever the order of arrival.
  salt    >= 600 consecutive hosts with rows of 3 or 4 hubs, alternating between two disjoint hub sets, rows 128 apart different; the
          partner's hubs by index mod 3: one of the host's own row (1 triangle), the row staged for the NEXT host (0), one of each (1).
  surplus two single gadgets whose host rows hold 131 / 132 ids of one bucket of tch_kernel's table (see surplus()).
  k4      single gadgets with two matches whose hubs are joined: one 4-clique {v, u, h1, h2} each, and a decoy edge that makes none.

Every expected value a Probe carries is confirmed against the CPU oracle by tests/test_probe_graphs_host.py."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

S1024_L = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 447, 448, 449, 511, 512, 513, 575, 576,
           577, 639, 640, 641, 703, 704, 705, 767, 768, 769, 1022, 1023)
S2048_L = S1024_L + (1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 1793, 2045, 2046)
PATTERNS = ("none", "first", "last", "middle", "tiles")
BATCH_ELLS = (16, 32, 33, 64, 127, 128, 129, 255, 256, 257, 383)
K4_L = (64, 65, 257, 513, 1025)
SALT_HOSTS = 640
# salt: hubs beyond the 24 in use only carry leaves.  A launch halves its chunk target (1024 entries) until a graph has 2 * 7 chunks per
# CU (csrc/gm_launch.hip run_pattern): 256 rows of 3 .. 4 keys stay one chunk only on a DAG of more than 14 * 256 CUs * 1024 entries
SALT_HUBS, SALT_D = 2100, 2000
MUL = 0x9E3779B1  # csrc/gm_tch.hip kTchMul


def positions(L: int, pattern: str) -> np.ndarray:
    """the match positions P inside S (0 .. L-1) of a pattern"""
    if pattern == "none":
        return np.zeros(0, np.int64)
    if pattern == "first":
        return np.array([0])
    if pattern == "last":
        return np.array([L - 1])
    if pattern == "middle":
        return np.array([L // 2])
    if pattern == "tiles":  # both the L-key and the (L + 1)-key view have matches on either side of every 64-key tile edge
        k = np.arange(L)
        return k[np.isin(k % 64, (0, 1, 62, 63))]
    raise ValueError(pattern)


@dataclass
class Gadget:
    family: str
    label: str        # what a failure prints: family, L, A, pattern
    u: int            # the vertex with the longer row (single: the host with L + 1 < A; batch: the host; salt: row of 3 - 4 hubs -- as
                      # numbered it hosts only with 1 + |S| < |R|, else its partner v does and streams u's row)
    v: int            # its partner (batch: -1)
    L: int            # keys of S (batch: ell)
    A: int            # keys of row(u)
    S: np.ndarray     # v's hubs, ascending ids (batch / salt: unused or the partner's hubs)
    R: np.ndarray     # u's hubs, ascending ids
    P: np.ndarray     # positions inside S of the matches
    tri: int          # triangles of this gadget
    cliques4: int = 0
    extra: dict = field(default_factory=dict)


class Probe:
    """a probe graph and what is known about it.  graph: graphminer_amd Graph; hubs: ids; gadgets; triangles: int32[T, 3], rows a < b < c,
    sorted; cliques4: int32[K, 4] likewise; owner[x]: the gadget of core vertex x (-1: hub)"""

    def __init__(self, name, graph, n_core, hubs, gadgets, triangles, cliques4, owner, D):
        self.name, self.graph, self.n_core, self.hubs, self.gadgets, self.D = name, graph, n_core, hubs, gadgets, D
        self.triangles = _sorted_rows(np.asarray(triangles, dtype=np.int32).reshape(-1, 3))
        self.cliques4 = np.sort(np.asarray(cliques4, dtype=np.int32).reshape(-1, 4), axis=1)
        self.owner = owner
        for a in (self.triangles, self.cliques4, self.hubs, self.owner):
            a.setflags(write=False)

    @property
    def tri_total(self) -> int:
        return len(self.triangles)

    def entry_of(self, a, b) -> np.ndarray:
        """CSR entry index of (a, b), arrays; asserted present"""
        g = self.graph
        nv = g.V()
        if not hasattr(self, "_keys"):
            src = np.repeat(np.arange(nv, dtype=np.int64), np.diff(g.row_ptr))
            self._keys = src * nv + g.col_idx  # ascending: rows ascending, ids inside a row ascending
        want = np.asarray(a, np.int64) * nv + np.asarray(b, np.int64)
        pos = np.searchsorted(self._keys, want)
        assert pos.size == 0 or (pos.max() < self._keys.size and (self._keys[pos] == want).all()), "an expected edge is not in the graph"
        return pos

    def supports(self) -> np.ndarray:
        """uint32 per CSR entry: the triangles its edge lies in (both directions carry it)"""
        t = self.triangles.astype(np.int64)
        sup = np.zeros(self.graph.E(), dtype=np.int64)
        for i, j in ((0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)):
            np.add.at(sup, self.entry_of(t[:, i], t[:, j]), 1)
        return sup.astype(np.uint32)

    def vertex_triangles(self) -> np.ndarray:
        return np.bincount(self.triangles.reshape(-1), minlength=self.graph.V()).astype(np.uint64)

    def diamonds(self) -> int:
        """pairs of triangles that share an edge: sum C(support, 2) over the edges, a 4-clique holds six of them -- what the oracle's diamond
        counts (confirmed against it in the host test)"""
        s = self.supports().astype(np.int64)
        return int((s * (s - 1) // 2).sum() // 2)

    def wedges(self) -> int:
        """open wedges: sum C(d, 2) - 3 T"""
        d = np.diff(self.graph.row_ptr).astype(np.int64)  # (degrees of a few thousand, 2^24 vertices: far inside 64 bits)
        return int((d * (d - 1) // 2).sum()) - 3 * self.tri_total

    def gadget_of_entry(self, e: int) -> str:
        """the label of the gadget an entry belongs to (a failure's message)"""
        g = self.graph
        s = int(np.searchsorted(g.row_ptr, e, side="right") - 1)
        d = int(g.col_idx[e])
        for x in (s, d):
            if x < self.n_core and self.owner[x] >= 0:
                return self.gadgets[int(self.owner[x])].label
        return f"no gadget (entry {s} - {d})"

    def gadget_of_vertex(self, x: int) -> str:
        if x < self.n_core and self.owner[x] >= 0:
            return self.gadgets[int(self.owner[x])].label
        return f"no gadget (vertex {x})"


def _sorted_rows(t):
    t = np.sort(t, axis=1)
    return np.ascontiguousarray(t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]) if len(t) else t


def _assemble(n_core: int, s, d, target_deg: np.ndarray, id_space: int | None = None, leaf_base: int | None = None):
    """The graph of the core edges (s, d) plus private leaves that bring every core vertex x with target_deg[x] > 0 to that degree.  Leaf
    ids follow the core (or start at leaf_base); a padded vertex's leaves are one id range above every core id, so its row is its core row
    followed by the range -- the CSR is put together without a sort of all entries."""
    from graphminer_amd.graph import Graph
    from graphminer_amd.rmat import csr_from_pairs

    core = csr_from_pairs(n_core, np.concatenate(s).astype(np.uint64), np.concatenate(d).astype(np.uint64))
    cdeg = np.diff(core.row_ptr)
    nleaf = np.where(target_deg > 0, target_deg - cdeg, 0)
    assert (nleaf >= 0).all(), "a padded vertex has more core neighbours than its target degree"
    leaf_base = n_core if leaf_base is None else leaf_base
    assert leaf_base >= n_core
    n_leaves = int(nleaf.sum())
    nv = max(leaf_base + n_leaves, id_space or 0)
    deg = np.zeros(nv, dtype=np.int64)
    deg[:n_core] = cdeg + nleaf
    deg[leaf_base:leaf_base + n_leaves] = 1
    rp = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(deg, out=rp[1:])
    col = np.empty(int(rp[-1]), dtype=np.int32)
    csrc = np.repeat(np.arange(n_core, dtype=np.int64), cdeg)
    col[rp[csrc] + (np.arange(core.col_idx.size) - core.row_ptr[csrc])] = core.col_idx
    owner = np.repeat(np.arange(n_core, dtype=np.int64), nleaf)               # the core vertex of every leaf, ascending
    first = np.zeros(n_core + 1, dtype=np.int64)
    np.cumsum(nleaf, out=first[1:])
    k = np.arange(n_leaves, dtype=np.int64) - first[owner]                    # its rank among that vertex's leaves
    col[rp[owner] + cdeg[owner] + k] = (leaf_base + np.arange(n_leaves)).astype(np.int32)
    col[rp[leaf_base:leaf_base + n_leaves]] = owner.astype(np.int32)
    return Graph(row_ptr=rp, col_idx=col, name="probe")


def _spread(pool: np.ndarray, n: int, shift: int = 0) -> np.ndarray:
    """n distinct elements of the ascending pool, spread over all of it (rotated by shift), ascending"""
    assert 0 <= n <= pool.size
    if n == 0:
        return pool[:0]
    return np.sort(pool[(np.arange(n, dtype=np.int64) * pool.size // n + shift) % pool.size])


def _single_sets(hubs: np.ndarray, L: int, A: int, P: np.ndarray, shift: int):
    S = _spread(hubs, L, shift)
    outside = np.setdiff1d(hubs, S, assume_unique=True)
    R = np.sort(np.concatenate([S[P], _spread(outside, A - len(P), shift)]))
    assert len(np.unique(R)) == A and np.array_equal(np.intersect1d(S, R), S[P])
    return S, R


def _single_specs(lengths, A):
    specs = [(L, A, pat) for L in lengths for pat in PATTERNS]
    for L in lengths:
        if L < A:
            specs += [(L, L, "last"), (L, L + 1, "last")]  # the tie of the host rule (tail >= d+(t))
    return specs


def _single_graph(name, n_hubs, D, specs):
    ng = len(specs)
    hubs = np.arange(2 * ng, 2 * ng + n_hubs, dtype=np.int64)
    n_core = 2 * ng + n_hubs
    owner = np.full(n_core, -1, dtype=np.int32)
    s, d, gadgets, tris = [], [], [], []
    for i, (L, A, pat) in enumerate(specs):
        v, u = 2 * i, 2 * i + 1
        owner[v] = owner[u] = i
        P = positions(L, pat)
        S, R = _single_sets(hubs, L, A, P, 37 * i)
        s += [np.array([v]), np.full(L, v), np.full(A, u)]
        d += [np.array([u]), S, R]
        tris += [(v, u, int(h)) for h in S[P]]
        gadgets.append(Gadget("single", f"{name} L={L} A={A} {pat}", u, v, L, A, S, R, P, len(P)))
    target = np.zeros(n_core, dtype=np.int64)
    target[hubs] = D
    graph = _assemble(n_core, s, d, target)
    return Probe(name, graph, n_core, hubs, gadgets, tris, [], owner, D)


SINGLE = {"s1024": (2048, 1100, S1024_L, 1023), "s2048": (4096, 2100, S2048_L, 2047)}  # hubs, D, lengths, A
SLICE_PATTERNS = PATTERNS + ("tie",)
# Classes of L by the way tch_kernel streams the list: the key stream (<= 32 keys, GM_TC_INLINE_MAX), the flattened pass (33 .. 383), one list at a
# time (>= kTchLongList = 384).  A gadget streams L keys on the topological copy and L + 1 as numbered (the tie gadgets L or L + 1 either
# way), so "stream", "flat" and "long" hold the L whose two views agree, and "edge" the two that straddle a switch: 32 and 383.
SLICE_CLASSES = {"stream": lambda L: L + 1 <= 32, "flat": lambda L: 33 <= L and L + 1 <= 383, "long": lambda L: L >= 384,
                 "edge": lambda L: L in (32, 383)}


@functools.lru_cache(maxsize=2)
def single(name: str, pattern: str | None = None, cls: str | None = None) -> Probe:
    """s1024: 2048 hubs, D = 1100, A = 1023 (the longest DAG row is 1024: tch_kernel<1024>); s2048: 4096 hubs, D = 2100, A = 2047.
    With (pattern, cls): the SLICE of the graph that keeps the gadgets of one match pattern ("tie": those at the tie of the host rule) and
    one class of lengths -- the same hubs, the same rows, so that a wrong TOTAL names pattern and class."""
    n_hubs, D, lengths, A = SINGLE[name]
    specs = _single_specs(lengths, A)
    if pattern is not None:
        specs = [(L, a, pat) for L, a, pat in specs if SLICE_CLASSES[cls](L) and ((a != A) if pattern == "tie" else (a == A and pat == pattern))]
        name = f"{name}:{pattern}:{cls}"
        assert specs
    return _single_graph(name, n_hubs, D, specs)


@functools.lru_cache(maxsize=None)
def k4() -> Probe:
    """single gadgets with two matches, at (first, last) and at (63, 64) ((62, 63) for L = 64), for every L of K4_L; A = 1023, and 1026 for
    L = 1025 (the 2048-entry stage).  The two matching hubs h1 < h2 are joined: the 4-clique {v, u, h1, h2}; h1 is also joined to a decoy
    hub that is in S but not in R: the triangle (v, h1, decoy), no clique.  A hub with a hub-hub edge belongs to ONE gadget (another
    gadget on both its ends would close triangles nobody planted), so the hub ids are three reserved blocks -- low, middle, high -- around
    two general pools, and a gadget's S takes its general hubs from the pools so that its reserved hubs get the ranks wanted."""
    specs = []
    for L in K4_L:
        A = 1023 if L < 1023 else L + 1
        specs += [(L, A, "first+last"), (L, A, "adjacent")]
    ng, D = len(specs), 1100
    blk = 2 * ng
    base = 2 * ng
    low = np.arange(base, base + blk, dtype=np.int64)
    pool1 = np.arange(low[-1] + 1, low[-1] + 1 + 200, dtype=np.int64)
    mid = np.arange(pool1[-1] + 1, pool1[-1] + 1 + blk, dtype=np.int64)
    pool2 = np.arange(mid[-1] + 1, mid[-1] + 1 + 2000, dtype=np.int64)
    high = np.arange(pool2[-1] + 1, pool2[-1] + 1 + blk, dtype=np.int64)
    hubs = np.arange(base, high[-1] + 1, dtype=np.int64)
    general = np.concatenate([pool1, pool2])
    n_core = int(high[-1]) + 1
    owner = np.full(n_core, -1, dtype=np.int32)
    s, d, gadgets, tris, k4s = [], [], [], [], []
    for i, (L, A, pat) in enumerate(specs):
        v, u = 2 * i, 2 * i + 1
        owner[v] = owner[u] = i
        if pat == "first+last":
            h1, h2, decoy = low[2 * i], high[2 * i], mid[2 * i]
            Sg = _spread(general, L - 3, 37 * i)
            P = np.array([0, L - 1])
        else:
            p0 = 63 if L > 64 else 62
            h1, h2, decoy = mid[2 * i], mid[2 * i + 1], low[2 * i]
            Sg = np.concatenate([_spread(pool1, p0 - 1, 11 * i), _spread(pool2, L - p0 - 2, 37 * i)])
            P = np.array([p0, p0 + 1])
        S = np.sort(np.concatenate([Sg, [h1, h2, decoy]]))
        assert len(S) == L and S[P[0]] == h1 and S[P[1]] == h2
        R = np.sort(np.concatenate([[h1, h2], _spread(np.setdiff1d(general, Sg, assume_unique=True), A - 2, 37 * i)]))
        s += [np.array([v, h1, h1]), np.full(L, v), np.full(A, u)]
        d += [np.array([u, h2, decoy]), S, R]
        tris += [(v, u, h1), (v, u, h2), (v, h1, h2), (u, h1, h2), (v, h1, decoy)]
        k4s.append((v, u, h1, h2))
        gadgets.append(Gadget("k4", f"k4 L={L} A={A} {pat} at {P.tolist()}", u, v, L, A, S, R, P, 5, 1, {"decoy": int(decoy)}))
    target = np.zeros(n_core, dtype=np.int64)
    target[hubs] = D
    return Probe("k4", _assemble(n_core, s, d, target), n_core, hubs, gadgets, tris, k4s, owner, D)


@functools.lru_cache(maxsize=1)
def batch(M: int, ell: int) -> Probe:
    """u = id 0 with a DAG row of the M mids; low mids 1 .. M/2, the hubs, the high mids.  Mid j (0 .. M-1 in id order): low j with
    j % 3 in (0, 1) points at the next low mid (match at position 0 of its row), low j with j % 3 == 2 at the high mid M/2 + j, high j
    with j % 3 == 0 at the next high mid (match at position ell - 1); the others, and those without a later mid, have no match.  The hubs
    of two adjacent mids come from different residue classes mod 4: no triangle but (u, m, target)."""
    assert M in (1024, 2048) and 2 <= ell <= 384
    half, n_hubs = M // 2, 4 * 384
    Dm, D = M + 30, M + 70
    hubs = np.arange(1 + half, 1 + half + n_hubs, dtype=np.int64)
    mids = np.concatenate([np.arange(1, 1 + half), np.arange(1 + half + n_hubs, 1 + half + n_hubs + half)]).astype(np.int64)
    n_core = 1 + M + n_hubs
    owner = np.full(n_core, -1, dtype=np.int32)
    owner[0] = 0
    owner[mids] = 0
    tgt = np.full(M, -1, dtype=np.int64)
    for j in range(M):
        if j < half:
            t = j + 1 if j % 3 < 2 else half + j
            tgt[j] = t if (t < half or j % 3 == 2) else -1
        elif j % 3 == 0 and j + 1 < M:
            tgt[j] = j + 1
    s, d, tris = [np.zeros(M, np.int64)], [mids], []
    match_pos = np.full(M, -1, dtype=np.int64)
    for j in range(M):
        nh = ell - (1 if tgt[j] >= 0 else 0)
        cls = (j + (2 if j >= half else 0)) % 4
        s.append(np.full(nh, mids[j]))
        d.append(hubs[cls + 4 * ((7 * j + np.arange(nh)) % 384)])
        if tgt[j] >= 0:
            s.append(np.array([mids[j]]))
            d.append(np.array([mids[tgt[j]]]))
            tris.append((0, int(mids[j]), int(mids[tgt[j]])))
            match_pos[j] = 0 if tgt[j] < half else ell - 1
    target = np.zeros(n_core, dtype=np.int64)
    target[hubs] = D
    target[mids] = Dm
    graph = _assemble(n_core, s, d, target)
    g = Gadget("batch", f"batch M={M} ell={ell}", 0, -1, ell, M, mids, mids, np.flatnonzero(tgt >= 0), len(tris),
               extra={"mids": mids, "target": tgt, "match_pos": match_pos, "Dm": Dm})
    return Probe(f"batch{M}_{ell}", graph, n_core, hubs, [g], tris, [], owner, D)


@functools.lru_cache(maxsize=None)
def salt() -> Probe:
    """partners 0 .. n-1, hosts n .. 2n-1 (n = SALT_HOSTS), two hub sets of 8 and 8 neutral hubs.  Host i takes a = 3 + (i // 2) % 2 hubs of
    set i % 2, cyclically from c(i) = (i // 2 + 3 * (i // 128)) % 8, so that the rows of hosts 128 apart differ in their LAST hub -- the one
    its partner matches.  Partner i has 2 or 3 hubs, by i % 3: 0: the host's last hub and one or two neutral hubs; 1: the
    first two or three hubs of host i + 1's row (the other set, staged beside the host's own row); 2: the host's last hub and the next host's last hub.
    The other SALT_HUBS - 24 hubs have leaves only: they make the graph large enough for chunks of 256 rows (see SALT_HUBS)."""
    n = SALT_HOSTS
    hubs = np.arange(2 * n, 2 * n + SALT_HUBS, dtype=np.int64)
    sets = (hubs[0:8], hubs[8:16])
    neutral = hubs[16:24]
    n_core = 2 * n + SALT_HUBS
    owner = np.full(n_core, -1, dtype=np.int32)

    def row(i):
        a = 3 + (i // 2) % 2
        c = (i // 2 + 3 * (i // 128)) % 8
        return sets[i % 2][(c + np.arange(a)) % 8]  # (in the order taken: the last one is the partner's match)

    s, d, gadgets, tris = [], [], [], []
    for i in range(n):
        v, u = i, n + i
        owner[v] = owner[u] = i
        R = row(i)
        other = row(i + 1) if i + 1 < n else row(i - 1)
        mode = i % 3
        if mode == 0:
            S = np.concatenate([R[-1:], neutral[[i % 8, (i + 3) % 8][: 1 + i % 2]]])
        elif mode == 1:
            S = other[: 2 + (len(R) > 3)]  # (fewer keys than the host's row: v -> u whatever the ids)
        else:
            S = np.array([R[-1], other[-1]])
        match = np.intersect1d(S, R)
        s += [np.array([v]), np.full(len(S), v), np.full(len(R), u)]
        d += [np.array([u]), S, R]
        tris += [(v, u, int(h)) for h in match]
        Ss = np.sort(S)
        gadgets.append(Gadget("salt", f"salt host {i} (id {u}) mode {mode}", u, v, len(S), len(R), Ss, np.sort(R),
                              np.flatnonzero(np.isin(Ss, match)), len(match)))
    target = np.zeros(n_core, dtype=np.int64)
    D = SALT_D
    target[hubs] = D
    return Probe("salt", _assemble(n_core, s, d, target), n_core, hubs, gadgets, tris, [], owner, D)


def one_bucket_ids(count: int, lo: int = 4096) -> np.ndarray:
    """ids in [lo, 2^24) whose products with kTchMul share their top ten bits: one bucket of the 1024-bucket table per row salt"""
    cinv = pow(MUL, -1, 1 << 32)
    t = (np.uint64(5) << np.uint64(22)) + np.arange(1 << 22, dtype=np.uint64)
    x = (t * np.uint64(cinv)) & np.uint64(0xFFFFFFFF)
    pool = np.sort(x[(x < (1 << 24)) & (x >= lo)]).astype(np.int64)
    assert pool.size >= count
    return pool[:count]


SURPLUS_ROWS = (131, 132)
SURPLUS_L = 100


@functools.lru_cache(maxsize=None)
def surplus() -> Probe:
    """The surplus list of tch_kernel's table exactly full, and one over (as numbered only: a renumbering changes the ids).

    csrc/gm_tch.hip, the build of a chunk's table: a bucket has four slots; every further entry of the bucket goes to the surplus list
    (n_ovf + 1 each), and a bucket that got more than four gives up its last slot for the marker, whose entry joins the list too (+ 1).
    A host row of k ids that all fall into ONE bucket therefore leaves n_ovf = (k - 4) + 1 = k - 3: 131 ids -> 128 = kTchOvfCap, the list
    exactly full and still used (fallback only when n_ovf > kTchOvfCap); 132 ids -> 129, the first chunk looked up by bisection instead.
    For the count to be exact the host must be alone in its chunk with its row: the chunk walk restarts every 512 vertices
    (kTableBlock, csrc/gm_tables.hip), so the two hosts get ids 0 and 512, their partners 1024 and 1536 (a partner's own row collides in one
    bucket as well), the leaves start at 2^23 and the hubs -- ids >= 4096 through the inverse of the multiplier -- have empty rows.
    Which four ids stay in the bucket's slots depends on the order of arrival, so ALL of S (100 keys, the flattened pass) are matches: at
    least 96 of them are found in the surplus list.  If the arithmetic above were off by one the counts asserted would still be right."""
    ids = one_bucket_ids(SURPLUS_ROWS[1] + 40)
    assert ids.min() >= 4096 and ids.max() < (1 << 23)
    n_core = int(ids.max()) + 1
    owner = np.full(n_core, -1, dtype=np.int32)
    s, d, gadgets, tris = [], [], [], []
    for i, A in enumerate(SURPLUS_ROWS):
        u, v = 512 * i, 1024 + 512 * i
        owner[u] = owner[v] = i
        R = ids[i:i + A]
        S = R[np.arange(SURPLUS_L) * A // SURPLUS_L]
        s += [np.array([v]), np.full(len(S), v), np.full(A, u)]
        d += [np.array([u]), S, R]
        tris += [(v, u, int(h)) for h in S]
        gadgets.append(Gadget("surplus", f"surplus A={A} L={SURPLUS_L}", u, v, SURPLUS_L, A, S, R, np.arange(SURPLUS_L), SURPLUS_L))
    hubs = ids[: SURPLUS_ROWS[1] + 1]
    target = np.zeros(n_core, dtype=np.int64)
    D = 200
    target[hubs] = D
    return Probe("surplus", _assemble(n_core, s, d, target, id_space=1 << 24, leaf_base=1 << 23), n_core, hubs, gadgets, tris, [], owner, D)


def hosts_as_source(tail: int, d_target: int) -> bool:
    """the host rule of csrc/gm_tasks.hip task_walk_rows for the DAG edge s -> t, both rows within the stage: does s host (and stream N+(t))?"""
    return tail >= d_target
