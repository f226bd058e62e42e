"""Probe graphs for the triangle nuclei (csrc/gm_nucleus34.hip): symmetric graphs in which ONE streamed list of nuc_index_kernel, or ONE
row u of nuc_walk, has a chosen length with its matches at chosen positions, so that a wrong value names a length and a position (test
helper, numpy only; imported by tests/test_nucleus_probes_host.py and tests/test_gpu_nucleus34_probes.py).

The machinery is tests/probe_graphs.py's: gadget vertices joined to HUBS that private leaves pad to one common degree D above every
gadget vertex's degree (probe_graphs._assemble), so that under the orientation (lower symmetric degree -> higher, ties by id) every gadget
vertex points at its hubs.  Unlike there, hubs carry planted hub-hub edges; the padding is computed after they are planted, so every hub
still has exactly D entries and the orientation among hubs goes by id.

Families (every gadget's label is family/length/pattern/way, which a failure prints):
  index  One edge v - u, N+(v) = {u} + S, N+(u) = R.  The hub ids are SLOTS of kStride ids: slot j holds one hub of the pool S draws its
         non-matches from, one of the pool R draws its non-matches from, and between them the private hubs of the gadgets that match at
         position j, so S & R are exactly the chosen positions and no two gadgets share a matched hub.  The k matched hubs m_0 < ... of a
         gadget are joined as a half graph (m_i ~ m_j iff i + j >= k), and -- no graph has pairwise different degrees -- a vertex x BELOW
         v and u (three to a dozen entries) is joined to v, u and the m_i with 2 i >= k: K4(v, u, m_i) = i, different from slot to slot of
         the entry's segment.  Ways: "v" (v's list of sn keys is streamed: u first, then S; |R| = sn + 3), "tie" (|R| = sn: du == dv,
         still v's list) and "u" (R is streamed, sn keys, against v's sn + 2; leaves lift u above v, so the SOURCE has the longer list).
  walk   One triangle u -> v -> w whose row u (symmetric) has du entries: v, w, the common neighbours of the three at the pattern's
         positions, and elsewhere non-members adjacent to (u, v), to (u, w) or to u alone.  Row u's ids are one block in position order
         with u's own id in its middle.  A common neighbour is below u, between u and v, between v and w or above w, each by its degree
         (leaves pad it) or by an id tie at the degree of u, v or w.  Pattern "all": every free position a common neighbour above v, so
         that the segment of entry (u, v) has du - 1 triangles.
  trips  One graph whose units (entries of the oriented copy; triangles) mix whole-wave and group units inside trips of eight: a FAN
         (source a with 106 keys whose row runs W G G G G G G G G nine times -- the whole-wave entry moves one slot per trip --, then
         W G four times, then sixteen W) and a BOOK on a hub triangle whose pages alternate between three-entry pages (group triangles
         of count 1) and pages padded to 70 entries (whole-wave triangles of count 1), then six long pages and five short ones.

Structure(g) restates what the kernels walk for ANY graph: the orientation, the entries, every entry's segment, the triangles in
gm_tc_list's order.  lookup_census / trip_slots / the lane models are computed from it."""
from __future__ import annotations

import functools
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

import probe_graphs as PG

INDEX_GROUP_SN = (1, 7, 8, 9, 15, 16, 17, 63)
INDEX_WAVE_SN = (64, 65, 127, 128, 129, 200)
WALK_GROUP_DU = (3, 7, 8, 9, 16, 17, 63)
WALK_WAVE_DU = (64, 65, 127, 128, 129, 193)
WALK_ALL_DU = (64, 65, 66)  # pattern "all": segments of 63, 64, 65 triangles
WAYS = ("v", "tie", "u")
MAX_MATCHES = 24
kStride = 1024


def pattern_positions(n: int, pattern: str, tile: int) -> np.ndarray:
    """probe_graphs.positions with the `tiles` pattern evaluated modulo `tile` (the group's 8 keys or the wave's 64)"""
    if pattern != "tiles":
        return PG.positions(n, pattern) if n > 0 else np.zeros(0, np.int64)
    k = np.arange(n)
    return k[np.isin(k % tile, (0, 1, tile - 2, tile - 1))]


@dataclass
class Gadget:
    family: str
    label: str
    sn: int                 # index: keys of the streamed list; walk: entries of row u
    pattern: str
    way: str
    P: np.ndarray           # positions of the matches (common neighbours) inside the streamed list (row u)
    corners: tuple          # index: (v, u); walk: (u, v, w)
    matched: np.ndarray     # the matched hubs (common neighbours), ascending position
    extra: dict = field(default_factory=dict)


class NProbe:
    """graph, gadgets, want: {sorted triple: K4 by construction}, where: {sorted triple: label with the position}"""

    def __init__(self, name, graph, gadgets, want, where, n_core):
        self.name, self.graph, self.gadgets, self.want, self.where, self.n_core = name, graph, gadgets, want, where, n_core
        self.triangles = sorted(want)

    def label_of(self, triple) -> str:
        return self.where.get(tuple(int(x) for x in triple), "no gadget")


def _local_k4(vertices, edges):
    """{sorted triple: common neighbours} of the small graph on `vertices` (global ids) with `edges` (pairs of global ids): what a
    gadget's dense part holds by construction -- the gadgets share no triangle"""
    vs = sorted(set(int(x) for x in vertices))
    at = {x: i for i, x in enumerate(vs)}
    n = len(vs)
    M = np.zeros((n, n), dtype=bool)
    for a, b in edges:
        M[at[int(a)], at[int(b)]] = M[at[int(b)], at[int(a)]] = True
    out = {}
    for i in range(n):
        for j in np.flatnonzero(M[i, i + 1:]) + i + 1:
            both = M[i] & M[j]
            for k in np.flatnonzero(both[j + 1:]) + j + 1:
                out[(vs[i], vs[j], vs[k])] = int((both & M[k]).sum())
    return out


def _pairs(edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return [e[:, 0]], [e[:, 1]]


# ---- index ---------------------------------------------------------------------------------------------------------------------------
def index_specs():
    return [(sn, pat, way) for sn in INDEX_GROUP_SN + INDEX_WAVE_SN for pat in PG.PATTERNS for way in WAYS]


def _index_positions(sn, pat, way, tile):
    P = pattern_positions(sn, pat, tile)
    if way != "u":  # position 0 of v's list is u itself
        P = P[P > 0]
        if pat == "first" and sn > 1:
            P = np.array([1])
    if len(P) > MAX_MATCHES:
        P = np.concatenate([P[:MAX_MATCHES // 2], P[-(MAX_MATCHES // 2):]])
    return P.astype(np.int64)


@functools.lru_cache(maxsize=None)
def index(group: int = 8, whole: int = 64) -> NProbe:
    specs = index_specs()
    ng = len(specs)
    base = 3 * ng
    n_slots = max(INDEX_GROUP_SN + INDEX_WAVE_SN) + 8
    assert ng + 2 < kStride // 2
    pool_s = lambda j: base + np.asarray(j, np.int64) * kStride             # noqa: E731
    pool_r = lambda j: base + np.asarray(j, np.int64) * kStride + kStride // 2  # noqa: E731
    n_core = base + n_slots * kStride
    target = np.zeros(n_core, dtype=np.int64)
    D = max(INDEX_GROUP_SN + INDEX_WAVE_SN) + 56
    edges, gadgets, want, where, hubs = [], [], {}, {}, set()
    for i, (sn, pat, way) in enumerate(specs):
        x, v, u = 3 * i, 3 * i + 1, 3 * i + 2
        P = _index_positions(sn, pat, way, group if sn < whole else whole)
        k = len(P)
        if way == "u":  # R is the streamed list: slot j <-> position j
            A, L = sn, sn + 2
            m = base + P * kStride + 1 + i
            Rn = pool_r(np.setdiff1d(np.arange(A), P))
            Sn = pool_s(np.arange(L - k))
        else:           # {u} + S is the streamed list: slot j <-> position j + 1
            L, A = sn - 1, sn + 3 if way == "v" else sn
            m = base + (P - 1) * kStride + 1 + i
            Sn = pool_s(np.setdiff1d(np.arange(L), P - 1))
            Rn = pool_r(np.arange(A - k))
        S, R = np.sort(np.concatenate([Sn, m])), np.sort(np.concatenate([Rn, m]))
        assert len(S) == L and len(R) == A and np.array_equal(np.intersect1d(S, R), m)
        streamed = R if way == "u" else np.concatenate([[u], S])
        assert len(streamed) == sn and np.array_equal(np.flatnonzero(np.isin(streamed, m)), P)
        dense = [(v, u)] + [(v, h) for h in m] + [(u, h) for h in m]
        dense += [(m[a], m[b]) for a in range(k) for b in range(a + 1, k) if a + b >= k]
        if k >= 2:
            dense += [(x, v), (x, u)] + [(x, m[a]) for a in range(k) if 2 * a >= k]
        edges += dense + [(v, h) for h in Sn] + [(u, h) for h in Rn]
        label = f"index/sn={sn}/{pat}/{way}"
        local = _local_k4([x, v, u] + list(m), dense)
        for t, c in local.items():
            want[t] = c
            where[t] = f"{label}: a side triangle of the half graph"
        for a in range(k):
            t = tuple(sorted((v, u, int(m[a]))))
            assert want[t] == a or k < 2
            where[t] = f"{label}: slot {a} of the entry's segment, position {int(P[a])} of the streamed list"
        if way == "u":  # leaves lift u above v: the source keeps the longer list
            target[u] = (1 + L + (k >= 2)) + 1
        hubs.update(int(h) for h in np.concatenate([S, R]))
        gadgets.append(Gadget("index", label, sn, pat, way, P, (v, u), m, {"L": L, "A": A}))
    hubs = np.array(sorted(hubs), dtype=np.int64)
    target[hubs] = D
    s, d = _pairs(edges)
    return NProbe("index", PG._assemble(n_core, s, d, target), gadgets, want, where, n_core)


# ---- walk ----------------------------------------------------------------------------------------------------------------------------
CLASSES = ("below/degree", "below/tie", "uv/degree", "uv/tie", "vw/degree", "vw/tie", "above/degree", "above/tie")


def walk_specs():
    return [(du, pat) for du in WALK_GROUP_DU + WALK_WAVE_DU for pat in PG.PATTERNS] + [(du, "all") for du in WALK_ALL_DU]


def _class_degree(cls, du, idx, iu, iv, iw):
    """the symmetric degree that puts a common neighbour of id idx into the class, or None if its id does not allow it (0: as it is,
    three entries)"""
    dv, dw = du + 4, du + 8
    if cls == "below/degree":
        return 0 if du > 3 else None
    if cls == "below/tie":
        return du if idx < iu else None
    if cls == "uv/degree":
        return du + 2
    if cls == "uv/tie":
        return du if idx > iu else (dv if idx < iv else None)
    if cls == "vw/degree":
        return du + 6
    if cls == "vw/tie":
        return dv if idx > iv else (dw if idx < iw else None)
    if cls == "above/degree":
        return du + 12
    return dw if idx > iw else None


@functools.lru_cache(maxsize=None)
def walk(group: int = 8, whole: int = 64) -> NProbe:
    specs = walk_specs()
    n_core = sum(du + 1 for du, _ in specs)
    target = np.zeros(n_core, dtype=np.int64)
    edges, gadgets, want, where = [], [], {}, {}
    b, turn, kind_turn = 0, 0, 0
    for du, pat in specs:
        upos = du // 2
        ids = np.array([b + p + (p >= upos) for p in range(du)], dtype=np.int64)  # row u by position; u's own id in the middle
        u = b + upos
        if pat == "all":
            free = [du // 3, (2 * du) // 3]
            P = np.setdiff1d(np.arange(du), free)
        else:
            P = pattern_positions(du, pat, group if du < whole else whole)
            P = P[:max(0, du - 2)] if pat != "last" else P
            free = [p for p in list(range(du // 3, du)) + list(range(du // 3)) if p not in set(P.tolist())][:2]
            free.sort()
        v, w = int(ids[free[0]]), int(ids[free[1]])
        label = f"walk/du={du}/{pat}"
        dense = [(u, v), (u, w), (v, w)]
        classes = []
        for p in P:
            xid = int(ids[p])
            for _ in range(len(CLASSES)):
                cls = CLASSES[turn % len(CLASSES)]
                turn += 1
                if pat == "all" and not cls.startswith(("vw", "above")):
                    continue
                deg = _class_degree(cls, du, xid, u, v, w)
                if deg is not None:
                    break
            else:
                raise AssertionError(label)
            target[xid] = deg
            classes.append(cls)
            dense += [(u, xid), (v, xid), (w, xid)]
        others = []
        for p in range(du):
            if p in free or p in set(P.tolist()):
                continue
            kind = ("uv", "uw", "u")[kind_turn % 3]
            kind_turn += 1
            others.append((u, int(ids[p])))
            if kind != "u":
                others.append((v if kind == "uv" else w, int(ids[p])))
        edges += dense + others
        target[v], target[w] = du + 4, du + 8
        local = _local_k4([u, v, w] + [int(ids[p]) for p in P], dense)
        for t, c in local.items():
            want[t] = c
            where[t] = f"{label}: a triangle on a common neighbour"
        for e in others:  # a non-member adjacent to u and to v (or w) closes a triangle without a clique
            if e[0] != u:
                t = tuple(sorted((u, e[0], e[1])))
                want[t] = 0
                where[t] = f"{label}: a triangle on a non-member"
        t = tuple(sorted((u, v, w)))
        assert want[t] == len(P)
        where[t] = f"{label}: the triangle itself, common neighbours at positions {P.tolist()[:8]}{' ...' if len(P) > 8 else ''} of row u"
        gadgets.append(Gadget("walk", label, du, pat, "", P.astype(np.int64), (u, v, w), ids[P], {"classes": classes}))
        b += du + 1
    s, d = _pairs(edges)
    return NProbe("walk", PG._assemble(n_core, s, d, target), gadgets, want, where, n_core)


# ---- trips ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trips(group: int = 8, whole: int = 64) -> NProbe:
    per = whole // group
    roles = ("W" + "G" * per) * (per + 1) + "WG" * (per // 2) + "W" * (2 * per)
    list_len = whole + 6                                         # keys of a whole-wave target's list: two tiles
    a = 0
    tgt = np.arange(1, 1 + len(roles), dtype=np.int64)
    h0 = 1 + len(roles)
    pool = np.arange(h0 + 1, h0 + 1 + list_len - 1, dtype=np.int64)  # the other keys of the whole-wave targets' lists
    A, B, C = (int(pool[-1]) + 1 + i for i in range(3))
    pages = "LS" * (3 * per) + "L" * 6 + "S" * 5                # L: padded to whole + 6 entries (whole-wave), S: three entries
    page = np.arange(C + 1, C + 1 + len(pages), dtype=np.int64)
    n_core = int(page[-1]) + 1
    target = np.zeros(n_core, dtype=np.int64)
    edges = [(a, int(t)) for t in tgt] + [(a, h0)] + [(int(t), h0) for t in tgt]
    for t, r in zip(tgt, roles):
        if r == "W":
            edges += [(int(t), int(h)) for h in pool]
    deg_a = len(roles) + 1
    target[tgt] = deg_a + 1                                      # a -> every target
    D = deg_a + 40
    target[h0] = target[pool] = D
    edges += [(A, B), (A, C), (B, C)]
    for q, r in zip(page, pages):
        edges += [(int(q), A), (int(q), B), (int(q), C)]
        if r == "L":
            target[q] = whole + 6
    target[[A, B, C]] = D
    want, where = {}, {}
    for t, r in zip(tgt, roles):
        want[tuple(sorted((a, int(t), h0)))] = 0
        where[tuple(sorted((a, int(t), h0)))] = f"trips/fan: target {int(t) - 1} ({'whole wave' if r == 'W' else 'group'})"
    for q, r in zip(page, pages):
        for pr in ((A, B), (A, C), (B, C)):
            want[tuple(sorted((int(q),) + pr))] = 1
            where[tuple(sorted((int(q),) + pr))] = f"trips/book: page {int(q - page[0])} ({'whole wave' if r == 'L' else 'group'})"
    want[(A, B, C)] = len(pages)
    where[(A, B, C)] = "trips/book: the hub triangle"
    s, d = _pairs(edges)
    g = Gadget("trips", "trips", whole, "", "", np.zeros(0, np.int64), (a, A, B, C), tgt, {"roles": roles, "pages": pages})
    return NProbe("trips", PG._assemble(n_core, s, d, target), [g], want, where, n_core)


# ---- dense cells -----------------------------------------------------------------------------------------------------------------------
DENSE_BIG, DENSE_SMALL, DENSE_SEED = 130, 56, 20261021


@functools.lru_cache(maxsize=None)
def dense_cell(n: int, seed: int = DENSE_SEED):
    """(graph, A): K_n minus a seeded set of edges, A its dense adjacency matrix in float64.  The edge {i, j} is taken out with
    probability (i + j) / (8 n): a handful of entries per row at the low ids, a quarter of the row at the high ones, so the degrees
    -- and with them the orientation, the lengths of the oriented rows and K4(t) -- are graded, not all alike"""
    from graphminer_amd.rmat import csr_from_pairs

    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) >= (iu + ju) / (8.0 * n)
    A = np.zeros((n, n), dtype=np.float64)
    A[iu[keep], ju[keep]] = A[ju[keep], iu[keep]] = 1.0
    return csr_from_pairs(n, iu[keep].astype(np.uint64), ju[keep].astype(np.uint64)), A


def dense_k4(A):
    """{sorted triple: K4} from float64 products of the dense adjacency matrix: for a fixed corner a, ((A * A[a]) @ A)[b, c] = the
    common neighbours of a, b and c.  Every value is an integer below n: exact"""
    n = A.shape[0]
    out = {}
    for a in range(n):
        K = (A * A[a]) @ A
        bs, cs = np.nonzero(np.triu(A * np.outer(A[a], A[a]), 1))
        ok = bs > a
        for b, c, k in zip(bs[ok].tolist(), cs[ok].tolist(), K[bs[ok], cs[ok]].tolist()):
            out[(a, b, c)] = int(k)
    return out


# ---- what the kernels walk, for any graph ------------------------------------------------------------------------------------------------
class Structure:
    """deg; the oriented copy (drp, dcol: lower (degree, id) -> higher, rows ascending); per entry e: src[e], dcol[e], sn[e] (the keys
    nuc_index_kernel streams), seg[e] (N+(src) & N+(dst), ascending); tri_off; the triangles (u, v, w) in gm_tc_list's order with their
    entry tri_e; k4(): the common neighbours of every triangle"""

    def __init__(self, g):
        rp, col = np.asarray(g.row_ptr, np.int64), np.asarray(g.col_idx, np.int64)
        nv = len(rp) - 1
        self.rp, self.col, self.nv = rp, col, nv
        self.deg = deg = np.diff(rp)
        src = np.repeat(np.arange(nv, dtype=np.int64), deg)
        keep = (deg[src] < deg[col]) | ((deg[src] == deg[col]) & (src < col))
        self.src, self.dcol = src[keep], col[keep]
        self.drp = np.zeros(nv + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.src, minlength=nv), out=self.drp[1:])
        dplus = np.diff(self.drp)
        self.dplus = dplus
        self.sn = np.minimum(dplus[self.src], dplus[self.dcol])
        self.u_short = dplus[self.src] <= dplus[self.dcol]
        out = {}
        for x in np.flatnonzero(dplus > 0).tolist():
            out[x] = set(self.dcol[self.drp[x]:self.drp[x + 1]].tolist())
        self.out = out
        self.seg = {}
        counts = np.zeros(len(self.src), dtype=np.int64)
        for e in np.flatnonzero(self.sn > 0).tolist():
            both = out[int(self.src[e])] & out[int(self.dcol[e])]
            if both:
                self.seg[e] = sorted(both)
                counts[e] = len(both)
        self.tri_off = np.zeros(len(self.src) + 1, dtype=np.int64)
        np.cumsum(counts, out=self.tri_off[1:])
        self.tri_e = np.repeat(np.arange(len(self.src), dtype=np.int64), counts)
        self.tri_w = np.array([w for e in sorted(self.seg) for w in self.seg[e]], dtype=np.int64)
        self.tris = np.stack([self.src[self.tri_e], self.dcol[self.tri_e], self.tri_w], axis=1) if len(self.tri_w) else np.zeros((0, 3), np.int64)

    def row(self, x):
        return self.col[self.rp[x]:self.rp[x + 1]]

    def orow(self, x):
        return self.dcol[self.drp[x]:self.drp[x + 1]]

    def members(self, t):
        """bool per entry of row u of triangle t: a common neighbour of its corners"""
        u, v, w = (int(x) for x in self.tris[t])
        r = self.row(u)
        return np.isin(r, self.row(v)) & np.isin(r, self.row(w))

    @functools.cached_property
    def k4(self):
        return np.array([int(self.members(t).sum()) for t in range(len(self.tris))], dtype=np.int64)

    def below(self, a, b):
        return (self.deg[a], a) < (self.deg[b], b)


def trip_slots(st: Structure, unit: str, group: int = 8, whole: int = 64):
    """per trip of whole // group consecutive units: (the slots that are whole-wave units, the slots that are group units with a
    non-zero value).  unit "entry": the entries, whole-wave from sn >= whole, value |segment|; "triangle": whole-wave from a row u of
    `whole` entries, value K4"""
    per = whole // group
    if unit == "entry":
        big, val = st.sn >= whole, np.diff(st.tri_off)
    else:
        big, val = st.deg[st.tris[:, 0]] >= whole, st.k4
    out = []
    for t0 in range(0, len(big), per):
        out.append((frozenset(np.flatnonzero(big[t0:t0 + per]).tolist()), frozenset(np.flatnonzero(~big[t0:t0 + per] & (val[t0:t0 + per] > 0)).tolist())))
    return out


def lookup_census(st: Structure):
    """the look-ups of the peel, for every triangle t = (u, v, w) and every common neighbour x of its corners -- the decomposition walks
    each exactly once.  Returns (cases, rows, segments): cases counts (sibling 0 .. 2, branch 0 .. 2, decided with a degree tie?) of
    nuc_id_with; rows the (length, position of the key) of every bisected row of the oriented copy; segments the same of every bisected
    tri_w segment"""
    cases, rows, segments = Counter(), Counter(), Counter()
    entry_at = {}
    for t in range(len(st.tris)):
        u, v, w = (int(x) for x in st.tris[t])
        r = st.row(u)
        for x in r[st.members(t)].tolist():
            for sib, (a, b) in enumerate(((u, v), (u, w), (v, w))):
                tie = st.deg[x] == st.deg[a]
                if st.below(x, a):
                    branch, (p, q, c) = 0, (x, a, b)
                else:
                    tie = tie or st.deg[x] == st.deg[b]
                    branch, (p, q, c) = (1, (a, x, b)) if st.below(x, b) else (2, (a, b, x))
                cases[(sib, branch, bool(tie))] += 1
                orow = st.orow(p)
                pos = int(np.searchsorted(orow, q))
                assert orow[pos] == q
                rows[(len(orow), pos)] += 1
                seg = st.seg[int(st.drp[p]) + pos]
                segments[(len(seg), seg.index(c))] += 1
    return cases, rows, segments


# ---- lane models (the sensitivity check of the host test) ----------------------------------------------------------------------------------
MUTANTS = ("last key of a trip dropped", "> instead of >= at the whole-wave boundary", "rank not carried from tile to tile",
           "group byte shifted by one group", "u_short inverted on a tie", "whole-wave count not written back to the group's lane")


def model_index(st: Structure, mutant=None, group: int = 8, whole: int = 64, n_entries=None):
    """DESIGN.md "The triangle index" lane by lane: eight entries to a trip, the shorter list streamed by the entry's group of `group`
    lanes in trips of `group` keys, the rank of a match from the group's byte of the ballot; a list of `whole` keys or more strided by
    the whole wave, the rank carried from tile to tile, the count written back to the group's first lane.  COUNT, the scan, FILL.
    Returns (cnt per entry, tri_w by slot with -1 where nothing was written)."""
    per = whole // group
    ne = len(st.src) if n_entries is None else n_entries

    def run(off):
        cnt, written = np.zeros(ne, dtype=np.int64), {}
        for e0 in range(0, ne, per):
            es = list(range(e0, min(e0 + per, ne)))
            lists = []
            for e in es:
                a, b = int(st.src[e]), int(st.dcol[e])
                da, db = int(st.dplus[a]), int(st.dplus[b])
                short_a = da <= db
                stream = st.orow(a if short_a else b)
                if mutant == MUTANTS[4] and da == db:
                    looked = set(stream.tolist())           # the base of the looked-up list chosen with < where the streamed one used <=
                else:
                    looked = st.out.get(b if short_a else a, set())
                lists.append((stream, looked, len(stream) >= whole))
            n = [0] * len(es)
            is_whole = [(len(s) > whole) if mutant == MUTANTS[1] else w for s, _, w in lists]
            mine = [0 if w else len(s) for s, _, w in lists]
            for k0 in range(0, max(mine, default=0), group):
                ballot = 0
                for gi in range(len(es)):
                    for gl in range(group):
                        k = k0 + gl
                        if k < mine[gi] and not (mutant == MUTANTS[0] and gl == group - 1) and int(lists[gi][0][k]) in lists[gi][1]:
                            ballot |= 1 << (gi * group + gl)
                for gi in range(len(es)):
                    shift = ((gi + 1) % per if mutant == MUTANTS[3] else gi) * group
                    m = (ballot >> shift) & ((1 << group) - 1)
                    for gl in range(group):
                        if ballot >> (gi * group + gl) & 1 and off is not None:
                            written[int(off[es[gi]]) + n[gi] + bin(m & ((1 << gl) - 1)).count("1")] = int(lists[gi][0][k0 + gl])
                    n[gi] += bin(m).count("1")
            for gi in range(len(es)):
                if not is_whole[gi]:
                    continue
                stream, looked, _ = lists[gi]
                nn = 0
                for t0 in range(0, len(stream), whole):
                    found = [t0 + lane < len(stream) and not (mutant == MUTANTS[0] and lane == whole - 1) and int(stream[t0 + lane]) in looked
                             for lane in range(whole)]
                    for lane in range(whole):
                        if found[lane] and off is not None:
                            written[int(off[es[gi]]) + (0 if mutant == MUTANTS[2] else nn) + sum(found[:lane])] = int(stream[t0 + lane])
                    nn += sum(found)
                if mutant != MUTANTS[5]:
                    n[gi] = nn
            cnt[es] = n
        return cnt, written

    cnt, _ = run(None)
    off = np.concatenate([[0], np.cumsum(cnt)])
    _, written = run(off)
    total = int(off[-1])
    return cnt, np.array([written.get(i, -1) for i in range(total)], dtype=np.int64)


def model_walk(st: Structure, mutant=None, group: int = 8, whole: int = 64):
    """DESIGN.md "One gather for the count and the peel" lane by lane: row u streamed, a group of `group` lanes striding a row below
    `whole` entries, the whole wave a longer one, its count written to the group's first lane.  Returns K4 per triangle."""
    out = np.zeros(len(st.tris), dtype=np.int64)
    for t in range(len(st.tris)):
        memb = st.members(t)
        du = len(memb)
        k = np.arange(du)
        if du < whole:
            keep = (k % group != group - 1) if mutant == MUTANTS[0] else np.ones(du, bool)
            out[t] = int((memb & keep).sum())
        elif (du > whole if mutant == MUTANTS[1] else True) and mutant != MUTANTS[5]:
            keep = (k % whole != whole - 1) if mutant == MUTANTS[0] else np.ones(du, bool)
            out[t] = int((memb & keep).sum())
    return out
