"""Plain Python reference of the triangle nuclei (gm_tri_clique4_local / gm_nucleus34 / gm_nucleus34_decompose): the triangles and 4-cliques
of a graph, K4(t), the whole-frontier rounds with the rule of the decrements of include/graphminer_amd.h, the fixed-c form, and a
one-triangle-at-a-time peel that recounts from scratch.  Every result is keyed by the sorted triple (a, b, c); `ordered` lines a result up
with the rows of tc_list, which is how the GPU tests pin "id = gm_tc_list position"."""
from collections import namedtuple
from itertools import combinations

import numpy as np

REMOVED = 0xFFFFFFFF
ALIVE, FRONTIER, GONE = 0, 1, 2

Decomposition = namedtuple("Decomposition", "theta round c_max rounds destroyed")  # theta, round: {triple: value}
Nucleus = namedtuple("Nucleus", "cnt triangles cliques rounds destroyed")           # cnt: {triple: count inside the set or REMOVED}


def adjacency(g):
    rp, col = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    return [set(int(x) for x in col[rp[v]:rp[v + 1]] if int(x) != v) for v in range(g.V())]


def triangles(g, adj=None):
    """the sorted triples a < b < c"""
    adj = adj or adjacency(g)
    out = []
    for a in range(len(adj)):
        above = sorted(x for x in adj[a] if x > a)
        for b in above:
            out.extend((a, b, c) for c in sorted(adj[a] & adj[b]) if c > b)
    return out


def cliques4(g, adj=None):
    """the sorted quadruples a < b < c < d"""
    adj = adj or adjacency(g)
    return [(a, b, c, d) for a, b, c in triangles(g, adj) for d in sorted(adj[a] & adj[b] & adj[c]) if d > c]


def k4(g):
    """{triple: the 4-cliques that contain it} = the common neighbours of its corners"""
    adj = adjacency(g)
    return {t: len(adj[t[0]] & adj[t[1]] & adj[t[2]]) for t in triangles(g, adj)}


class _State:
    """the triangles (ids in sorted order), the 4-cliques as four triangle ids each, the cliques on every triangle, and the counts"""

    def __init__(self, g):
        if isinstance(g, _State):  # (a prepared graph: the enumeration is shared, the counts and the marks are this run's own)
            self.tris, self.cliques, self.on = g.tris, g.cliques, g.on
        else:
            adj = adjacency(g)
            self.tris = triangles(g, adj)
            ids = {t: i for i, t in enumerate(self.tris)}
            self.cliques = [tuple(ids[t] for t in combinations(q, 3)) for q in cliques4(g, adj)]
            self.on = [[] for _ in self.tris]
            for q, four in enumerate(self.cliques):
                for t in four:
                    self.on[t].append(q)
        self.cnt = np.array([len(x) for x in self.on], dtype=np.int64)
        self.mark = np.zeros(len(self.tris), dtype=np.int8)
        self.destroyed = 0

    def round(self, thr, census=None):
        """steps 1 - 3 of a round: last round's frontier becomes removed, the alive triangles below thr become the frontier, the peel.
        Returns the frontier.  The rule: a 4-clique counts only if none of its triangles was removed before the round began; with at
        least one frontier triangle it is destroyed, accounted once by its frontier triangle of the smallest id, and every triangle of it
        outside the frontier loses one.  With a Counter `census` the round also records what the blocked rule met (round_census)."""
        self.mark[self.mark == FRONTIER] = GONE
        front = np.flatnonzero((self.mark == ALIVE) & (self.cnt < thr))
        self.mark[front] = FRONTIER
        mark, cnt = self.mark, self.cnt
        for t in front.tolist():
            for q in self.on[t]:
                four = self.cliques[q]
                if census is not None:
                    # the siblings of t in this clique are numbered as the peel kernel looks them up, with the ids in place of the
                    # orientation: `four` lists the triangles of the sorted quadruple by the corner left out, the largest first, so
                    # of the other three the first keeps t's two smallest corners (sibling 0), the second its smallest and its largest
                    # (sibling 1), the third its two largest (sibling 2)
                    blocked = False
                    for sib, s in enumerate(s for s in four if s != t):
                        if mark[s] == GONE:
                            census[("skipped: a sibling removed earlier", sib)] += 1
                            blocked = True
                        elif mark[s] == FRONTIER and s < t:
                            census[("skipped: a sibling in the frontier at a smaller id", sib)] += 1
                            blocked = True
                    if not blocked:
                        census[("destroyed: frontier triangles", sum(1 for s in four if mark[s] == FRONTIER))] += 1
                if any(mark[s] == GONE or (mark[s] == FRONTIER and s < t) for s in four if s != t):
                    continue  # (blocked: it was destroyed in an earlier round, or a frontier triangle of a smaller id accounts it)
                self.destroyed += 1
                for s in four:
                    if mark[s] == ALIVE:
                        cnt[s] -= 1
        return front

    def alive(self):
        return self.mark == ALIVE


def prepare(g):
    """the enumeration of a graph, for several runs of decompose / nucleus on it: they take it in place of the graph"""
    return _State(g)


def decompose(g, census=None):
    s = _State(g)
    n = len(s.tris)
    theta, rnd = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    rounds, c_max = 0, 0
    level = int(s.cnt.min()) if n else 0
    while True:
        front = s.round(level + 1, census)
        rounds += 1
        if front.size == 0:
            alive = s.alive()
            if not alive.any():
                break
            level = int(s.cnt[alive].min())
            continue
        theta[front], rnd[front], c_max = level, rounds, level
    assert (s.cnt >= 0).all()
    return Decomposition({t: int(theta[i]) for i, t in enumerate(s.tris)}, {t: int(rnd[i]) for i, t in enumerate(s.tris)}, c_max, rounds, s.destroyed)


def round_census(g):
    """what the blocked rule meets over the rounds of decompose(g), a Counter: ("destroyed: frontier triangles", 1 .. 4) per destroyed
    clique, and per frontier triangle that skips a clique ("skipped: a sibling removed earlier", sibling) or ("skipped: a sibling in the
    frontier at a smaller id", sibling), once for every sibling 0 .. 2 that blocks it (numbered as in _State.round)"""
    from collections import Counter

    census = Counter()
    decompose(g, census)
    return census


def nucleus(g, c):
    s = _State(g)
    rounds = 0
    while True:
        front = s.round(c)
        rounds += 1
        if front.size == 0:
            break
    alive = s.alive()
    assert (s.cnt >= 0).all()
    cnt = {t: int(s.cnt[i]) if alive[i] else REMOVED for i, t in enumerate(s.tris)}
    return Nucleus(cnt, int(alive.sum()), len(s.cliques) - s.destroyed, rounds, s.destroyed)


def peel_one_at_a_time(g):
    """{triple: theta} by the textbook peel: recount K4_t(H) of every triangle of H from scratch, remove ONE triangle of the smallest count,
    theta = the largest smallest count seen so far"""
    s = _State(g)
    inside = [True] * len(s.tris)
    theta, level = {}, 0
    for _ in s.tris:
        counts = {t: sum(1 for q in s.on[t] if all(inside[x] for x in s.cliques[q])) for t in range(len(s.tris)) if inside[t]}
        t = min(counts, key=lambda x: (counts[x], x))
        level = max(level, counts[t])
        theta[s.tris[t]] = level
        inside[t] = False
    return theta


def ordered(rows, values, dtype=np.uint32):
    """the values {triple: v} in the order of tc_list's rows (a < b < c per row)"""
    return np.array([values[(int(a), int(b), int(c))] for a, b, c in np.asarray(rows)], dtype=dtype)
