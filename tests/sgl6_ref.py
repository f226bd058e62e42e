"""References for the two 6-vertex patterns of the reference's sgl solver, 6path and dumbbell (test helper):
  * loops(g, pattern): the loop nests of src/sgl/cpu_kernels/{6path,dumbbell}.h restated line by line in plain Python, with the two set
    helpers the dumbbell uses (intersection_set(a, b, up) and intersect_ns_bound_except(.., up, nodes), include/VertexSet.h:206-222) --
    small graphs only;
  * raw_sums(g, need): the nine raw sums of gm_sgl6_raw (X, Y, Z, R, D, C5, M, B, K4) from numpy / Python integers; R and Z from the
    UNPRUNED definition (every ordered pair of opposite corners), C5 and K4 from the CPU oracle; `need` limits the work;
  * finish(pattern, raw): the closed forms, modulo 2^64;
  * complete_counts(n), kab_raw(a, b): analytic values for K_n and K_{a,b}.
Notation: d(v) the degree, t(e) = |N(u) ^ N(v)| the support of e = {u, v}, x = t - 1, T_v the triangles at v, e1(v) = sum_{a in N(v)} (d(a) - 1).
"""
from __future__ import annotations

from math import comb

import numpy as np

PATTERNS = ("6path", "dumbbell")
RAW = ("X", "Y", "Z", "R", "D", "C5", "M", "B", "K4")
NEEDS = {"6path": ("X", "Y", "Z", "R", "D", "C5"), "dumbbell": ("M", "B", "K4")}
M64 = 2**64


def mask(names) -> int:
    return sum(1 << RAW.index(k) for k in names)


def adjacency(g):
    rp, ci = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    return [ci[rp[v]:rp[v + 1]].tolist() for v in range(len(rp) - 1)]


def intersection_set(a, b, up=None):
    """the members of the ascending lists a and b, below `up` when given (a merge, as VertexSet does it)"""
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        left, right = a[i], b[j]
        if up is not None and (left >= up or right >= up):
            break
        if left <= right:
            i += 1
        if right <= left:
            j += 1
        if left == right:
            out.append(left)
    return out


def intersect_ns_bound_except(a, b, up, nodes) -> int:
    """|{w in a ^ b : w < up, w not in nodes}|"""
    n, i, j = 0, 0, 0
    while i < len(a) and j < len(b):
        left, right = a[i], b[j]
        if left >= up or right >= up:
            break
        if left <= right:
            i += 1
        if right <= left:
            j += 1
        if left == right and left not in nodes:
            n += 1
    return n


def loops(g, pattern: str) -> int:
    N = adjacency(g)
    nv, counter = len(N), 0
    if pattern == "6path":
        for v0 in range(nv):
            for v1 in N[v0]:
                if v1 >= v0:
                    break
                for v2 in N[v0]:
                    if v2 == v1:
                        continue
                    for v3 in N[v1]:
                        if v3 == v0 or v3 == v2:
                            continue
                        for v4 in N[v2]:
                            if v4 == v0 or v4 == v1 or v4 == v3:
                                continue
                            for v5 in N[v3]:
                                if v5 == v0 or v5 == v1 or v5 == v2 or v5 == v4:
                                    continue
                                counter += 1
    elif pattern == "dumbbell":
        for v0 in range(nv):
            adj0 = N[v0]
            for v1 in adj0:
                for v2 in intersection_set(adj0, N[v1], v1):
                    for v3 in adj0:
                        if v3 >= v0:
                            break
                        if v3 == v1 or v3 == v2:
                            continue
                        adj3 = N[v3]
                        for v4 in adj3:
                            if v4 == v0 or v4 == v1 or v4 == v2:
                                continue
                            counter += intersect_ns_bound_except(adj3, N[v4], v4, (v0, v1, v2))
    else:
        raise ValueError(pattern)
    return counter


def _c2(x: int) -> int:
    return x * (x - 1) // 2


DENSE_MAX = 8192  # vertices up to which the common-neighbour counts are taken from the dense product A A


def _dense_common(g):
    """|N(v) ^ N(x)| for every pair as a dense float32 matrix (entries at most nv < 2^24: exact)"""
    rp, ci = np.asarray(g.row_ptr).astype(np.int64), np.asarray(g.col_idx).astype(np.int64)
    nv = len(rp) - 1
    a = np.zeros((nv, nv), np.float32)
    a[np.repeat(np.arange(nv, dtype=np.int64), np.diff(rp)), ci] = 1.0
    return a @ a


def _common_counts(g, dense=None):
    """every ordered pair (v, x), v != x, with c = |N(v) ^ N(x)| >= 2: (v, x, c) as int64 arrays -- dense A A for a small graph, else the
    wedges v - p - x grouped by their ends"""
    rp, ci = np.asarray(g.row_ptr).astype(np.int64), np.asarray(g.col_idx).astype(np.int64)
    nv = len(rp) - 1
    deg = np.diff(rp)
    src = np.repeat(np.arange(nv, dtype=np.int64), deg)
    if dense is not None:
        c = dense.copy()
        np.fill_diagonal(c, 0.0)
        v, x = np.nonzero(c >= 2.0)
        return v.astype(np.int64), x.astype(np.int64), c[v, x].astype(np.int64)
    cnt = deg[src]  # entry (p, v): one wedge v - p - x per x in N(p)
    off = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    v = np.repeat(ci, cnt)
    x = ci[np.repeat(rp[src], cnt) + off]
    keep = v != x
    keys, c = np.unique(v[keep] * nv + x[keep], return_counts=True)
    big = c >= 2
    return keys[big] // nv, keys[big] % nv, c[big].astype(np.int64)


def raw_sums(g, need=RAW) -> dict:
    """the raw sums named in `need` as exact Python integers modulo 2^64 (the others 0)"""
    import sgl5_ref as R5

    rp, ci = np.asarray(g.row_ptr).astype(np.int64), np.asarray(g.col_idx).astype(np.int64)
    nv = len(rp) - 1
    deg = np.diff(rp)
    src = np.repeat(np.arange(nv, dtype=np.int64), deg)
    need = set(need)
    out = dict.fromkeys(RAW, 0)
    dense = _dense_common(g) if nv <= DENSE_MAX and need & {"X", "Y", "M", "Z", "R"} else None
    if need & {"X", "Y", "M"}:
        keys = src * nv + ci
        und = src < ci
        eu, ev = src[und], ci[und]
        if dense is not None:
            t = dense[eu, ev].astype(np.int64).tolist()
        else:  # t(e): the keys of the shorter list looked up in the longer one
            short_is_u = deg[eu] <= deg[ev]
            s_end, l_end = np.where(short_is_u, eu, ev), np.where(short_is_u, ev, eu)
            cnt = deg[s_end]
            eid = np.repeat(np.arange(len(eu), dtype=np.int64), cnt)
            off = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            w = ci[np.repeat(rp[s_end], cnt) + off]
            q = np.repeat(l_end, cnt) * nv + w
            pos = np.minimum(np.searchsorted(keys, q), max(len(keys) - 1, 0))
            hit = keys[pos] == q if len(keys) else np.zeros(0, bool)
            t = np.bincount(eid[hit], minlength=len(eu)).tolist()
        dl, eul, evl = deg.tolist(), eu.tolist(), ev.tolist()
        tv2 = [0] * nv
        e1 = [0] * nv
        for a, b, x in zip(eul, evl, t):
            tv2[a] += x
            tv2[b] += x
            e1[a] += dl[b] - 1
            e1[b] += dl[a] - 1
        tv = [x // 2 for x in tv2]
        out["X"] = sum((e1[a] - (dl[b] - 1) - x) * (e1[b] - (dl[a] - 1) - x) for a, b, x in zip(eul, evl, t))
        out["Y"] = sum(x * (d - 2) ** 2 for x, d in zip(tv, dl))
        out["M"] = sum((tv[a] - x) * (tv[b] - x) for a, b, x in zip(eul, evl, t))
    if need & {"Z", "R"}:
        v, x, c = _common_counts(g, dense)
        c2 = [_c2(k) for k in c.tolist()]
        r4 = sum(c2)  # every 4-cycle at each of its four corners
        assert r4 % 4 == 0
        out["R"] = r4 // 4
        out["Z"] = sum(k * d for k, d in zip(c2, deg[v].tolist()))
    five = tuple(k for k in ("D", "B", "K4") if k in need)
    if five:
        r5 = R5.raw_sums(g, need=five)
        for k in five:
            out[k] = r5[k]
    if "C5" in need:
        import oracle as O

        out["C5"] = O.pentagon(O.OGraph(g.row_ptr, g.col_idx))
    return {k: (v % M64 if k in need else 0) for k, v in out.items()}


def finish(pattern: str, raw) -> int:
    r = raw if isinstance(raw, dict) else dict(zip(RAW, raw))
    v = {"6path": r["X"] - r["Y"] - 2 * r["Z"] + 12 * r["R"] + 4 * r["D"] - 5 * r["C5"],
         "dumbbell": r["M"] - r["B"] + 6 * r["K4"]}[pattern]
    return v % M64


def complete_counts(n: int) -> dict:
    """K_n: an ordered choice of six vertices is a 6-path twice; two disjoint triangles and one of the nine edges between them"""
    p = 1
    for i in range(6):
        p *= max(n - i, 0)
    return {"6path": p // 2, "dumbbell": comb(n, 2) * comb(n - 2, 2) * comb(n - 4, 2)}


def kab_raw(a: int, b: int) -> dict:
    """K_{a,b}: R = C(a,2) C(b,2), every 4-cycle has degree sum 2 (a + b), no odd cycle"""
    r = comb(a, 2) * comb(b, 2)
    return {"R": r, "Z": 2 * (a + b) * r % M64, "C5": 0}
