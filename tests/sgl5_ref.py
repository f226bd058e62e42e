"""References for the six 5-vertex patterns of the reference's sgl solver beyond house / pentagon (test helper):
  * loops(g, pattern): the loop nests of src/sgl/cpu_kernels/{hourglass,taileddiamond,taileddiamond2,semihouse,closedhouse,5path}.h restated
    line by line in plain Python -- small graphs only;
  * raw_sums(g): the eleven raw sums of gm_sgl5_raw (T, D, W, A, B, H, S, P, K4, R, Q) from numpy / Python integers, K4 and R from the CPU
    oracle; `need` limits the work on large graphs;
  * finish(pattern, raw): the closed forms, modulo 2^64;
  * complete_raw(n): the sums of K_n in closed form.
"""
from __future__ import annotations

from math import comb

import numpy as np

PATTERNS = ("hourglass", "taileddiamond", "taileddiamond2", "closedhouse", "semihouse", "5path")
RAW = ("T", "D", "W", "A", "B", "H", "S", "P", "K4", "R", "Q")
M64 = 2**64


def adjacency(g):
    rp, ci = np.asarray(g.row_ptr), np.asarray(g.col_idx)
    return [ci[rp[v]:rp[v + 1]].tolist() for v in range(len(rp) - 1)]


def loops(g, pattern: str) -> int:
    N = adjacency(g)
    S = [set(a) for a in N]
    nv, counter = len(N), 0

    def inter(a, b, upper=None):  # intersection_set(N(a), N(b)[, upper]), ascending
        return [x for x in N[a] if x in S[b] and (upper is None or x < upper)]

    if pattern == "hourglass":
        for v0 in range(nv):
            for v1 in N[v0]:
                for v2 in inter(v0, v1, v1):
                    for v3 in N[v0]:
                        if v3 >= v1:
                            break
                        if v3 == v2:
                            continue
                        counter += sum(1 for v4 in N[v0] if v4 in S[v3] and v4 < v3 and v4 != v2)
    elif pattern == "taileddiamond":
        for v0 in range(nv):
            for v1 in N[v0]:
                if v1 >= v0:
                    break
                a = inter(v0, v1)
                if len(a) > 1:
                    for v2 in a:
                        for v3 in a:
                            if v3 == v2:
                                continue
                            counter += sum(1 for v4 in N[v2] if v4 != v0 and v4 != v1 and v4 != v3)
    elif pattern == "taileddiamond2":
        for v0 in range(nv):
            for v1 in N[v0]:
                a = inter(v0, v1)
                if len(a) > 1:
                    for v2 in a:
                        for v3 in a:
                            if v3 >= v2:
                                break
                            counter += sum(1 for v4 in N[v0] if v4 != v1 and v4 != v2 and v4 != v3)
    elif pattern == "semihouse":
        for v0 in range(nv):
            for v1 in N[v0]:
                if v1 >= v0:
                    break
                for v2 in inter(v0, v1):
                    for v3 in inter(v0, v2):
                        if v3 == v1:
                            continue
                        counter += sum(1 for x in N[v1] if x in S[v2] and x != v0 and x != v3)
    elif pattern == "closedhouse":
        for v0 in range(nv):
            for v1 in N[v0]:
                if v1 >= v0:
                    break
                y = inter(v0, v1)
                for v2 in y:
                    for v3 in y:
                        if v3 == v2:
                            continue
                        counter += sum(1 for x in y if x in S[v3] and x != v2)
    elif pattern == "5path":
        for v0 in range(nv):
            for v1 in N[v0]:
                for v2 in N[v0]:
                    if v2 >= v1:
                        break
                    for v3 in N[v2]:
                        if v3 == v0 or v3 == v1:
                            continue
                        counter += sum(1 for v4 in N[v1] if v4 != v0 and v4 != v2 and v4 != v3)
    else:
        raise ValueError(pattern)
    return counter


def _c2(x: int) -> int:
    return x * (x - 1) // 2


SPARSE_MAX_ROWS = 10**8  # rows of several int64 arrays each: beyond this the enumeration below is killed for memory, not merely slow


def raw_sums(g, need=RAW) -> dict:
    """the raw sums named in `need` as exact Python integers modulo 2^64 (the others 0)"""
    rp, ci = np.asarray(g.row_ptr).astype(np.int64), np.asarray(g.col_idx).astype(np.int64)
    nv = len(rp) - 1
    deg = np.diff(rp)
    src = np.repeat(np.arange(nv, dtype=np.int64), deg)
    keys = src * nv + ci  # ascending: the CSR order
    out = dict.fromkeys(RAW, 0)
    need = set(need)
    if need & {"T", "D", "W", "A", "B", "H", "S", "Q"}:
        und = src < ci
        eu, ev = src[und], ci[und]
        ne = len(eu)
        ekeys = eu * nv + ev  # ascending
        short_is_u = deg[eu] <= deg[ev]
        s_end, l_end = np.where(short_is_u, eu, ev), np.where(short_is_u, ev, eu)
        cnt = deg[s_end]
        if int(cnt.sum()) > SPARSE_MAX_ROWS:
            raise ValueError(f"sgl5_ref.raw_sums: {int(cnt.sum())} (edge, key of the shorter list) rows are beyond the sparse enumeration "
                             f"(limit {SPARSE_MAX_ROWS}); a dense graph of a few thousand vertices goes through dense_graded.dense_raw5")
        eid = np.repeat(np.arange(ne, dtype=np.int64), cnt)
        off = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        w = ci[np.repeat(rp[s_end], cnt) + off]  # every key of the shorter list
        q = np.repeat(l_end, cnt) * nv + w
        pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
        hit = keys[pos] == q
        eid, w = eid[hit], w[hit]  # one row per (edge, common neighbour): every triangle three times
        t = np.bincount(eid, minlength=ne)
        tl, dl = t.tolist(), deg.tolist()
        eul, evl = eu.tolist(), ev.tolist()
        out["T"] = sum(tl) // 3
        out["D"] = sum(_c2(x) for x in tl)
        out["W"] = sum(_c2(x) * (dl[a] + dl[b] - 6) for x, a, b in zip(tl, eul, evl))
        tv = [0] * nv
        for x, a, b in zip(tl, eul, evl):
            tv[a] += x
            tv[b] += x
        assert all(x % 2 == 0 for x in tv)
        tv = [x // 2 for x in tv]
        out["H"] = sum(_c2(x) for x in tv)
        out["S"] = sum(x * d for x, d in zip(tv, dl))
        if need & {"A", "B"}:
            a_end, b_end = eu[eid], ev[eid]
            e1 = np.searchsorted(ekeys, np.minimum(a_end, w) * nv + np.maximum(a_end, w))
            e2 = np.searchsorted(ekeys, np.minimum(b_end, w) * nv + np.maximum(b_end, w))
            x = (t - 1).tolist()
            A = B2 = 0
            for e, ww, f1, f2 in zip(eid.tolist(), w.tolist(), e1.tolist(), e2.tolist()):
                A += x[e] * (dl[ww] - 2)
                B2 += x[e] * (x[f1] + x[f2])
            assert B2 % 2 == 0
            out["A"], out["B"] = A, B2 // 2
        if "Q" in need:
            adj = [set(a) for a in adjacency(g)]
            members = [[] for _ in range(ne)]
            for e, ww in zip(eid.tolist(), w.tolist()):
                members[e].append(ww)
            Q = 0
            for m in members:
                if len(m) >= 3:
                    ms = set(m)
                    Q += (len(m) - 2) * sum(len(ms & adj[c]) for c in m)
            out["Q"] = Q
    if "P" in need:
        x = (deg - 1)[ci]
        e1l, p2l = [0] * nv, [0] * nv
        for v, y in zip(src.tolist(), x.tolist()):
            e1l[v] += y
            p2l[v] += y * y
        out["P"] = sum((a * a - b) // 2 for a, b in zip(e1l, p2l))
    if need & {"K4", "R"}:
        import oracle as O

        sym = O.OGraph(g.row_ptr, g.col_idx)
        if "K4" in need:
            out["K4"] = O.clique(O.orient(sym), 4)
        if "R" in need:
            out["R"] = O.rectangle(sym)
    return {k: (v % M64 if k in need else 0) for k, v in out.items()}


def complete_raw(n: int) -> dict:
    """K_n: t = n - 2, d = n - 1, T_v = C(n - 1, 2), K4 = C(n, 4) (P, R, Q left 0: closedhouse and 5path are not asked of it)"""
    t, d, x = n - 2, n - 1, n - 3
    tri, e = comb(n, 3), comb(n, 2)
    out = dict.fromkeys(RAW, 0)
    out.update(T=tri, D=e * _c2(t), W=e * _c2(t) * (2 * d - 6), A=tri * 3 * x * (d - 2), B=tri * 3 * x * x, H=n * _c2(comb(n - 1, 2)),
               S=n * comb(n - 1, 2) * d, K4=comb(n, 4))
    return {k: v % M64 for k, v in out.items()}


def finish(pattern: str, raw) -> int:
    r = raw if isinstance(raw, dict) else dict(zip(RAW, raw))
    v = {"hourglass": r["H"] - 2 * r["D"], "taileddiamond2": r["W"], "taileddiamond": r["A"] - 12 * r["K4"],
         "semihouse": r["B"] - 12 * r["K4"], "closedhouse": r["Q"], "5path": r["P"] - 2 * r["S"] + 9 * r["T"] - 4 * r["R"]}[pattern]
    return v % M64
