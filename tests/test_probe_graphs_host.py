"""The probe graphs of tests/probe_graphs.py hold what they promise (no GPU): under the CPU oracle's orientation every named row has the
promised length, the streamed list of every gadget is the promised list with its matches at the promised positions -- as numbered and on
the topological copy (the numpy restatement of the renumbering, common.renumbered_expected) --, the hub rows are empty, the longest row
fits the stage meant, and the oracle's triangle, diamond and 4-clique counts are the sums over the gadgets: the expected values the GPU
tests compare against (tests/test_gpu_probe_lists.py) rest on the reference, not on the builder's arithmetic."""
import functools
from math import comb

import numpy as np
import pytest

import oracle as O
import probe_graphs as PG
from common import renumbered_expected, renumbering
from graphminer_amd.graph import Graph


@functools.lru_cache(maxsize=2)
def oriented(key):
    """(probe, oracle's symmetric graph, its orientation) of probe `key`; the two latest are kept"""
    p = {"s1024": lambda: PG.single("s1024"), "s2048": lambda: PG.single("s2048"), "k4": PG.k4, "salt": PG.salt, "surplus": PG.surplus}.get(key)
    p = p() if p else PG.batch(*key)
    sym = O.OGraph(p.graph.row_ptr, p.graph.col_idx)
    return p, sym, O.orient(sym)


def row(dag, x):
    return dag.col_idx[dag.row_ptr[x]:dag.row_ptr[x + 1]]


def check_totals(p, sym, dag, diamonds=None):
    """the expected triangles are distinct triangles of the graph and as many as the oracle counts: they are all of them; likewise the
    4-cliques; the diamonds from the expected supports"""
    t = p.triangles.astype(np.int64)
    assert len(np.unique(t, axis=0)) == len(t) and ((t[:, 0] < t[:, 1]) & (t[:, 1] < t[:, 2])).all()
    for i, j in ((0, 1), (0, 2), (1, 2)):
        p.entry_of(t[:, i], t[:, j])  # asserts the edge
    assert O.tc(dag) == p.tri_total == sum(g.tri for g in p.gadgets)
    q = p.cliques4.astype(np.int64)
    for i in range(4):
        for j in range(i + 1, 4):
            p.entry_of(q[:, i], q[:, j])
    assert O.clique(dag, 4) == len(q) == len(np.unique(q, axis=0)) == sum(g.cliques4 for g in p.gadgets)
    want = O.diamond(sym)
    assert want == p.diamonds()
    if diamonds is not None:
        assert want == diamonds
    sup = p.supports()
    src = np.repeat(np.arange(p.graph.V()), np.diff(p.graph.row_ptr))
    assert np.array_equal(np.bincount(src, weights=sup, minlength=p.graph.V()).astype(np.uint64), 2 * p.vertex_triangles())


def check_hubs(p, dag, stage, hub_row_max=0):
    rows = np.diff(dag.row_ptr)
    deg = np.diff(p.graph.row_ptr)
    assert (deg[p.hubs] == p.D).all() and deg[:p.n_core][p.owner >= 0].max() < p.D
    assert rows[p.hubs].max() <= hub_row_max
    assert stage // 2 < rows.max() <= stage


def streamed(dag_row_s, dag_row_t, t, topo):
    """the DAG edge s -> t: (the list streamed, the row it is looked up in), by the host rule of csrc/gm_tasks.hip"""
    i = int(np.flatnonzero(dag_row_s == t)[0])
    tail = len(dag_row_s) - i - 1 if topo else len(dag_row_s)
    if PG.hosts_as_source(tail, len(dag_row_t)):
        return dag_row_t, dag_row_s
    return (dag_row_s[i + 1:] if topo else dag_row_s), dag_row_t


@pytest.mark.parametrize("name", ["s1024", "s2048", "k4"])
def test_single_lists(name):
    p, sym, dag = oriented(name)
    check_hubs(p, dag, 1024 if name == "s1024" else 2048, hub_row_max=2 if name == "k4" else 0)
    newid = renumbering(np.diff(p.graph.row_ptr))
    trp, tci = renumbered_expected(Graph(row_ptr=dag.row_ptr, col_idx=dag.col_idx), np.diff(p.graph.row_ptr), False)
    hub_new = newid[p.hubs]
    assert (np.diff(hub_new) > 0).all()  # the hubs keep their relative order
    seen = set()
    for g in p.gadgets:
        rv, ru = row(dag, g.v), row(dag, g.u)
        assert len(rv) == g.L + 1 and len(ru) == g.A and rv[0] == g.u, g.label
        assert np.array_equal(rv[1:], g.S) and np.array_equal(ru, g.R), g.label
        assert np.array_equal(np.flatnonzero(np.isin(rv, ru)), g.P + 1), g.label
        # as numbered: u hosts and streams row(v) when L + 1 < A, else v hosts and streams row(u)
        lst, host_row = streamed(rv, ru, g.u, topo=False)
        if g.L + 1 < g.A:
            assert len(lst) == g.L + 1 and lst[0] == g.u and np.array_equal(np.flatnonzero(np.isin(lst, host_row)), g.P + 1), g.label
        else:
            assert np.array_equal(lst, g.R) and np.array_equal(lst[np.isin(lst, host_row)], g.S[g.P]), g.label
        # the topological copy: the trimmed tail of L keys, the matches at P
        nv_, nu = newid[g.v], newid[g.u]
        tv, tu = tci[trp[nv_]:trp[nv_ + 1]], tci[trp[nu]:trp[nu + 1]]
        assert tv[0] == nu and np.array_equal(tv[1:], newid[g.S]) and np.array_equal(tu, newid[g.R]), g.label
        lst, host_row = streamed(tv, tu, nu, topo=True)
        if g.L < g.A:
            assert len(lst) == g.L and np.array_equal(np.flatnonzero(np.isin(lst, host_row)), g.P), g.label
        else:
            assert np.array_equal(lst, tu) and np.array_equal(lst[np.isin(lst, host_row)], newid[g.S[g.P]]), g.label
        seen.add((g.L, g.A))
    if name != "k4":
        A = 1023 if name == "s1024" else 2047
        lengths = PG.S1024_L if name == "s1024" else PG.S2048_L
        assert seen == {(L, A) for L in lengths} | {(L, L + k) for L in lengths if L < A for k in (0, 1)}
        assert len(p.gadgets) == 5 * len(lengths) + 2 * sum(L < A for L in lengths)
        assert any(g.P.size and g.P.max() >= 2 for g in p.gadgets)
        check_totals(p, sym, dag, diamonds=sum(comb(len(g.P), 2) for g in p.gadgets))
    else:
        for g in p.gadgets:
            h1, h2 = g.S[g.P]
            decoy = g.extra["decoy"]
            assert h2 in row(dag, h1) and (decoy in row(dag, h1) or h1 in row(dag, decoy)), g.label
            assert decoy in g.S and decoy not in g.R, g.label
        check_totals(p, sym, dag)


@pytest.mark.parametrize("M", [1024, 2048])
@pytest.mark.parametrize("ell", PG.BATCH_ELLS)
def test_batch_lists(M, ell):
    from graphminer_amd.dist import chunk_table

    p, sym, dag = oriented((M, ell))
    check_hubs(p, dag, M)
    (g,) = p.gadgets
    mids, tgt, pos = g.extra["mids"], g.extra["target"], g.extra["match_pos"]
    ru = row(dag, g.u)
    assert np.array_equal(ru, mids) and len(ru) == M and (np.diff(p.graph.row_ptr)[mids] == g.extra["Dm"]).all()
    assert (np.diff(dag.row_ptr)[mids] == ell).all()
    for k in range(3):
        assert abs(int((np.where(tgt < 0, 2, pos > 0) == k).sum()) - M // 3) <= 2  # a third each: first key, last key, no match
    lst, host_row = streamed(ru, row(dag, mids[0]), mids[0], topo=False)  # u hosts every task (tail = M >= ell) and streams the mid's row
    assert len(lst) == ell and host_row is ru
    rows = dag.col_idx[dag.row_ptr[mids][:, None] + np.arange(ell)[None, :]]  # the M streamed lists, one per line
    hit = np.isin(rows, ru)
    assert np.array_equal(hit.sum(axis=1), (tgt >= 0).astype(np.int64))       # one match or none ...
    has = np.flatnonzero(tgt >= 0)
    assert hit[has, pos[has]].all() and np.array_equal(rows[has, pos[has]], mids[tgt[has]])  # ... at position 0 or ell - 1: the mid pointed at
    assert set(pos[has].tolist()) == {0, ell - 1}
    # (the table of the default 1024-entry target; a launch halves its target on a graph this small, but a row of >= 1024 entries is a
    # chunk of its own at any target)
    recs = chunk_table(dag.row_ptr)
    assert tuple(recs[0][:2]) == (0, 1) and recs[0][2] == 0 and tuple(recs[1][:2]) != (0, 2)  # u starts a chunk and is alone in it
    if M == 1024:
        assert tuple(recs[0]) == (0, 1, 0, 1024)
    check_totals(p, sym, dag)


def test_salt_rows():
    from graphminer_amd.dist import chunk_table

    p, sym, dag = oriented("salt")
    n = PG.SALT_HOSTS
    rows = np.diff(dag.row_ptr)
    deg = np.diff(p.graph.row_ptr)
    assert (deg[p.hubs] == p.D).all() and rows[p.hubs].max() == 0 and n >= 600
    sets = (set(p.hubs[:8].tolist()), set(p.hubs[8:16].tolist()))
    for i, g in enumerate(p.gadgets):
        assert (g.v, g.u) == (i, n + i)  # consecutive partners, consecutive hosts
        ru, rv = row(dag, g.u), row(dag, g.v)
        assert len(ru) in (3, 4) and set(ru.tolist()) <= sets[i % 2] and np.array_equal(ru, g.R), g.label
        assert rv[0] == g.u and len(rv) - 1 in (2, 3) and np.array_equal(rv[1:], g.S), g.label
        hit = rv[np.isin(rv, ru)]
        assert len(hit) == g.tri == (0 if i % 3 == 1 else 1), g.label
        if i % 3 == 1 and i + 1 < n:  # the keys of a partner without a triangle are staged for the next host of the chunk
            assert set(rv[1:].tolist()) <= set(row(dag, g.u + 1).tolist()), g.label
        if i >= 128 and len(hit):  # a host tag that wraps at 128 rows looks the match up in a row that does not hold it
            assert hit[0] not in row(dag, g.u - 128) and hit[0] not in row(dag, g.v - 128), g.label
    assert dag.ne > 14 * 256 * 1024  # the launch keeps its chunk target of 1024 entries on a GPU of 256 CUs (see probe_graphs.SALT_HUBS)
    recs = chunk_table(dag.row_ptr)
    full = [r for r in recs if r[1] - r[0] == 256]
    assert any(r[0] >= n and r[1] <= 2 * n for r in full) and any(r[1] <= n for r in full)  # 256 hosts (partners) in one chunk
    check_totals(p, sym, dag, diamonds=0)


def test_surplus_rows():
    from graphminer_amd.dist import chunk_table

    p, sym, dag = oriented("surplus")
    rows = np.diff(dag.row_ptr)
    assert rows[p.hubs].max() == 0 and rows.max() == 132 and p.graph.V() == 1 << 24
    # (the default 1024-entry target; the launch's smaller one changes nothing: every other row of a host's 512-vertex block is empty)
    recs = chunk_table(dag.row_ptr)
    for g in p.gadgets:
        ru, rv = row(dag, g.u), row(dag, g.v)
        assert len(ru) == g.A and np.array_equal(ru, g.R) and rv[0] == g.u and np.array_equal(rv[1:], g.S), g.label
        assert np.isin(g.S, g.R).all() and g.tri == g.L
        bucket = ((ru.astype(np.uint64) * np.uint64(PG.MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)  # TchHash<1024>::bucket, salt 0
        assert len(set(bucket.tolist())) == 1, g.label
        lst, host_row = streamed(rv, ru, g.u, topo=False)
        assert lst is rv and host_row is ru  # u hosts, as numbered
        (mine,) = [r for r in recs if r[0] <= g.u < r[1]]
        assert mine[0] == g.u and mine[3] - mine[2] == g.A, (g.label, mine)  # nothing but u's row in its chunk
    assert [g.A for g in p.gadgets] == [131, 132]
    check_totals(p, sym, dag)


@pytest.mark.parametrize("name", list(PG.SINGLE))
def test_single_slices(name):
    """the slices (one pattern, one class of lengths) partition the gadgets of the graph, keep its hubs and rows, and hold the triangles the
    oracle counts"""
    full = PG.single(name)
    n_hubs, D, lengths, A = PG.SINGLE[name]
    labels = []
    for pat in PG.SLICE_PATTERNS:
        for cls in PG.SLICE_CLASSES:
            p = PG.single(name, pat, cls)
            dag = O.orient(O.OGraph(p.graph.row_ptr, p.graph.col_idx))
            rows = np.diff(dag.row_ptr)
            assert len(p.hubs) == n_hubs and (np.diff(p.graph.row_ptr)[p.hubs] == D).all() and rows[p.hubs].max() == 0
            assert rows.max() in (A, A + 1) or pat == "tie"
            for g in p.gadgets:
                assert len(row(dag, g.v)) == g.L + 1 and len(row(dag, g.u)) == g.A and row(dag, g.v)[0] == g.u, g.label
            assert O.tc(dag) == p.tri_total == sum(len(g.P) for g in p.gadgets), p.name
            labels += [g.label.split(" ", 1)[1] for g in p.gadgets]
    assert sorted(labels) == sorted(g.label.split(" ", 1)[1] for g in full.gadgets)
