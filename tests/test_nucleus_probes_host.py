"""The probe graphs of tests/nucleus_probes.py hold what they promise (no GPU), and the conditions the GPU tests of
tests/test_gpu_nucleus34_probes.py rest on are asserted here, on the reference alone: the by-construction K4(t) equal the enumeration of
tests/nucleus34_ref.py, the orientation assumed equals the CPU oracle's, the matched triangles of an entry have pairwise different counts,
the look-ups reach every (sibling, branch, tie) case and the segment lengths on both sides of the wave, the trips mix whole-wave and group
units at every slot, the dense cell's rounds meet every case of the blocked rule -- and a lane model of the index build and of the gather,
written from DESIGN.md, reproduces the expected arrays and loses at least one of them under each of six mutations.

Time of the Python reference per probe graph, measured on the development machine (one core): index 1.5 s for K4(t) and 1.9 s for the
rounds (397,266 vertices, most of them leaves; 4,122 triangles, 8,706 cliques); walk and trips 0.1 s each (3,653 and 283 triangles); the
dense cell of 56 vertices 1.4 s (18,294 triangles, 161,863 cliques; its census 3.5 s)."""
import functools

import numpy as np
import pytest

import nucleus34_ref as R
import nucleus_probes as NP
import oracle as O
from common import gm_constant

FAMILIES = {"index": NP.index, "walk": NP.walk, "trips": NP.trips}


@functools.lru_cache(maxsize=None)
def built(name):
    group, whole = gm_constant("nuc_group"), gm_constant("nuc_whole_wave")
    p = FAMILIES[name](group, whole)
    return p, NP.Structure(p.graph), group, whole


@pytest.mark.parametrize("name", list(FAMILIES))
def test_expected_values_are_the_reference(name):
    p, st, _, _ = built(name)
    k4 = R.k4(p.graph)
    print(f"{name}: {p.graph.V()} vertices, {len(p.want)} triangles by construction, {len(k4)} enumerated, {sum(k4.values()) // 4} cliques", flush=True)
    assert p.triangles == R.triangles(p.graph)
    bad = [t for t in k4 if k4[t] != p.want[t]]
    assert not bad, [(t, p.where[t], p.want[t], k4[t]) for t in bad[:5]]
    assert all(t in p.where for t in k4)
    # what the kernels walk: the triangles in the listing's order are the same set, the segments hold the same counts
    got = {tuple(sorted(int(x) for x in st.tris[i])): int(st.k4[i]) for i in range(len(st.tris))}
    assert got == p.want
    assert len(set(g.label for g in p.gadgets)) == len(p.gadgets)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_orientation_is_the_oracles(name):
    p, st, _, _ = built(name)
    dag = O.orient(O.OGraph(p.graph.row_ptr, p.graph.col_idx))
    assert np.array_equal(np.asarray(dag.row_ptr), st.drp) and np.array_equal(np.asarray(dag.col_idx), st.dcol)
    assert O.tc(dag) == len(p.want)


def test_index_gadgets():
    p, st, group, whole = built("index")
    seen = set()
    for g in p.gadgets:
        v, u = g.corners
        rv, ru = st.orow(v), st.orow(u)
        assert rv[0] == u and len(rv) == g.extra["L"] + 1 and len(ru) == g.extra["A"], g.label
        e = int(st.drp[v])
        assert st.dcol[e] == u and st.sn[e] == g.sn and bool(st.u_short[e]) == (g.way != "u"), g.label
        streamed = rv if g.way != "u" else ru
        looked = ru if g.way != "u" else rv
        assert np.array_equal(np.flatnonzero(np.isin(streamed, looked)), g.P), g.label
        assert st.seg.get(e, []) == g.matched.tolist(), g.label
        if g.way == "tie":
            assert len(rv) == len(ru), g.label
        values = [p.want[tuple(sorted((v, u, int(m))))] for m in g.matched]
        if len(values) >= 2:  # a triangle written to the wrong slot of its segment shows
            assert len(set(values)) == len(values) and values == list(range(len(values))), (g.label, values)
        assert len(g.P) <= NP.MAX_MATCHES
        seen.add((g.sn, g.pattern, g.way, g.sn >= whole))
    assert seen == {(sn, pat, way, sn >= whole) for sn, pat, way in NP.index_specs()}
    assert {sn for sn, _, _, w in seen if not w} == set(NP.INDEX_GROUP_SN) and {sn for sn, _, _, w in seen if w} == set(NP.INDEX_WAVE_SN)
    last = [g for g in p.gadgets if g.pattern == "last"]
    assert all(g.P.tolist() == [g.sn - 1] for g in last if g.sn > 1)
    # the tiles pattern: a match in the last lane of one group's trip of keys and in the first of the next, on the group path
    assert any(g.sn < whole and {group - 1, group} <= set(g.P.tolist()) for g in p.gadgets)
    assert any(g.sn >= whole and {whole - 1, whole} <= set(g.P.tolist()) and g.P.max() >= 2 * whole - 2 for g in p.gadgets)
    hubs = np.flatnonzero(st.deg == st.deg.max())
    assert all(st.deg[int(m)] == st.deg.max() for g in p.gadgets for m in g.matched) and len(hubs) > 400  # re-padded to exactly D


def test_walk_gadgets():
    p, st, group, whole = built("walk")
    tri_at = {tuple(int(x) for x in st.tris[i]): i for i in range(len(st.tris))}
    kinds = set()
    for g in p.gadgets:
        u, v, w = g.corners
        assert (u, v, w) in tri_at, g.label  # u -> v -> w in the orientation
        assert st.deg[u] == g.sn, g.label
        memb = st.members(tri_at[(u, v, w)])
        assert np.array_equal(np.flatnonzero(memb), g.P), g.label
        r = st.row(u)
        in_v, in_w = np.isin(r, st.row(v)), np.isin(r, st.row(w))
        kinds |= {("v only", g.sn >= whole)} if (in_v & ~in_w & (r != w)).any() else set()
        kinds |= {("w only", g.sn >= whole)} if (in_w & ~in_v & (r != v)).any() else set()
        kinds |= {("neither", g.sn >= whole)} if (~in_w & ~in_v).any() else set()
        if g.pattern == "last":
            assert g.P.tolist() == [g.sn - 1], g.label
    assert kinds == {(k, wv) for k in ("v only", "w only", "neither") for wv in (False, True)}
    assert {g.sn for g in p.gadgets if g.pattern != "all"} == set(NP.WALK_GROUP_DU + NP.WALK_WAVE_DU)
    classes = {c for g in p.gadgets for c in g.extra["classes"]}
    assert classes == set(NP.CLASSES)


def test_lookups_reach_every_case():
    p, st, _, _ = built("walk")
    cases, rows, segments = NP.lookup_census(st)
    print("walk look-ups (sibling, branch, tie): " + ", ".join(f"{k}: {v}" for k, v in sorted(cases.items())), flush=True)
    assert set(cases) == {(s, b, t) for s in range(3) for b in range(3) for t in (False, True)}
    lens = sorted({n for n, _ in segments})
    print(f"bisected tri_w segments: lengths {lens}; bisected rows of the oriented copy: lengths {sorted({n for n, _ in rows})}", flush=True)
    for n in (1, 2, 63, 64, 65):
        assert (n, 0) in segments and (n, n - 1) in segments, n


def conditions_of_trips(ts, per):
    covered = set()
    for big, small in ts:
        if small:
            covered |= big
    between = any(any(a < b < c for a in big for c in big for b in set(range(per)) - big) for big, _ in ts if len(big) >= 2)
    return covered, between, any(not big for big, _ in ts), any(len(big) == per for big, _ in ts)


@pytest.mark.parametrize("unit", ["entry", "triangle"])
def test_trips_census(unit):
    p, st, group, whole = built("trips")
    per = whole // group
    ts = NP.trip_slots(st, unit, group, whole)
    covered, between, none, eight = conditions_of_trips(ts, per)
    print(f"trips, {unit}: {len(ts)} trips; whole-wave slots beside a group unit of non-zero value {sorted(covered)}; two whole-wave units around a "
          f"group unit {between}; a trip without {none}; a trip of {per} {eight}", flush=True)
    assert covered == set(range(per)) and between and none and eight


@functools.lru_cache(maxsize=None)
def dense_small():
    g, A = NP.dense_cell(NP.DENSE_SMALL)
    return g, A, R.round_census(g)


def test_dense_cells():
    whole = gm_constant("nuc_whole_wave")
    g, A = NP.dense_cell(NP.DENSE_BIG)
    st = NP.Structure(g)
    big = np.flatnonzero(st.sn >= whole)
    mixed = 0
    for e in big.tolist():
        a, b = int(st.src[e]), int(st.dcol[e])
        stream, looked = (st.orow(a), st.out[b]) if st.u_short[e] else (st.orow(b), st.out[a])
        found = np.array([int(x) in looked for x in stream[whole:2 * whole]])
        mixed += bool(found.any() and not found.all())
    k4 = NP.dense_k4(A)
    print(f"K_{NP.DENSE_BIG} cell: {len(st.tris)} triangles, {sum(k4.values()) // 4} cliques, {len(big)} entries of {whole} keys or more, {mixed} with "
          f"matches and non-matches in the second tile, {len(set(k4.values()))} different K4(t), longest oriented row {st.dplus.max()}", flush=True)
    assert len(big) >= 500 and mixed >= 50 and len(set(k4.values())) >= 32
    assert len(k4) == len(st.tris) and all(k4[tuple(sorted(int(x) for x in st.tris[i]))] == st.k4[i] for i in range(0, len(st.tris), 97))
    # the small sibling: the matrix products against the enumeration, and the rounds' census
    g, A, census = dense_small()
    assert NP.dense_k4(A) == R.k4(g)
    print(f"K_{NP.DENSE_SMALL} cell, the rounds: " + ", ".join(f"{k}: {v}" for k, v in sorted(census.items(), key=str)), flush=True)
    for n in (1, 2, 3, 4):
        assert census[("destroyed: frontier triangles", n)] > 0, n
    for sib in range(3):
        assert census[("skipped: a sibling removed earlier", sib)] > 0 and census[("skipped: a sibling in the frontier at a smaller id", sib)] > 0, sib
    assert sum(v for k, v in census.items() if k[0].startswith("destroyed")) == sum(R.k4(g).values()) // 4


# ---- sensitivity: the lane models ---------------------------------------------------------------------------------------------------------------
def model_outputs(name, mutant):
    p, st, group, whole = built(name)
    n_entries = int(st.drp[p.n_core])  # (the leaves' entries follow; their lists hold one key and match nothing)
    cnt, tri_w = NP.model_index(st, mutant, group, whole, n_entries)
    return cnt, tri_w, NP.model_walk(st, mutant, group, whole)


def expected_outputs(name):
    p, st, _, _ = built(name)
    n_entries = int(st.drp[p.n_core])
    assert st.tri_off[n_entries] == len(st.tris)
    return np.diff(st.tri_off)[:n_entries], st.tri_w, st.k4


@pytest.mark.parametrize("name", list(FAMILIES))
def test_lane_model_reproduces_the_expected_arrays(name):
    for got, want, what in zip(model_outputs(name, None), expected_outputs(name), ("c(e)", "tri_w", "K4(t)")):
        assert np.array_equal(got, want), (name, what)


@pytest.mark.parametrize("mutant", NP.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for name in FAMILIES:
        p, st, _, _ = built(name)
        for got, want, what in zip(model_outputs(name, mutant), expected_outputs(name), ("c(e)", "tri_w", "K4(t)")):
            bad = np.flatnonzero(got != want) if got.shape == want.shape else np.array([0])
            if bad.size:
                i = int(bad[0])
                if what == "c(e)":
                    t = int(st.tri_off[i]) if st.tri_off[i + 1] > st.tri_off[i] else None
                    label = p.label_of(sorted(int(x) for x in st.tris[t])) if t is not None else f"entry {int(st.src[i])} -> {int(st.dcol[i])}"
                else:
                    label = p.label_of(sorted(int(x) for x in st.tris[min(i, len(st.tris) - 1)]))
                caught.append(f"{name} {what}: {bad.size} values, the first at {i} ({label})")
    print(f"mutant '{mutant}': " + ("; ".join(caught) if caught else "NOT CAUGHT"), flush=True)
    assert caught, mutant
