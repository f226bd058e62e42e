"""The triangle nuclei on the GPU against the position-exact probe graphs of tests/nucleus_probes.py (csrc/gm_nucleus34.hip: every path of
nuc_index_kernel, nuc_walk, nuc_id_with, the blocked rule of nuc_peel_kernel, the second pass of the grid-stride loops).  tests/
test_nucleus_probes_host.py asserts on the CPU what the graphs hold and which cases they reach; here every comparison is exact: the
by-construction K4(t), tests/nucleus34_ref.py's rounds, a closed form, or float64 matrix products of integers far below 2^53.  A failure
prints the gadget's label (family/length/pattern/way) and the position inside the entry's segment or inside row u.  Every value is printed
before it is asserted."""
import functools

import numpy as np
import pytest

import nucleus34_ref as R
import nucleus_probes as NP
from common import gm_constant
from graphminer_amd import nucleus34, nucleus34_decompose, tri_clique4_local
from test_gpu_nucleus34 import REMOVED, book, check, check_arrays, check_decompose, check_nucleus, dev, rows_of  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu
FAMILIES = {"index": NP.index, "walk": NP.walk, "trips": NP.trips}
LABELS = [f"index/sn={sn}/{pat}/{way}" for sn, pat, way in NP.index_specs()] + [f"walk/du={du}/{pat}" for du, pat in NP.walk_specs()]


@functools.lru_cache(maxsize=None)
def probe(name):
    return FAMILIES[name](gm_constant("nuc_group"), gm_constant("nuc_whole_wave"))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(prepared enumeration, its decomposition, {c: the fixed-c form at c_max // 2 and c_max})"""
    state = R.prepare(probe(name).graph)
    d = R.decompose(state)
    return state, d, {c: R.nucleus(state, c) for c in sorted({d.c_max // 2, d.c_max})}


def explain(p, what, rows, got, want):
    """the labels of the first rows that differ, before the checker asserts"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape:
        for i in np.flatnonzero(got != want)[:8].tolist():
            print(f"{what}: triangle {i} {rows[i].tolist()} got {int(got[i])} want {int(want[i])} -- {p.label_of(sorted(rows[i].tolist()))}", flush=True)


def check_family(name, dev):
    """the three calls on one probe graph through the suite's checkers; returns what the per-label test reads"""
    p = probe(name)
    state, d, fixed = reference(name)
    print(f"{name}: {p.graph.V()} vertices, {len(p.want)} triangles, {d.destroyed} cliques, c_max {d.c_max}, rounds {d.rounds}", flush=True)
    with p.graph.to_device(dev) as sym:
        rows = rows_of(sym)
        total, k4 = tri_clique4_local(sym)
        check(f"{name} (T, 4-cliques)", (k4.shape[0], total), (len(p.want), sum(p.want.values()) // 4))
        want_k4 = R.ordered(rows, p.want)
        explain(p, f"{name} K4(t)", rows, k4, want_k4)
        check_arrays(f"{name} K4(t) against the values by construction", k4, want_k4)
        theta, rnd, _, _ = nucleus34_decompose(sym)
        explain(p, f"{name} theta", rows, theta, R.ordered(rows, d.theta))
        explain(p, f"{name} round", rows, rnd, R.ordered(rows, d.round))
        check_decompose(name, sym, d, rows)
        cnts = {}
        for c, want in fixed.items():
            cnt = nucleus34(sym, c)[2]
            explain(p, f"{name} c={c}", rows, cnt, R.ordered(rows, want.cnt))
            cnts[c] = check_nucleus(name, sym, c, want, rows)
    return rows, k4, theta, rnd, cnts


_RESULTS = {}


def family_results(name, dev):
    """check_family once per family; a failure is kept and raised again for every label of the family"""
    if name not in _RESULTS:
        try:
            _RESULTS[name] = check_family(name, dev)
        except BaseException as e:  # noqa: BLE001
            _RESULTS[name] = e
    if isinstance(_RESULTS[name], BaseException):
        raise _RESULTS[name]
    return _RESULTS[name]


@functools.lru_cache(maxsize=None)
def rows_by_label(name):
    rows = family_results(name, 0)[0]
    p = probe(name)
    out = {}
    for i, r in enumerate(rows.tolist()):
        out.setdefault(p.label_of(sorted(r)).split(":")[0], []).append(i)
    return out


# ---- 1. index and walk, by label ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_gadget(dev, label):
    name = label.split("/")[0]
    p = probe(name)
    _, d, fixed = reference(name)
    rows, k4, theta, rnd, cnts = family_results(name, dev)
    idx = rows_by_label(name).get(label, [])
    (g,) = [g for g in p.gadgets if g.label == label]
    print(f"{label}: {len(idx)} triangles, matches at positions {g.P.tolist()}", flush=True)
    for i in idx:
        t = tuple(sorted(rows[i].tolist()))
        got = (int(k4[i]), int(theta[i]), int(rnd[i])) + tuple(int(cnts[c][i]) for c in fixed)
        want = (p.want[t], d.theta[t], d.round[t]) + tuple(fixed[c].cnt[t] for c in fixed)
        print(f"  {p.where[t]}: (K4, theta, round, {', '.join(f'c={c}' for c in fixed)}) got {got} want {want}", flush=True)
        assert got == want, p.where[t]
    assert len(idx) == sum(1 for t in p.want if p.where[t].split(":")[0] == label)


@pytest.mark.parametrize("name", ["index", "walk"])
def test_family(dev, name):
    family_results(name, dev)


# ---- 2. whole-wave and group units in one trip ---------------------------------------------------------------------------------------------------
def test_trips(dev):
    p = probe("trips")
    st = NP.Structure(p.graph)
    group, whole = gm_constant("nuc_group"), gm_constant("nuc_whole_wave")
    for unit in ("entry", "triangle"):
        ts = [(sorted(big), sorted(small)) for big, small in NP.trip_slots(st, unit, group, whole) if big]
        print(f"trips, {unit}: (whole-wave slots, group slots of non-zero value) of the trips with a whole-wave unit: {ts}", flush=True)
    family_results("trips", dev)


# ---- 3. a dense cell with long oriented rows -----------------------------------------------------------------------------------------------------
def test_dense_cell_long_rows(dev):
    """K_130 minus a seeded, graded set of edges: oriented rows of 64 .. 100 keys, matches and non-matches in the second tile, 57 different
    K4(t) (the conditions: tests/test_nucleus_probes_host.py).  K4(t) against float64 products of the dense adjacency matrix; of the
    decomposition the totals and invariants -- the enumeration of 5 M cliques is too slow for the Python rounds"""
    g, A = NP.dense_cell(NP.DENSE_BIG)
    want = NP.dense_k4(A)
    cliques = sum(want.values()) // 4
    with g.to_device(dev) as sym:
        rows = rows_of(sym)
        total, k4 = tri_clique4_local(sym)
        check(f"K_{NP.DENSE_BIG} cell (T, 4-cliques)", (k4.shape[0], total), (len(want), cliques))
        check_arrays(f"K_{NP.DENSE_BIG} cell K4(t) against the matrix products", k4, R.ordered(rows, want))
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)  # (the call checks that it destroyed every clique and removed every triangle)
        check(f"K_{NP.DENSE_BIG} cell c_max against theta", c_max, int(theta.max()))
        check(f"K_{NP.DENSE_BIG} cell theta <= K4(t), the smallest theta = the smallest K4(t), every triangle in a round 1 .. rounds - 1",
              (bool((theta <= k4).all()), int(theta.min()), int(rnd.min()) >= 1, int(rnd.max()) == rounds - 1), (True, int(k4.min()), True, True))
        ntri, ncl, cnt, _ = nucleus34(sym, c_max)
        inside = cnt != REMOVED
        check(f"K_{NP.DENSE_BIG} cell c = c_max: the set is theta >= c_max, 4 x cliques = the surviving counts, every count >= c_max",
              (bool(np.array_equal(inside, theta >= c_max)), 4 * ncl, ntri, bool((cnt[inside] >= c_max).all())),
              (True, int(cnt[inside].astype(np.int64).sum()), int(inside.sum()), True))
        ntri, ncl, cnt, _ = nucleus34(sym, c_max + 1)
        check(f"K_{NP.DENSE_BIG} cell c = c_max + 1", (ntri, ncl, np.unique(cnt).tolist()), (0, 0, [REMOVED]))


def test_dense_cell_rounds(dev):
    """the sibling built the same way from K_56 (the Python rounds on K_72's 0.5 M cliques take more than a few seconds): every theta,
    every round; its rounds meet every case of the blocked rule (tests/test_nucleus_probes_host.py)"""
    g, A = NP.dense_cell(NP.DENSE_SMALL)
    state = R.prepare(g)
    want = R.decompose(state)
    print(f"K_{NP.DENSE_SMALL} cell: {len(want.theta)} triangles, {want.destroyed} cliques, c_max {want.c_max}, rounds {want.rounds}", flush=True)
    with g.to_device(dev) as sym:
        rows = rows_of(sym)
        _, k4 = tri_clique4_local(sym)
        check_arrays(f"K_{NP.DENSE_SMALL} cell K4(t) against the matrix products", k4, R.ordered(rows, NP.dense_k4(A)))
        check_decompose(f"K_{NP.DENSE_SMALL} cell", sym, want, rows)
        for c in (want.c_max // 2, want.c_max):
            check_nucleus(f"K_{NP.DENSE_SMALL} cell", sym, c, R.nucleus(state, c), rows)


# ---- 4. the second pass of the grid-stride loops --------------------------------------------------------------------------------------------------
def test_book_past_one_pass_of_the_grid(dev):
    """nuc_mark_kernel and nuc_out_kernel run at most 8 blocks of 256 lanes per CU: a book with more triangles than that takes a second
    trip through both loops, and the frontier's slots of round 1 are reserved across the two.  By the closed form of test_book"""
    import torch

    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    one_pass = 8 * cus * 256
    m = one_pass // 3 + 238
    T = 3 * m + 1
    print(f"{cus} CUs: one pass of the grid covers {one_pass} triangles, the book of {m} pages has {T}", flush=True)
    assert T > one_pass
    with book(m).to_device(dev) as sym:
        rows = rows_of(sym)
        centre = int(np.flatnonzero((rows == (0, 1, 2)).all(axis=1))[0])
        theta, rnd, c_max, rounds = nucleus34_decompose(sym)
        check(f"book {m} (T, theta, c_max, rounds)", (theta.shape[0], np.unique(theta).tolist(), c_max, rounds), (T, [1], 1, 3))
        check(f"book {m} rounds per triangle: the centre in round 2", (int(rnd[centre]), int((rnd == 2).sum()), int((rnd == 1).sum())), (2, 1, 3 * m))
        ntri, ncl, cnt, rounds = nucleus34(sym, 1)
        check(f"book {m} c = 1", (ntri, ncl, int(cnt[centre]), np.unique(np.delete(cnt, centre)).tolist(), rounds), (T, m, m, [1], 1))
        ntri, ncl, cnt, rounds = nucleus34(sym, 2)
        check(f"book {m} c = 2", (ntri, ncl, np.unique(cnt).tolist(), rounds), (0, 0, [REMOVED], 3))
