"""The ground truth of the local 4-cycle counts (tests/rect_local_ref.py) and the planted-square graphs (tests/planted_squares.py) on the
CPU: the reference against the `rectangle` goldens of the reference binaries, against a listing of every cycle, against closed forms and
against its own identities; and, for every cell of tests/test_gpu_rect_local.py, the conditions its inputs have to meet for the GPU
comparison to mean something -- those on the values (input_conditions) and those that place the cell on its path of the kernel (cell_path,
against the constants the library exports)."""
import functools
from math import comb

import numpy as np
import pytest

import planted_squares as P
import rect_local_ref as R
from common import GOLDEN, load_graph, random_graph

GOLDEN_SMALL = [n for n in ("citeseer", "cora") + tuple(k for k, e in GOLDEN.items() if isinstance(e, dict) and e.get("kind") == "rmat" and e["scale"] <= 10)]


def from_pairs(nv, pairs):
    s, d = np.asarray(pairs, dtype=np.int64).T
    return P._graph(nv, s, d)


def row_sums(g, ent):
    return np.add.reduceat(np.r_[ent, np.uint64(0)], g.row_ptr[:-1].astype(np.int64))[: g.V()] * (np.diff(g.row_ptr) > 0)


@functools.lru_cache(maxsize=None)
def consts():
    return P.constants()


@functools.lru_cache(maxsize=None)
def cell(name):
    g = P.cell_graph(name, consts())
    return (g,) + R.rect_local(g)


def test_golden_list():
    assert set(GOLDEN_SMALL) == {"citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"}
    assert (GOLDEN["citeseer"]["rectangle"], GOLDEN["cora"]["rectangle"]) == (6059, 4664)


@pytest.mark.parametrize("name", GOLDEN_SMALL)
def test_reference_against_the_goldens(name):
    g = load_graph(name)
    assert g.V() <= 1024 or name in ("citeseer", "cora")
    ent, rv = R.rect_local(g)
    total = R.total(rv)
    print(f"{name}: sum R_v / 4 = {total}, golden {GOLDEN[name]['rectangle']}; sum of the entries {int(ent.sum())}", flush=True)
    assert total == GOLDEN[name]["rectangle"]
    assert int(ent.sum()) == 8 * total
    assert np.array_equal(row_sums(g, ent), 2 * rv)  # R_v is half its row sum
    assert P.input_conditions(g, ent)[2]             # both directions of an edge are equal


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_against_a_listing_of_every_cycle(seed):
    g = random_graph(40, 220, seed) if seed < 3 else load_graph("rmat6_ef4_s1")
    ent, rv = R.rect_local(g)
    want_ent, want_rv = R.brute_force(g)
    assert want_ent.any() and np.array_equal(ent, want_ent) and np.array_equal(rv, want_rv)
    assert ent.dtype == np.uint64 and rv.dtype == np.uint64


def test_closed_forms():
    c4 = from_pairs(4, [(0, 1), (1, 2), (2, 3), (3, 0)])
    ent, rv = R.rect_local(c4)
    assert ent.tolist() == [1] * 8 and rv.tolist() == [1] * 4 and R.total(rv) == 1
    k4 = from_pairs(4, [(a, b) for a in range(4) for b in range(a + 1, 4)])
    ent, rv = R.rect_local(k4)
    assert ent.tolist() == [2] * 12 and rv.tolist() == [3] * 4 and R.total(rv) == 3
    for a, b in ((2, 7), (3, 5), (6, 6)):
        g = from_pairs(a + b, [(i, a + j) for i in range(a) for j in range(b)])
        ent, rv = R.rect_local(g)
        assert np.unique(ent).tolist() == [(a - 1) * (b - 1)], (a, b)
        assert rv.tolist() == [(a - 1) * comb(b, 2)] * a + [(b - 1) * comb(a, 2)] * b
        assert R.total(rv) == comb(a, 2) * comb(b, 2)
    q4 = from_pairs(16, [(v, v ^ (1 << i)) for v in range(16) for i in range(4) if v < v ^ (1 << i)])
    ent, rv = R.rect_local(q4)  # every edge of Q_d lies in d - 1 squares, every vertex in C(d, 2)
    assert np.unique(ent).tolist() == [3] and np.unique(rv).tolist() == [6] and R.total(rv) == 24
    tree = from_pairs(15, [(v, (v - 1) // 2) for v in range(1, 15)])
    petersen = from_pairs(10, [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)])
    for g in (tree, petersen, P.windmill(30, 50)):  # (the Petersen graph has girth 5)
        ent, rv = R.rect_local(g)
        assert not ent.any() and not rv.any()


def test_k2n_and_the_windmill():
    """the two graphs the GPU tests take closed forms for, at a size the reference finishes"""
    n = 300
    g = P.k2n(n)
    ent, rv = R.rect_local(g)
    assert np.unique(ent).tolist() == [n - 1] and rv.tolist() == [n - 1] * n + [comb(n, 2)] * 2
    assert comb(92700, 2) > 2 ** 32 > 92700 and 4 * 92700 < 2 ** 31
    w = P.windmill(300, 5000)
    assert int(np.diff(w.row_ptr).max()) == 5600 > consts()["range"] and not R.rect_local(w)[0].any()


@pytest.mark.parametrize("name", P.CELLS)
def test_cell_inputs(name):
    g, ent, rv = cell(name)
    distinct, nonzero, symmetric = P.input_conditions(g, ent)
    core = int((np.diff(g.row_ptr) >= 2).sum())
    print(f"{name}: {g.V()} vertices ({core} of degree >= 2), {g.E()} entries, {R.total(rv)} 4-cycles; {distinct} distinct non-zero entry values, "
          f"{nonzero:.3f} of the core entries non-zero, directions equal: {symmetric}", flush=True)
    assert distinct >= 32 and nonzero >= 0.5 and symmetric
    assert core <= 2600 and int(ent.sum()) == 8 * R.total(rv) and np.array_equal(row_sums(g, ent), 2 * rv)


@pytest.mark.parametrize("name", P.CELLS)
def test_cell_paths(name):
    g = cell(name)[0]
    for claim, holds in P.cell_path(name, g, consts()).items():
        print(f"{name}: {claim}: {holds}", flush=True)
        assert holds, claim


def test_small_range_on_rmat10():
    g = load_graph("rmat10_ef16_s42")
    for h in (P.degree_copy(g)[0], g):
        f = P.walk_facts(h, consts(), P.SMALL_RANGE)
        assert f.key_on_first and f.key_on_last and f.cut_at_centre and f.gap and f.max_ranges_used >= 3


def test_shuffling_carries_the_entries():
    g, ent, rv = cell("centre-1")
    h, newid = P.shuffled(g, seed=11)
    ent_h, rv_h = R.rect_local(h)
    want_rv = np.empty_like(rv)
    want_rv[newid] = rv
    assert np.array_equal(ent_h, P.entries_to(g, newid, ent)) and np.array_equal(rv_h, want_rv)
    d, did = P.degree_copy(g)
    assert bool((np.diff(np.diff(d.row_ptr)) >= 0).all())  # ascending in degree
    assert np.array_equal(R.rect_local(d)[0], P.entries_to(g, did, ent))


def test_constants_and_the_python_mirror():
    import graphminer_amd
    from graphminer_amd import _lib

    c = consts()
    print(f"constants: {c}", flush=True)
    assert c["range"] % 4 == 0 and 16 <= P.SMALL_RANGE < c["range"] and c["one_task"] % 64 == 0 and 1 < c["long_row"] <= c["range"]
    assert "rect_local" in graphminer_amd.__all__ and callable(graphminer_amd.rect_local)
    assert any(name == "gm_rect_local" for name, _, _ in _lib.SYMBOLS)
    assert hasattr(_lib.load(), "gm_rect_local")
