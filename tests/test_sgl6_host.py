"""6path and dumbbell without a GPU: the closed forms of tests/sgl6_ref.py against the restated loop nests of the reference, the host-only
entry points gm_sgl6_need / gm_sgl6_finish against tests/golden/sgl6.json (the reference's sgl_omp_base) on the numpy raw sums, their
refusals, and the arithmetic modulo 2^64."""
import ctypes as C
import functools
import json
import os

import pytest

import sgl6_ref as R6
from common import ROOT, load_graph, random_graph
from graphminer_amd import _lib
from graphminer_amd.solvers import SGL6_PATTERNS, SGL6_RAW, sgl6_finish, sgl6_need

with open(os.path.join(ROOT, "tests", "golden", "sgl6.json")) as f:
    SGL6 = json.load(f)


@functools.lru_cache(maxsize=None)
def numpy_raw(name):
    return R6.raw_sums(load_graph(name))


def test_names_and_order():
    assert SGL6_PATTERNS == R6.PATTERNS and SGL6_RAW == R6.RAW


def small_graphs():
    yield "rmat6_ef4_s1", load_graph("rmat6_ef4_s1")
    for nv, ne, seed in ((9, 30, 1), (11, 40, 2), (12, 60, 3)):
        yield f"random{nv}_s{seed}", random_graph(nv, ne, seed)


@pytest.mark.parametrize("pattern", R6.PATTERNS)
def test_closed_forms_equal_the_loop_nests(pattern):
    for name, g in small_graphs():
        want = R6.loops(g, pattern)
        got = R6.finish(pattern, R6.raw_sums(g, need=R6.NEEDS[pattern]))
        print(f"{name} {pattern}: loops {want} closed form {got}", flush=True)
        assert got == want and want > 0, name


def test_loop_nests_equal_the_golden_of_the_small_rmat():
    for pattern in R6.PATTERNS:
        assert R6.loops(load_graph("rmat6_ef4_s1"), pattern) == SGL6["rmat6_ef4_s1"][pattern]


@pytest.mark.parametrize("name", ["citeseer", "cora", "rmat8_ef8_s42"])
def test_finish_on_numpy_raw_sums_equals_goldens(name):
    raw = numpy_raw(name)
    for pattern in R6.PATTERNS:
        got = sgl6_finish(pattern, [raw[k] for k in R6.RAW])
        print(f"{name} {pattern}: gm_sgl6_finish {got} golden {SGL6[name][pattern]}", flush=True)
        assert got == SGL6[name][pattern] == R6.finish(pattern, raw)


def test_goldens_hold_the_graphs_that_are_never_left_out():
    for name in ("citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42"):
        for pattern in R6.PATTERNS:
            assert isinstance(SGL6[name][pattern], int) and f"{name}:{pattern}" not in SGL6["_omitted"]


def test_analytic_values():
    import twin_graphs as T

    for n in (5, 6, 8):
        g = T.graph("complete", (n,))
        for pattern in R6.PATTERNS:
            assert R6.loops(g, pattern) == R6.complete_counts(n)[pattern] == R6.finish(pattern, R6.raw_sums(g, need=R6.NEEDS[pattern]))
    for a, b in ((2, 5), (3, 4)):
        raw = R6.raw_sums(T.graph("kab", (a, b)), need=("Z", "R", "C5"))
        assert {k: raw[k] for k in ("R", "Z", "C5")} == R6.kab_raw(a, b)


def test_need_masks():
    assert sgl6_need("6path") == R6.mask(("X", "Y", "Z", "R", "D", "C5")) == 0b000111111
    assert sgl6_need("dumbbell") == R6.mask(("M", "B", "K4")) == 0b111000000
    assert sgl6_need("all") == (1 << len(R6.RAW)) - 1


def test_refusals():
    lib = _lib.load()
    raw = (C.c_uint64 * len(R6.RAW))()
    for name in (b"diamond", b"hourglass", b""):
        mask, total = C.c_uint32(7), C.c_uint64(0)
        assert lib.gm_sgl6_need(name, C.byref(mask)) == _lib.GM_ERR_INVALID and mask.value == 0
        assert lib.gm_sgl6_finish(name, raw, C.byref(total)) == _lib.GM_ERR_INVALID
    total = C.c_uint64(0)
    assert lib.gm_sgl6_finish(b"all", raw, C.byref(total)) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_finish(b"6path", None, C.byref(total)) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_finish(b"6path", raw, None) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl6_need(b"6path", None) == _lib.GM_ERR_INVALID


def test_arithmetic_wraps_modulo_2_64():
    # X - Y - 2 Z is negative before the other terms are added
    raw = dict.fromkeys(R6.RAW, 0)
    raw.update(X=10, Y=2**63, Z=2**62 + 5, R=3, D=7, C5=11)
    want = (10 - 2**63 - 2 * (2**62 + 5) + 36 + 28 - 55) % 2**64
    assert 10 - 2**63 - 2 * (2**62 + 5) < 0
    assert sgl6_finish("6path", [raw[k] for k in R6.RAW]) == want == R6.finish("6path", raw)
    raw = dict.fromkeys(R6.RAW, 0)
    raw.update(M=5, B=2**64 - 1, K4=2**62)
    assert sgl6_finish("dumbbell", [raw[k] for k in R6.RAW]) == (5 - (2**64 - 1) + 6 * 2**62) % 2**64 == R6.finish("dumbbell", raw)
