"""The six 5-vertex closed forms without a GPU: the library exports gm_sgl5_raw / gm_sgl5_finish, gm_sgl5_finish applied to the numpy raw
sums of the small golden graphs gives tests/golden/sgl5.json (from the reference's sgl_omp_base), the plain-Python restatement of the
reference's loop nests gives the same, and the closed forms hold modulo 2^64."""
import ctypes as C
import functools
import json
import os

import pytest

import sgl5_ref as R5
from common import ROOT, load_graph
from graphminer_amd import _lib
from graphminer_amd.solvers import SGL5_PATTERNS, SGL5_RAW, sgl5_finish

with open(os.path.join(ROOT, "tests", "golden", "sgl5.json")) as f:
    SGL5 = json.load(f)
SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]
M64 = 2**64


@functools.lru_cache(maxsize=None)
def numpy_raw(name):
    return R5.raw_sums(load_graph(name))


def test_exports_and_order():
    lib = _lib.load()
    assert lib.gm_sgl5_raw and lib.gm_sgl5_finish and lib.gm_sgl5_raw_need
    raw = (C.c_uint64 * len(R5.RAW))()
    assert lib.gm_sgl5_raw_need(None, 1, None, raw, None) == _lib.GM_ERR_INVALID  # (the refusals with a handle: tests/test_gpu_sgl5.py)
    assert tuple(SGL5_RAW) == R5.RAW and set(SGL5_PATTERNS) == set(R5.PATTERNS)


def test_golden_has_the_issue_figures():
    want = {"hourglass": 16034, "taileddiamond": 83073, "taileddiamond2": 110576, "closedhouse": 11176, "semihouse": 22629, "5path": 1708895}
    assert {p: SGL5["citeseer"][p] for p in want} == want


@pytest.mark.parametrize("name", SMALL)
def test_finish_of_numpy_raw_is_golden(name):
    raw = numpy_raw(name)
    for pat in R5.PATTERNS:
        got = sgl5_finish(pat, [raw[k] for k in R5.RAW])
        print(name, pat, got, SGL5[name][pat], flush=True)
        assert got == SGL5[name][pat] == R5.finish(pat, raw), (name, pat)


@pytest.mark.parametrize("name", ["rmat6_ef4_s1", "citeseer"])
@pytest.mark.parametrize("pat", R5.PATTERNS)
def test_loop_restatement_is_golden(name, pat):
    assert R5.loops(load_graph(name), pat) == SGL5[name][pat]


def test_finish_unknown_name():
    lib, total = _lib.load(), C.c_uint64(7)
    raw = (C.c_uint64 * len(R5.RAW))()
    for name in (b"6path", b"dumbbell", b"diamond", b"all", b""):
        assert lib.gm_sgl5_finish(name, raw, C.byref(total)) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl5_finish(b"hourglass", None, C.byref(total)) == _lib.GM_ERR_INVALID
    assert lib.gm_sgl5_finish(b"hourglass", raw, None) == _lib.GM_ERR_INVALID


def test_finish_wraps_modulo_2_64():
    # the true H = 2^64 + 10 and D = 2^63 + 2 arrive reduced: H < 2 D modulo 2^64, and hourglass = H - 2 D = 6 all the same
    raw = dict.fromkeys(R5.RAW, 0)
    raw.update(H=(2**64 + 10) % M64, D=2**63 + 2)
    assert raw["H"] < (2 * raw["D"]) % M64 or raw["H"] < 2 * raw["D"]
    assert sgl5_finish("hourglass", [raw[k] for k in R5.RAW]) == 6
    # every term of 5path wrapped: P - 2 S + 9 T - 4 R
    raw = dict(zip(R5.RAW, [2**62 + 1, 0, 0, 5, 9, 0, 2**63 + 3, 11, 2**60, 2**62 + 2, 0]))
    want = (raw["P"] - 2 * raw["S"] + 9 * raw["T"] - 4 * raw["R"]) % M64
    assert sgl5_finish("5path", [raw[k] for k in R5.RAW]) == want
    assert sgl5_finish("taileddiamond", [raw[k] for k in R5.RAW]) == (raw["A"] - 12 * raw["K4"]) % M64
    assert sgl5_finish("semihouse", [raw[k] for k in R5.RAW]) == (raw["B"] - 12 * raw["K4"]) % M64
