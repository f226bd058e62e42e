"""Triangle listing, the part that needs no GPU: the plain numpy reference of tests/list_ref.py against the golden triangle counts, and
the ABI surface of gm_tc_list (declared, bound, refusing a null handle, mirrored as tc_list)."""
import numpy as np
import pytest

import graphminer_amd
from common import GOLDEN, load_graph
from graphminer_amd import _lib
from list_ref import list_ref

SMALL = ["citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42", "rmat10_ef16_s42"]


@pytest.mark.parametrize("name", SMALL)
def test_list_ref_matches_the_golden_counts(name):
    tri = list_ref(load_graph(name))
    print(f"{name}: {len(tri)} rows, golden {GOLDEN[name]['motif3'][1]}", flush=True)
    assert tri.dtype == np.int32 and tri.shape == (GOLDEN[name]["motif3"][1], 3)
    assert bool((tri[:, 0] < tri[:, 1]).all() and (tri[:, 1] < tri[:, 2]).all()), "every row ascending"
    assert len(np.unique(tri, axis=0)) == len(tri), "every row once"


def test_entry_point_is_bound():
    assert "gm_tc_list" in {s[0] for s in _lib.SYMBOLS}


def test_null_handle_is_refused():
    rc = _lib.load().gm_tc_list(None, None, 0, 0, None, None, None, None)
    print(f"gm_tc_list on a null handle: {rc}", flush=True)
    assert rc == _lib.GM_ERR_INVALID


def test_python_mirror_is_exported():
    assert "tc_list" in graphminer_amd.__all__ and callable(graphminer_amd.tc_list)
