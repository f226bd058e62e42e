"""The batch graphs of tests/test_gpu_tch_flat_groups.py hold what they promise (no GPU): for every (M, ell) of
tests/flat_group_cases.py the 64 * ell flattened positions of a batch land where the case says -- worked out from the kernel's group and
window sizes --, and the graph is the batch graph tests/test_probe_graphs_host.py checks for the lengths of the existing suite: every
streamed list has exactly `ell` keys with its match at position 0 or ell - 1, one host alone in its chunk, and the oracle's triangle,
diamond and 4-clique counts are the expected ones."""
import pytest

import flat_group_cases as FG
import test_probe_graphs_host as H


@pytest.mark.parametrize("M,ell", FG.PARAMS)
def test_case_lands_where_it_says(M, ell):
    assert FG.where(M, ell) == FG.CASES[M][ell]
    assert 33 <= ell < 384  # the flattened pass: beyond the key stream, below the one-list-at-a-time limit (GM_TC_INLINE_MAX, kTchLongList)


def test_cases_cover_the_switches():
    for M in FG.CASES:
        got = set(FG.CASES[M].values())
        assert {"group boundary", "one tile short of a group", "one tile past a group"} <= got
        assert any("short of the window" in s for s in got) and any("past the window" in s for s in got)


@pytest.mark.parametrize("M,ell", FG.PARAMS)
def test_batch_lists(M, ell):
    H.test_batch_lists(M, ell)  # (rows, streamed lists, match positions, chunk table, oracle counts)
