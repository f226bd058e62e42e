"""The rule that chooses which pairs of 256-row blocks (IB <= JB) of the hub corner the triangle count's masked product takes
(gm_tc_pair_rule, gm_tasks.hip): a pair is taken iff  keys * R > 65536 * (region - 512 * (JB >> 1))  -- the keys the stream would move for
the pair's edges, R bit-products a key, against the bit-products of the pair's column range.  CPU only: the exported host function against a
restatement in Python integers, on random cell tables."""
import numpy as np
import pytest

from graphminer_amd.solvers import tc_pair_rule

NBS = [2, 3, 6, 128]
HUGE_R = 1 << 62


def _cells(nb, seed):
    """random cells up to the 32-bit range a pair can reach (65536 edges x 2048 keys), a third of them empty, the lower triangle filled too
    (the rule must not look at it)"""
    rng = np.random.default_rng(seed)
    keys = (2.0 ** rng.uniform(0, 27, (nb, nb))).astype(np.uint32)
    keys[rng.random((nb, nb)) < 0.33] = 0
    return keys


def _restated(keys, nb, region, R):
    sel = np.zeros((nb, nb), dtype=bool)
    for ib in range(nb):
        for jb in range(ib, nb):
            sel[ib, jb] = int(keys[ib, jb]) * R > 65536 * (region - 512 * (jb >> 1))
    return sel


def _region(nb):
    return 256 * nb


@pytest.mark.parametrize("nb", NBS)
def test_rule_equals_its_restatement(nb):
    keys = _cells(nb, 100 + nb)
    for R in (1, 1250, 2480, 2500, 5000, 10 ** 6, HUGE_R):
        got = tc_pair_rule(keys, nb, _region(nb), R)
        assert np.array_equal(got, _restated(keys, nb, _region(nb), R)), (nb, R)


@pytest.mark.parametrize("nb", NBS)
def test_only_upper_pairs_never_an_empty_cell_monotone_in_R_and_everything_at_a_huge_R(nb):
    keys = _cells(nb, 200 + nb)
    upper = np.triu(np.ones((nb, nb), dtype=bool))
    prev = None
    for R in (HUGE_R, 10 ** 9, 5000, 2500, 2480, 1250, 100, 1, 0):  # falling
        sel = tc_pair_rule(keys, nb, _region(nb), R)
        assert not (sel & ~upper).any()      # only IB <= JB
        assert not (sel & (keys == 0)).any()  # an empty cell is never taken
        if prev is not None:
            assert not (sel & ~prev).any(), R  # the selection shrinks as R falls
        prev = sel
    assert np.array_equal(tc_pair_rule(keys, nb, _region(nb), HUGE_R), upper & (keys != 0))
    assert not tc_pair_rule(keys, nb, _region(nb), 0).any()


def test_a_cell_at_the_edge_of_the_rule():
    """keys * R == the pair's bit-products is NOT taken, one key more is (nb = 6: pair (1, 5) starts at chunk 2 of 3)"""
    nb, region, R = 6, 1536, 4096
    cost = 65536 * (region - 512 * (5 >> 1))
    assert cost % R == 0
    keys = np.zeros((nb, nb), dtype=np.uint32)
    keys[1, 5] = cost // R
    assert not tc_pair_rule(keys, nb, region, R).any()
    keys[1, 5] += 1
    sel = tc_pair_rule(keys, nb, region, R)
    assert sel[1, 5] and sel.sum() == 1


def test_invalid_arguments():
    """tables of the right size, so that the library's own checks answer: a region that is not 256 nb, no block, more blocks than the core
    bitmap has rows for"""
    for nb, region in ((2, 1024), (0, 0), (129, 129 * 256)):
        with pytest.raises(ValueError):
            tc_pair_rule(np.ones((nb, nb), dtype=np.uint32), nb, region, 2480)
