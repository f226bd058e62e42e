"""tch_kernel (gm_tch.hip) on graphs whose streamed lists straddle its one-task-at-a-time threshold (kTchLongList, 384 keys; below it
the lists are flattened 64 to a batch, several mark windows per batch once a batch holds more than 8192 keys).  Dense random graphs
give DAG rows and streamed tails of roughly 100 .. 600 keys.  Triangle count and 3-motif against the CPU oracle:
  * on small ids and on ids just below 2^24 (the largest ids the key stream of the short lists can tag);
  * on ids chosen through the inverse of the bucket multiplier, so that every id of a row falls into one bucket per row: the surplus
    list overflows and every chunk is looked up by bisection in global memory; and with a few such ids per row, so that the surplus
    list is used without overflowing;
  * with the forced global-memory lookup (tune[6] & 0x800000), on the graph as numbered (0x200), split over ranks, and on the chunked
    sorted-copy kernel (0x4000000) as a second opinion."""
import numpy as np
import pytest

import oracle as O
from graphminer_amd import MotifSolver, TCSolver
from graphminer_amd.rmat import csr_from_pairs

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200
FALLBACK = 0x800000
SORTED_COPY = 0x4000000
MUL = 0x9E3779B1  # gm_tch.hip kTchMul


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


def _dense(n, p, seed):
    """Edge pairs (i < j) of a G(n, p) graph on the local ids 0 .. n-1."""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    return iu[keep].astype(np.uint64), ju[keep].astype(np.uint64)


def _one_bucket_ids(count):
    """Ids below 2^24 whose products with the multiplier share their top bits: one bucket per row salt."""
    cinv = pow(MUL, -1, 1 << 32)
    t = (np.uint64(5) << np.uint64(22)) + np.arange(1 << 22, dtype=np.uint64)
    x = (t * np.uint64(cinv)) & np.uint64(0xFFFFFFFF)
    pool = np.sort(x[(x < (1 << 24)) & (x > 0)])
    assert pool.size >= count
    return pool[np.linspace(0, pool.size - 1, count).astype(np.int64)]


def _check(g, dev, motif=True):
    osym = O.OGraph(g.row_ptr, g.col_idx)
    want = O.tc(O.orient(osym))
    assert want > 0
    sym = g.to_device(dev)
    dag = sym.orient()
    rows = np.diff(dag.download().row_ptr)
    assert rows.max() >= 384  # lists on both sides of the threshold
    assert TCSolver(dag) == want
    assert TCSolver(dag, tune=[0, 0, 0, 0, 0, 0, AS_NUMBERED]) == want
    assert TCSolver(dag, tune=[0, 0, 0, 0, 0, 0, AS_NUMBERED | FALLBACK]) == want
    assert TCSolver(dag, tune=[0, 0, 0, 0, 0, 0, FALLBACK]) == want
    assert TCSolver(dag, tune=[0, 0, 0, 0, 0, 0, SORTED_COPY]) == want
    assert sum(TCSolver(dag, rank=r, world=3, tune=[0, 0, 0, 0, 0, 0, AS_NUMBERED]) for r in range(3)) == want
    if motif:
        assert MotifSolver(sym, 3) == [int(x) for x in O.motif3(osym)]


@pytest.mark.parametrize("n,p", [(2500, 0.25), (1800, 0.4)])
def test_tc_mid_and_long_lists_small_ids(dev, n, p):
    s, d = _dense(n, p, seed=n)
    _check(csr_from_pairs(n, s, d), dev)


def test_tc_mid_and_long_lists_ids_near_2_24(dev):
    n = 2200
    s, d = _dense(n, 0.3, seed=7)
    base = np.uint64((1 << 24) - n)  # the largest id is 2^24 - 1
    _check(csr_from_pairs(1 << 24, s + base, d + base), dev)


def test_tc_mid_and_long_lists_all_ids_in_one_bucket(dev):
    n = 1600
    ids = _one_bucket_ids(n)
    s, d = _dense(n, 0.35, seed=5)
    _check(csr_from_pairs(1 << 24, ids[s], ids[d]), dev, motif=False)


def test_tc_mid_and_long_lists_surplus_list(dev):
    n = 2400
    rng = np.random.default_rng(9)
    ids = np.arange(100000, 100000 + n, dtype=np.uint64)
    few = rng.choice(n, size=12, replace=False)  # a dozen vertices of every row's neighbourhood collide
    ids[few] = _one_bucket_ids(12)
    s, d = _dense(n, 0.3, seed=9)
    _check(csr_from_pairs(1 << 24, ids[s], ids[d]), dev, motif=False)
