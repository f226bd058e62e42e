"""Triangle count: the hub corner chosen per PAIR of 256-row blocks (tc_pairs_setup, gm_tasks.hip) -- the masked product (gm_ctc.hip) takes
the edges of the chosen pairs (IB <= JB) of a region at the end of the core bitmap, the key stream everything else.  Every triangle is
counted by its (smallest, middle) edge, so the total must equal the oracle's (omp_base.cc:15-21) for ANY set of pairs: every forced
selection, the rule, ranks' shares, the kernels without the stream (their corner stays row-based), the formula 3-motif and the diamond.

GM_TC_PAIRS / GM_TC_PAIR_R / GM_TC_PAIR_REGION / GM_TC_CORE_H / GM_TOPO_MIN_ROW are read when a handle's renumbered copy and key stream are
built: every case uploads a fresh graph."""
import numpy as np
import pytest

import oracle as O
from graphminer_amd import MotifSolver, SglSolver, TCSolver
from graphminer_amd.rmat import csr_from_pairs, rmat_csr_numpy
from graphminer_amd.solvers import tc_core_info, tc_pairs_info

pytestmark = pytest.mark.gpu

NO_STREAM = [0, 0, 0, 0, 0, 0, 0x20000000]  # the kernels without the key stream: every edge a task of the lists


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    return 0


def _want(g):
    return O.tc(O.orient(O.OGraph(g.row_ptr, g.col_idx)))


@pytest.fixture(scope="module")
def dense():
    """dense random, n = 1536, p = 0.3: as one region nb = 6 blocks and nc = 3 chunks (an odd chunk count: the pairs of JB = 4, 5 start at
    the last chunk, those of JB = 2, 3 at the middle one)"""
    n, p = 1536, 0.3
    rng = np.random.default_rng(1536)
    s, d = np.triu_indices(n, 1)
    keep = rng.random(s.size) < p
    g = csr_from_pairs(n, s[keep].astype(np.uint64), d[keep].astype(np.uint64))
    return g, _want(g)


@pytest.fixture(scope="module")
def rmat14():
    g = rmat_csr_numpy(14, 24, seed=14)
    return g, _want(g)


def _check_counts(dag, want, worlds=(2, 3)):
    got, st = TCSolver(dag, return_stats=True)
    assert got == want, (got, want, tc_pairs_info(dag), tc_core_info(dag))
    assert st.tasks == dag.E()
    assert TCSolver(dag) == want  # again: the dequeue word and the counters are zeroed by every launch
    assert TCSolver(dag, tune=NO_STREAM) == want
    for world in worlds:  # a rank takes every world-th entry of the product's list and its share of the chunks
        parts = [TCSolver(dag, rank=r, world=world, return_stats=True) for r in range(world)]
        assert sum(c for c, _ in parts) == want, (world, [c for c, _ in parts])
        assert sum(t.tasks for _, t in parts) == dag.E()


@pytest.mark.parametrize("mode", ["all", "none", "checker", "diag", "offdiag", "rule"])
def test_every_forced_selection_on_a_small_dense_graph(dev, dense, mode, devopt):
    g, want = dense
    devopt("GM_TOPO_MIN_ROW", "0")  # renumber whatever the mean row
    devopt("GM_TC_PAIR_REGION", str(g.V()))  # the whole graph is the region
    devopt("GM_TC_PAIRS", mode)
    nb = g.V() // 256
    with g.to_device(dev) as s, s.orient() as dag:
        _check_counts(dag, want)
        pi = tc_pairs_info(dag)
        assert pi["region"] == g.V() and pi["pairs_possible"] == nb * (nb + 1) // 2, pi  # p = 0.3: every pair holds edges with keys
        taken = {"all": nb * (nb + 1) // 2, "none": 0, "checker": sum((i + j) % 2 for i in range(nb) for j in range(i, nb)),
                 "diag": nb, "offdiag": nb * (nb - 1) // 2}
        if mode in taken:
            assert pi["pairs"] == taken[mode], pi
        else:
            assert 0 <= pi["pairs"] <= pi["pairs_possible"] and pi["R"] == 2480, pi
        if mode == "all":
            assert pi["pairs"] == pi["pairs_possible"] and pi["edges"] == dag.E(), pi
        if mode == "none":  # the count came from the stream alone
            assert pi["pairs"] == 0 and pi["edges"] == 0 and pi["keys_moved"] == 0, pi
        assert (pi["edges"] > 0) == (pi["pairs"] > 0) == (pi["keys_moved"] > 0)


def test_complete_graph_checkerboard(dev, devopt):
    """K_512: nb = 2, only the pair (0, 1) is in the product, both diagonal blocks in the stream -- C(512, 3)"""
    devopt("GM_TOPO_MIN_ROW", "0")
    devopt("GM_TC_PAIR_REGION", "512")
    devopt("GM_TC_PAIRS", "checker")
    n = 512
    iu, ju = np.triu_indices(n, 1)
    g = csr_from_pairs(n, iu.astype(np.uint64), ju.astype(np.uint64))
    with g.to_device(dev) as s, s.orient() as dag:
        _check_counts(dag, n * (n - 1) * (n - 2) // 6, worlds=(2,))
        pi = tc_pairs_info(dag)
        assert pi["region"] == 512 and pi["pairs"] == 1 and pi["edges"] == 256 * 256, pi


@pytest.mark.parametrize("mode", ["rule", "checker"])
def test_rmat14_default_region_and_the_formula_motif(dev, rmat14, mode, devopt):
    """R-MAT-14 ef 24: the density rule names a base corner, the region is the last quarter of the vertices; gm_tc_core_info keeps describing
    the base corner"""
    g, want = rmat14
    infos = {}
    for m in ("off", mode):
        devopt("GM_TOPO_MIN_ROW", "0")
        devopt("GM_TC_PAIRS", m)
        with g.to_device(dev) as s, s.orient() as dag:
            if m == "off":
                assert TCSolver(dag) == want
            else:
                _check_counts(dag, want)
            infos[m] = (tc_core_info(dag), tc_pairs_info(dag))
            wedges_tri = MotifSolver(s, 3, formula=True)
            assert wedges_tri[1] == want
            assert MotifSolver(s, 3) == wedges_tri
    assert infos["off"][0] == infos[mode][0], infos
    assert infos["off"][0]["h"] > 0, infos  # (R-MAT-14's hubs are dense: without a base corner nothing here would be tested)
    assert infos["off"][1]["region"] == 0 and infos["off"][1]["pairs"] == 0, infos
    pi = infos[mode][1]
    assert pi["region"] == g.V() // 4 and 0 < pi["pairs"] <= pi["pairs_possible"], infos


def test_region_that_is_no_multiple_of_512(dev, devopt):
    """a graph of 2050 vertices: core bitmap rows of 65 words, which the block kernel's 16-byte loads cannot walk -- no region, so no
    selection.  (core_h, region): a region of 512 rows, a valid size, is refused for the rows' width alone and, with no base corner,
    every edge stays in the stream; a region of 2050 is no multiple of 512; and the forced corner of the whole graph runs as a full
    triangle on the guarded kernel"""
    nv = 2050
    rng = np.random.default_rng(nv)
    m = nv * 40
    s_ = rng.integers(0, nv, m).astype(np.uint64)
    d_ = (rng.integers(0, nv, m) ** 2 // nv).astype(np.uint64)  # skewed targets: hubs
    g = csr_from_pairs(nv, s_, d_)
    want = _want(g)
    for core_h, region in ((None, 512), (None, nv), ("32768", nv)):
        devopt("GM_TOPO_MIN_ROW", "0")
        devopt("GM_TC_PAIRS", "all")
        devopt("GM_TC_PAIR_REGION", str(region))
        devopt("GM_TC_CORE_H", core_h)
        with g.to_device(dev) as s, s.orient() as dag:
            _check_counts(dag, want, worlds=(2,))
            assert tc_pairs_info(dag)["region"] == 0
            assert (tc_core_info(dag)["h"] > 0) == (core_h is not None)


def test_a_misspelt_option_is_an_error(dev, dense, devopt):
    """also on a graph that would get no selection: the option is checked before anything else"""
    from graphminer_amd._lib import GraphMinerError

    g, want = dense
    for name, value in (("GM_TC_PAIRS", "chequer"), ("GM_TC_PAIR_REGION", "all"), ("GM_TC_PAIR_R", "2k")):
        devopt(None)
        devopt("GM_TOPO_MIN_ROW", "0")
        devopt(name, value)
        with g.to_device(dev) as s, s.orient() as dag:
            with pytest.raises(GraphMinerError):
                TCSolver(dag)
    devopt(None)
    devopt("GM_TOPO_MIN_ROW", "0")
    with g.to_device(dev) as s, s.orient() as dag:
        assert TCSolver(dag) == want


def test_diamond_is_the_same_with_and_without_the_selection(dev, rmat14, devopt):
    g, _ = rmat14
    got = {}
    for m in ("off", "rule"):
        devopt("GM_TOPO_MIN_ROW", "0")
        devopt("GM_TC_PAIRS", m)
        with g.to_device(dev) as s:
            got[m] = SglSolver(s, "diamond")
    assert got["off"] == got["rule"] and got["off"] > 0, got
