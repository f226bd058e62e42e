"""gm_kernel_times / gm_corner_times report the launches of the most recent CALL on a handle, whichever handle they ran on: a DAG pattern runs
on the cached topological copy, the SgL map solvers on a copy renumbered by degree, the one-GPU diamond on the oriented copy's topological copy,
the 4-motif on three handles at once.  bench.py takes every kernel time it reports through these two calls.

The relation pinned for every synchronous one-rank call: kernel_times_ms(1)[0] and the call's gm_stats.kernel_ms are both double sums of the
same one to three float HIP-event durations, so they differ by summation order at most -- far below 1e-6 ms for durations under 10^4 ms."""
import numpy as np
import pytest

from common import load_graph
from graphminer_amd import CliqueSolver, MotifSolver, SglSolver, TCSolver
from graphminer_amd.solvers import diamond_support_finish, diamond_support_partial, diamond_support_size

pytestmark = pytest.mark.gpu
PER_EDGE = [0, 0, 0, 0, 0, 0, 0x10000000]     # GM_T6_PER_EDGE
AS_NUMBERED = [0, 0, 0, 0, 0, 0, 0x200]       # GM_T6_AS_NUMBERED
TOL_MS = 1e-6
GRAPHS = ["rmat8_ef8_s42", "cora"]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    return 0


@pytest.fixture(scope="module", params=GRAPHS)
def graph(request):
    return load_graph(request.param)


def _same_call(label, handle, stats):
    """the handle's most recent entry of gm_kernel_times is the time the call itself reported"""
    got = handle.kernel_times_ms(1)
    print(f"{label}: kernel_times_ms(1) = {got}, stats.kernel_ms = {stats.kernel_ms!r}", flush=True)
    assert len(got) == 1 and stats.kernel_ms > 0.0, label
    assert abs(got[0] - stats.kernel_ms) <= TOL_MS, (label, got[0], stats.kernel_ms)


def test_dag_patterns_run_on_a_copy_that_differs(dev, graph):
    """the alias chain is really exercised: the topological copy is not the oriented graph as given"""
    with graph.to_device(dev) as sym, sym.orient() as dag:
        given, copy = dag.download(), dag.renumbered(2)
        assert given.V() == copy.V() and given.E() == copy.E()
        assert not (np.array_equal(given.row_ptr, copy.row_ptr) and np.array_equal(given.col_idx, copy.col_idx))


def test_tc_and_cliques_on_the_oriented_handle(dev, graph):
    with graph.to_device(dev) as sym, sym.orient() as dag:
        _, st = TCSolver(dag, return_stats=True)
        _same_call("tc", dag, st)
        corner, whole = dag.corner_times_ms(1), dag.kernel_times_ms(1)
        print(f"tc: corner_times_ms(1) = {corner}", flush=True)
        assert len(corner) == 1 and 0.0 <= corner[0] <= whole[0]
    for k in (4, 5):
        with graph.to_device(dev) as sym, sym.orient() as dag:
            _, st = CliqueSolver(dag, k, return_stats=True)
            _same_call(f"clique k={k}", dag, st)


@pytest.mark.parametrize("k,tune", [(3, None), (3, PER_EDGE), (4, None)], ids=["motif3", "motif3-per-edge", "motif4"])
def test_motifs_on_the_symmetric_handle(dev, graph, k, tune):
    with graph.to_device(dev) as sym:
        _, st = MotifSolver(sym, k, tune=tune, return_stats=True)
        _same_call(f"motif k={k} tune={tune}", sym, st)


@pytest.mark.parametrize("pattern", ["diamond", "rectangle", "house", "pentagon"])
def test_sgl_patterns_on_the_symmetric_handle(dev, graph, pattern):
    with graph.to_device(dev) as sym:
        _, st = SglSolver(sym, pattern, return_stats=True)
        _same_call(pattern, sym, st)


def test_diamond_support_partial_then_finish(dev, graph):
    import torch

    with graph.to_device(dev) as sym:
        n = diamond_support_size(sym, 1)
        buf = torch.empty(n, dtype=torch.int32, device=f"cuda:{dev}")
        st = diamond_support_partial(sym, buf.data_ptr(), n, return_stats=True)
        _same_call("diamond_support_partial", sym, st)
        total, st = diamond_support_finish(sym, buf.data_ptr(), n, return_stats=True)
        _same_call("diamond_support_finish", sym, st)
        assert total == SglSolver(sym, "diamond")


def test_no_stale_alias_across_calls_on_one_handle(dev, graph):
    """rectangle (degree copy), diamond (oriented copy -> topological copy), TC on the oriented copy, rectangle on the graph as numbered:
    after each call the handle's most recent time is that call's, not one an earlier call's alias still points at"""
    with graph.to_device(dev) as sym, sym.orient() as dag:
        want = SglSolver(sym, "rectangle", tune=AS_NUMBERED)
        seen = []
        for label, handle, call in (
            ("rectangle", sym, lambda: SglSolver(sym, "rectangle", return_stats=True)),
            ("diamond", sym, lambda: SglSolver(sym, "diamond", return_stats=True)),
            ("tc", dag, lambda: TCSolver(dag, return_stats=True)),
            ("rectangle as numbered", sym, lambda: SglSolver(sym, "rectangle", tune=AS_NUMBERED, return_stats=True)),
        ):
            total, st = call()
            _same_call(label, handle, st)
            seen.append((label, total))
        assert seen[0][1] == seen[3][1] == want
