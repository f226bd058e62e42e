"""tch_kernel's flattened pass (gm_tch.hip) at the places where it changes form: the full tile groups of a mark window run peeled (no
range test, no guarded selects), its last, partial group guarded, one group ahead in flight across the switch.  The batch graphs of
tests/probe_graphs.py put 64 equal lists into every batch, so 64 * ell names the place: a group boundary, one tile to either side of it,
the mark window to either side (tests/flat_group_cases.py; tests/test_probe_flat_groups_host.py confirms the places and the expected
counts against the CPU oracle).  Every comparison is exact.

Each case runs the triangle count with the tunes of tests/test_gpu_probe_lists.py and as rank shares of 3, on the narrow form of the
key addressing (32-bit byte offsets, DAGs below 2^30 entries) and -- developer option GM_TCH_WIDE_NE=0 -- on the exact form kept for
larger ones."""
import pytest

import flat_group_cases as FG
import probe_graphs as PG
from graphminer_amd import TCSolver

pytestmark = pytest.mark.gpu
AS_NUMBERED, FALLBACK, SORTED_COPY, PARTS = 0x200, 0x800000, 0x4000000, 0x1000
TC_TUNES = (0, AS_NUMBERED, AS_NUMBERED | FALLBACK, FALLBACK, SORTED_COPY, 0x20000000, PARTS)  # (those of test_gpu_probe_lists.py)


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def tc_every_way(label, dag, want):
    for t in TC_TUNES:
        check(f"{label} TCSolver tune[6]={t:#x}", TCSolver(dag, tune=t6(t)), want)
    for t in (0, AS_NUMBERED):
        check(f"{label} rank shares of 3, tune[6]={t:#x}", sum(TCSolver(dag, rank=r, world=3, tune=t6(t)) for r in range(3)), want)


@pytest.mark.parametrize("M,ell", FG.PARAMS)
def test_flat_groups(M, ell, devopt):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    p = PG.batch(M, ell)
    label = f"batch{M}_{ell} ({FG.CASES[M][ell]})"
    with p.graph.to_device(0) as sym:
        dag = sym.orient()
        tc_every_way(label, dag, p.tri_total)
        devopt("GM_TCH_WIDE_NE", "0")  # (read at every launch)
        tc_every_way(label + " wide form", dag, p.tri_total)
        devopt(None)
        dag.free()


@pytest.mark.parametrize("M,ell", [(1024, 37), (2048, 65)])
def test_either_side_of_the_limit(M, ell, devopt):
    """GM_TCH_WIDE_NE at the DAG's entry count (the WIDE instance: entries >= limit) and one above it (the narrow one): the same count;
    what the rule does with the numbers is tests/test_tch_rule_host.py's"""
    p = PG.batch(M, ell)
    with p.graph.to_device(0) as sym:
        dag = sym.orient()
        for limit in (dag.ne, dag.ne + 1):
            devopt("GM_TCH_WIDE_NE", str(limit))
            tc_every_way(f"batch{M}_{ell} GM_TCH_WIDE_NE={limit} (ne {dag.ne})", dag, p.tri_total)
        dag.free()


@pytest.mark.parametrize("M,ell", [(1024, 16), (2048, 32)])
def test_task_major_copies(M, ell, devopt):
    """A handle of more than 2^24 vertices cannot have the key stream: its lists of <= 32 keys are streamed, flattened, from task-major
    copies BEHIND col[] -- the indices the pass forms reach past the DAG's entry count, and the extent of that longer array chooses the
    addressing.  The batch graph padded with isolated vertices; the narrow form, the limit one above the DAG's entries (WIDE only
    because the copies count), and WIDE forced.  The lengths are those tests/test_probe_graphs_host.py confirms."""
    import numpy as np
    from graphminer_amd.graph import Graph

    p = PG.batch(M, ell)
    nv = (1 << 24) + 64
    rp = np.full(nv + 1, p.graph.row_ptr[-1], dtype=np.int64)
    rp[:p.graph.V() + 1] = p.graph.row_ptr
    g = Graph(row_ptr=rp, col_idx=p.graph.col_idx, name="probe-padded")
    with g.to_device(0) as sym:
        dag = sym.orient()
        tc_every_way(f"batch{M}_{ell} padded", dag, p.tri_total)
        for limit in (dag.ne + 1, 0):
            devopt("GM_TCH_WIDE_NE", str(limit))
            tc_every_way(f"batch{M}_{ell} padded GM_TCH_WIDE_NE={limit}", dag, p.tri_total)
        dag.free()


@pytest.mark.parametrize("name", ["s1024:tiles:flat", "s2048:tiles:flat", "s1024:tie:edge", "surplus"])
def test_wide_form_single_lists(name, devopt):
    """the exact form on single lists of every flattened length, matches on either side of every tile edge; the narrow form of these
    graphs is test_gpu_probe_lists.py's"""
    p = PG.surplus() if name == "surplus" else PG.single(*name.split(":"))
    devopt("GM_TCH_WIDE_NE", "0")
    with p.graph.to_device(0) as sym:
        dag = sym.orient()
        tc_every_way(f"{name} wide form", dag, p.tri_total)
        dag.free()
