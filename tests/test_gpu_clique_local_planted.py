"""Local k-clique counts on the GPU (gm_clique_local, csrc/gm_kcl_local.hip) on planted-clique graphs (tests/planted_cliques.py): graphs
whose root rows have a chosen length -- on both sides of every row length at which the kernel changes path -- and whose entries carry
hundreds of different values, known entry by entry.  A pair credited to the wrong entry of the right row, a descent that reads a
neighbouring matrix row, a search that lands on a wrong position: each of them changes an entry here, where a complete graph hides it.

  A  lane per pair (kcl_local_kernel<K, false>): rows around kcl_local_regs2_row at k = 3 .. 8, up to kcl_local_split_row at k = 5, 6, 8
     (the 8-register descent), around regs8 / regs12 / lds_row at k = 3, 4
  B  wave per pair (kcl_local_kernel<K, true>): rows from split_row + 1 to lds_row at k = 5, 6, 8, sets of 8, 12 and 16 registers; a
     complete block of 70 whose pairs need a second deal round
  C  wide kernel: rows of lds_row + 1, 2048, 2049 and 2060 entries at k = 3 .. 6 (k = 8: lds_row + 1 only), scattered
  D  roots of 100, 300, 513 and 1100 entries in one call at k = 5: all three kernels, both lists, a scratch slot used twice
  E  kcl_wave_find on rows of 64, 65 and 200 entries with the tops' ids below, between and above the H ids, under a split and a wide
     root; roots of 8 entries whose H vertices have rows of more than 32: the second branch of the matrix build

Every case runs the default copy and the graph as numbered (tune[6] & 0x200), asserts that the DAG's longest row lies between the constants
(gm_constant) its path needs, and prints every figure before it asserts.  tests/test_planted_cliques_host.py checks the expected values
and the conditions on the inputs on the CPU.  GM_PLANTED_MS_JSON=<file>: the kernel_ms of the cells that ran are merged
into that file (profiles/clique_local_planted_ms.json)."""
import json
import os

import numpy as np
import pytest

import planted_cliques as P
from common import kcl_row_constants
from graphminer_amd import clique_local

pytestmark = pytest.mark.gpu
AS_NUMBERED = 0x200


def t6(x):
    return [0, 0, 0, 0, 0, 0, x]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return 0


@pytest.fixture(scope="module")
def ms_log():
    log = {}
    yield log
    path = os.environ.get("GM_PLANTED_MS_JSON")
    if path:
        cells = {}
        if os.path.exists(path):  # (a run of some cells replaces their figures and keeps the others)
            with open(path) as f:
                cells = json.load(f).get("cells", {})
        cells.update(log)
        with open(path, "w") as f:
            json.dump({"unit": "gm_stats.kernel_ms of one call", "cells": cells}, f, indent=1, sort_keys=True)
            f.write("\n")


def differ(label, got, want, g=None):
    """prints the comparison; returns whether the arrays differ"""
    got, want = np.asarray(got), np.asarray(want)
    same_kind = got.dtype == want.dtype and got.shape == want.shape
    bad = np.flatnonzero(got != want) if same_kind else np.arange(0)
    where = ""
    if g is not None and bad.size:  # entries: the row and the neighbour of the first that differ
        src = np.searchsorted(g.row_ptr, bad[:5], side="right") - 1
        where = f" = entries {[(int(s), int(g.col_idx[e]), int(e - g.row_ptr[s])) for s, e in zip(src, bad[:5])]} (row, neighbour, position)"
    print(f"{label}: {want.size} values, dtype/shape ok {same_kind}, {bad.size} differ, first at {bad[:5].tolist()}{where}: "
          f"got {got[bad[:5]].tolist()} want {want[bad[:5]].tolist()}", flush=True)
    return (not same_kind) or bad.size > 0


@pytest.mark.parametrize("cell", P.CELLS, ids=[c.name for c in P.CELLS])
def test_cell(dev, ms_log, cell):
    consts = kcl_row_constants()
    g = P.cell_graph(cell, tuple(sorted(consts.items())))
    print(f"{cell.name}: {g.nv} vertices, {g.col_idx.size} entries, roots {g.root_rows()[:6]}, DAG max row {g.max_row}, above "
          f"{[(n, consts[n]) for n in cell.above]}, up to {[(n, consts[n]) for n in cell.upto]}", flush=True)
    # the cell sits where it claims, wherever the constants are
    assert all(g.max_row > consts[n] for n in cell.above) and all(g.max_row <= consts[n] for n in cell.upto)
    if cell.special == "mixed":
        rows = P.mixed_rows(consts)
        assert sorted(g.root_rows()) == sorted(rows) and rows[0] <= consts["split"] < rows[1] <= consts["lds"] < rows[2] < rows[3]
    elif cell.special != "branch":
        assert g.root_rows() == [consts[cell.base] + cell.off] and g.max_row == g.root_rows()[0]
    failed = []
    with g.graph.to_device(dev) as sym:
        for k in cell.ks:
            want_ent, want_kv, want_total, _ = g.expected(k)
            for tune, how in ((None, "default"), (t6(AS_NUMBERED), "as numbered")):
                total, kv, ent, st = clique_local(sym, k, tune=tune, return_stats=True)
                label = f"{cell.name} k={k} {how}"
                print(f"{label}: kernel_ms {st.kernel_ms}", flush=True)
                ms_log[label] = round(float(st.kernel_ms), 4)
                bad = [differ(f"{label} entries", ent, want_ent, g), differ(f"{label} K_v", kv, want_kv)]
                print(f"{label} total: got {total} want {want_total}", flush=True)
                if any(bad) or total != want_total:
                    failed.append(label)
    assert not failed, failed
