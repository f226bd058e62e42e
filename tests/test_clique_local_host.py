"""The plain Python reference of the local k-clique counts (tests/clique_local_ref.py) against the goldens of the reference binaries and
against closed forms -- no device needed.  The GPU tests compare the library with this reference, so it is checked first.  Every value is
printed before it is asserted."""
import functools
from math import comb

import numpy as np
import pytest

import clique_local_ref as R
import twin_graphs as T
from common import GOLDEN, load_graph

CASES = [(n, k) for n in ("citeseer", "cora", "rmat6_ef4_s1", "rmat8_ef8_s42") for k in range(3, 9)] + [("rmat10_ef16_s42", 4), ("rmat10_ef16_s42", 5)]


def golden(name, k):
    return GOLDEN[name]["tc"] if k == 3 else GOLDEN[name][f"clique{k}"]


@functools.lru_cache(maxsize=None)
def ref(name, k):
    g = load_graph(name)
    ent = R.entry_cliques(g, k)
    return g, ent, R.vertex_cliques(g, k, ent)


def check(label, got, want):
    print(f"{label}: got {got} want {want}", flush=True)
    assert got == want, label


def both_directions_equal(g, ent):
    src = np.repeat(np.arange(g.V(), dtype=np.int64), np.diff(g.row_ptr))
    dst = g.col_idx.astype(np.int64)
    o = np.argsort(np.minimum(src, dst) * g.V() + np.maximum(src, dst), kind="stable")
    return bool((ent[o][0::2] == ent[o][1::2]).all())


@pytest.mark.parametrize("name,k", CASES)
def test_reference_against_the_goldens(name, k):
    g, ent, kv = ref(name, k)
    check(f"{name} k={k} entry sum", sum(int(x) for x in ent), k * (k - 1) * golden(name, k))
    check(f"{name} k={k} vertex sum", sum(int(x) for x in kv), k * golden(name, k))
    check(f"{name} k={k} both directions", both_directions_equal(g, ent), True)
    assert ent.dtype == np.uint64 and ent.shape == (g.E(),) and kv.dtype == np.uint64 and kv.shape == (g.V(),)


@pytest.mark.parametrize("k", range(3, 9))
def test_closed_forms_complete_and_multipartite(k):
    n = 12
    g = T.graph("complete", (n,))
    ent = R.entry_cliques(g, k)
    check(f"K_{n} k={k} entries", np.unique(ent).tolist(), [comb(n - 2, k - 2)])
    check(f"K_{n} k={k} vertices", np.unique(R.vertex_cliques(g, k, ent)).tolist(), [comb(n - 1, k - 1)])
    r, s = 5, 3
    g = T.graph("multipartite", (r, s))
    ent = R.entry_cliques(g, k)
    check(f"K_{r}x{s} k={k} entries", np.unique(ent).tolist(), [comb(r - 2, k - 2) * s ** (k - 2)])
    check(f"K_{r}x{s} k={k} vertices", np.unique(R.vertex_cliques(g, k, ent)).tolist(), [comb(r - 1, k - 1) * s ** (k - 1)])


def test_apex_graph():
    p, s = 3, 4
    g, part = R.apex(p, s)
    want_ent, want_kv = R.apex_expected(g, part, p, s)
    ent = R.entry_cliques(g, p + 2)
    kv = R.vertex_cliques(g, p + 2, ent)
    check(f"A({p},{s}) entries", ent.tolist(), want_ent.tolist())
    check(f"A({p},{s}) vertices", kv.tolist(), want_kv.tolist())
    check(f"A({p},{s}) total", sum(int(x) for x in kv) // (p + 2), s ** p)
