"""One window of gm_tc_list / gm_clique_list with guard words on BOTH sides (test helper of tests/test_gpu_list.py and
tests/test_gpu_clique_list.py).  The fill kernels walk rows that lie before the window -- list_kernel<true> a whole batch from its first
slot, KclListRing up to 127 queued rows -- and only the lower clip of their flush keeps those rows out of the caller's memory.  A buffer
that starts at the window cannot see a write in front of it: here the window lies in the middle of a buffer pre-filled with a sentinel no
id can equal, and everything around the rows the call reports is asserted to be untouched."""
from __future__ import annotations

import ctypes as C

import numpy as np

U64_MAX = 2**64 - 1


def tc_call(sym):
    """gm_tc_list of a handle as call(first, cap, ptr) -> (status, total, n_written)"""
    from graphminer_amd import _lib

    def call(first, cap, ptr):
        total, written = C.c_uint64(99), C.c_uint64(99)
        rc = _lib.load().gm_tc_list(sym.handle, None, first, cap, ptr, C.byref(total), C.byref(written), None)
        return rc, int(total.value), int(written.value)

    call.device = sym.device
    return call


def clique_call(sym, k):
    """gm_clique_list of (handle, k) as call(first, cap, ptr) -> (status, total, n_written)"""
    from graphminer_amd import _lib

    def call(first, cap, ptr):
        total, written = C.c_uint64(99), C.c_uint64(99)
        rc = _lib.load().gm_clique_list(sym.handle, k, None, first, cap, ptr, C.byref(total), C.byref(written), None)
        return rc, int(total.value), int(written.value)

    call.device = sym.device
    return call


def out_list(g, u):
    """N+(u) of the orientation by (degree, id), ascending ids: the row of u in the oriented copy as numbered (plain numpy)"""
    rp, col = np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.col_idx, dtype=np.int64)
    deg = np.diff(rp)
    nu = col[rp[u]:rp[u + 1]]
    return np.sort(nu[(deg[nu] > deg[u]) | ((deg[nu] == deg[u]) & (nu > u))])


def root_boundaries(g, keys, root):
    """Where the rows of one root, of its entries and of its pairs start in a k-clique list (k >= 4) whose order keys are `keys`
    (clique_list_ref.order_keys of the pinned list: root, then the other members ascending -- the first of them is the entry, the first two
    the pair).  Returns (bounds, exact, info): bounds [(label, slot)] -- the slots a window should start and end on; exact [(label, first,
    cap)] -- the windows of exactly the root, its fattest entry and its fattest pair; info: what the caller asserts on (the pair whose
    second position lies in a later 64-position chunk of the root's row than its first, behind an earlier pair of the same entry)."""
    sel = np.flatnonzero(keys[:, 0] == root)
    assert sel.size and sel[-1] - sel[0] + 1 == sel.size, "the rows of a root are consecutive"
    r0, r1 = int(sel[0]), int(sel[-1]) + 1
    kk = keys[r0:r1]
    e_start = r0 + np.flatnonzero(np.r_[True, kk[1:, 1] != kk[:-1, 1]])
    e_end = np.r_[e_start[1:], r1]
    p_start = r0 + np.flatnonzero(np.r_[True, (kk[1:, 1:3] != kk[:-1, 1:3]).any(axis=1)])
    p_end = np.r_[p_start[1:], r1]
    L = out_list(g, root)
    pos_i, pos_l = np.searchsorted(L, keys[p_start, 1]), np.searchsorted(L, keys[p_start, 2])
    assert np.array_equal(L[pos_i], keys[p_start, 1]) and np.array_equal(L[pos_l], keys[p_start, 2]) and bool((pos_i < pos_l).all())
    fe = int(np.argmax(e_end - e_start))
    in_fe = np.flatnonzero((p_start >= e_start[fe]) & (p_start < e_end[fe]))
    fp = int(np.argmax(p_end - p_start))
    bounds = [("the root's first slot", r0), ("the slot behind the root", r1)]
    bounds += [(f"the root's {w} entry", int(e_start[j])) for w, j in (("first", 0), ("median", len(e_start) // 2), ("last", len(e_start) - 1))]
    bounds += [(f"the fattest entry's {w} pair", int(p_start[in_fe[j]])) for w, j in (("first", 0), ("median", len(in_fe) // 2), ("last", len(in_fe) - 1))]
    # a pair (i, l) with l in a later chunk than i, not the first pair of its entry; if there is one, one whose entry starts in an earlier
    # chunk than l (the chunk's carried base is not the entry's first slot)
    first_of_entry = np.searchsorted(e_start, p_start, side="right") - 1  # the entry of every pair
    entry_first_pair = np.searchsorted(p_start, e_start[first_of_entry])
    later = np.flatnonzero((pos_l // 64 > pos_i // 64) & (p_start > e_start[first_of_entry]))
    carried = later[pos_l[entry_first_pair[later]] // 64 < pos_l[later] // 64]
    cross = int(carried[len(carried) // 2]) if carried.size else (int(later[len(later) // 2]) if later.size else -1)
    info = {"rows": r1 - r0, "entries": len(e_start), "pairs": len(p_start), "row": len(L), "fattest entry": int(e_end[fe] - e_start[fe]),
            "pairs of the fattest entry": len(in_fe), "fattest pair": int(p_end[fp] - p_start[fp]), "cross pairs": int(later.size),
            "cross pairs behind a carried base": int(carried.size)}
    if cross >= 0:
        bounds.append(("a pair in a later chunk than its entry", int(p_start[cross])))
        info["cross pair"] = (int(pos_i[cross]), int(pos_l[cross]), int(p_start[cross] - e_start[first_of_entry[cross]]))
    for step in (64, 128):
        if p_end[fp] - p_start[fp] >= step:
            bounds.append((f"{step} rows into the fattest pair", int(p_start[fp]) + step))
    exact = [("exactly the root", r0, r1 - r0), ("exactly the fattest entry", int(e_start[fe]), int(e_end[fe] - e_start[fe])),
             ("exactly the fattest pair", int(p_start[fp]), int(p_end[fp] - p_start[fp]))]
    return bounds, exact, info


def guarded_window(call, k, first, cap, pad=1024, sentinel=-7, rows=None):
    """call(first, cap, ptr) into the middle of an int32 device buffer of pad + k * rows + pad ints filled with the sentinel (rows: the rows
    the caller's buffer holds, `cap` unless the cap is larger than anything that can be allocated).  Returns (rc, total, n_written, the
    n_written rows as int32[n_written, k]) after asserting that both pads are still all sentinel, that exactly k * n_written ints of the
    middle changed and that the ints behind row n_written are still sentinel."""
    import torch

    rows = cap if rows is None else rows
    assert 0 <= rows < 2**40 and pad >= 0 and sentinel < 0, (rows, pad, sentinel)
    buf = torch.full((pad + k * rows + pad,), sentinel, dtype=torch.int32, device=f"cuda:{getattr(call, 'device', 0)}")
    rc, total, n = call(first, cap, buf.data_ptr() + 4 * pad)
    host = buf.cpu().numpy()
    front, mid, back = host[:pad], host[pad:pad + k * rows], host[pad + k * rows:]
    where = f"window first={first} cap={cap} rows={rows} k={k}: rc {rc} total {total} n_written {n}"
    hit = np.flatnonzero(front != sentinel)
    assert hit.size == 0, f"{where}: {hit.size} ints IN FRONT of the window were written, the nearest {pad - int(hit[-1])} ints before it"
    hit = np.flatnonzero(back != sentinel)
    assert hit.size == 0, f"{where}: {hit.size} ints BEHIND the buffer were written, the nearest {int(hit[0])} ints behind it"
    assert n <= rows, f"{where}: more rows reported than the buffer holds"
    changed = int((mid != sentinel).sum())
    assert changed == k * n, f"{where}: {changed} ints of the window changed, {k * n} expected"
    assert bool((mid[k * n:] == sentinel).all()), f"{where}: ints behind row {n} were written"
    return rc, total, n, mid[:k * n].reshape(-1, k).copy()
